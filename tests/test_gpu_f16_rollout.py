"""The fp16 mode (``set_precision("f16")``) on the routes a rollout takes, against float64 (cases and references:
f16_rollout_cases.py; that they are in their regimes and tell right from wrong: test_f16_rollout_cases.py).

  1 sorted     gm_epd_forward on edge attributes in the csr's order -- the systolic edge encoder and the launches of a step as the
               fused forward schedules them -- in rule B's envelope (precision_cases: err = max |x - ref64| / max(max |ref64|, 1e-3),
               err(restatement) / 4 <= err(device) <= 4 err(restatement)); other bits than EncProcDecGNN.forward on the same edges;
               the same handle back at "f32" at the float32 parity bar
  2 steps      four RolloutEngine.step calls, each held to rule B on the features of the device's OWN window before that step, the
               edge count to the oracle's; the last step again at "f32" from the same window, at the parity bar
  3 compound   an 8-step rollout: d = the largest deviation of a sand row's end position from the float64 rollout's over the largest
               displacement of a sand row; d(device) <= COMPOUND_C d(restatement's own rollout), and finite.  Nothing from below.
  4 ranking    six candidates rolled out as one batch in "f16" and "f32": on every pair that the restatement's own noise leaves
               decided, the float64 Sinkhorn loss of the device's end positions orders the two as the float64 rollouts do, and so
               does SamplesLoss on the device
  5 raw rows   GraphIndependent in the mode at hidden 128 and 100 against the restatement that rounds every raw feature row at the
               kernels' scale, check A's bar (rel_rms <= 3 g, g recomputed per case); the sorted route on the same cases in rule B's
               envelope of that restatement

Every test prints err(device), err(restatement) and their ratio (1, 2, 5), d(device) / d(restatement) (3) and the per-pair table
(4).

Measured on an MI355X (no bar was tightened to these figures):
  1  err(device) / err(restatement) 0.81 .. 1.17 over the six graphs and both kernels (err(restatement) 9.3e-4 .. 1.7e-3)
  2  0.84 .. 1.44 over the 48 steps (two scenes, six models, four steps each); the edge counts equal the oracle's at every step
  3  d(device) / d(restatement) 0.88 .. 1.06 over the eight cases (n300: 1.04 hm, 0.88 sys, 1.00 sys_all, 0.88 default; n700: 1.06,
     1.06, 0.97, 1.06), d(restatement) 1.45e-4 / 1.38e-4.  COMPOUND_C = max(4, 2 x 1.06) = 4: the one-forward factor decides
  4  15 of 15 pairs decided by the references (the CPU test asks for 12 and the best against all); all 120 comparisons agree ("f16"
     and "f32", both kernels, float64 loss and SamplesLoss).  Losses 7.99e-6 .. 8.00e-6, gaps 2.5e-10 .. 1.2e-8, nu 1.7e-11 .. 5.7e-11;
     the closest pair (0, 1): gap 2.49e-10 in float64, 2.86e-10 from the f16 device rollout, 2.67e-10 through SamplesLoss
  5  encoder block against the restatement at the kernels' scale 1.0e-7 .. 8.9e-6 (3 g: 2.2e-6 .. 8.1e-5; closest 0.88 of its bar,
     hidden 100, features times 1e3, encoder_h); against the restatement that rounds rows and weights as they stand the device is
     2.9e-4 .. 3.2e-4 away with the features times 1e-4 (rows below 2^-14) and 9.8e-5 .. 2.1e-4 away with them times 1e3 (first-Linear
     weights below 2^-14), 13 and up to 24 times the bar: the kernels round at their scales, and the header's "scales commute with
     the rounding" was what was wrong (corrected there and in precision_cases.py).  Sorted route: 0.83 .. 1.05 of the restatement
"""
import ctypes as C

import numpy as np
import pytest
import torch

import f16_rollout_cases as fc
import layernorm_cases as lc
import precision_cases as pc
import yardstick
from conftest import assert_forward_close
from gpu_support import dev, graph_attr, load_model, to_dev as _t

pytestmark = pytest.mark.gpu

# d(device) <= COMPOUND_C d(restatement): twice the worst ratio measured over the eight cases (1.06: docstring), and not below the
# factor 4 of the one-forward envelope -- which is what decides
COMPOUND_C = 4.0


def _sorted_forward(m, nodes, ea, ei, dev):
    """gm_epd_forward with edge_attr_is_csr_order = 1 on edges that are in destination order already."""
    from gnn_manip_amd._lib import ModelDesc, check, current_stream, lib, ptr
    from gnn_manip_amd.epd_gnn import DstCsr
    from gnn_manip_amd.graph import _ws
    L = lib()
    n, e = nodes.shape[0], ea.shape[0]
    csr = DstCsr(ei, n)
    d = ModelDesc(*m.model_desc())
    fws = _ws(L.gm_forward_workspace_bytes(C.byref(d), n, e), dev)
    out = torch.empty((n, 3), dtype=torch.float32, device=dev)
    check(L.gm_epd_forward(m.device_handle(dev), ptr(nodes), n, ptr(ea), 1, ptr(csr.ws), e, ptr(out), ptr(fws), fws.numel(), current_stream(dev)))
    assert csr.validate() == e
    return out


def _in_envelope(fails, what, out, ref, err_r):
    """Rule B; prints err(device), err(restatement) and their ratio, appends to `fails` what lies outside."""
    finite = bool(np.isfinite(out).all())
    err_g = pc.max_err(out, ref, pc.B_FLOOR) if finite else float("inf")
    print(f"[f16 rollout] {what}: err(device) {err_g:.2e}, err(restatement) {err_r:.2e}, ratio {err_g / err_r:.2f}")
    if not (finite and err_r / 4 <= err_g <= 4 * err_r):
        fails.append((what, err_g, err_r))
    return err_g


# ================================================================== 1: sorted attributes
@pytest.mark.parametrize("name", fc.SORTED_GRAPHS)
@pytest.mark.parametrize("kernel", fc.SORTED_KERNELS)
def test_1_forward_on_sorted_attributes_in_the_envelope(dev, kernel, name):
    p, dims, nodes, ea, ei = fc.sorted_graph(name)
    ref, err_r = fc.sorted_reference(name)
    m = load_model(p, dims, dev, kernel, "f16")
    tn, te, ti = _t(nodes, dev), _t(ea, dev), _t(ei, dev)
    out16 = _sorted_forward(m, tn, te, ti, dev)
    fails = []
    print()
    _in_envelope(fails, f"sorted attributes {kernel} {name}", out16.cpu().numpy(), ref, err_r)
    assert not fails, fails
    if name == "scene":   # another encoder ran: the module hands edge_attr over in the caller's order
        with torch.no_grad():
            assert not yardstick.same_bits(m.forward(tn, te, ti), out16)
    m.set_precision("f32")
    out32 = _sorted_forward(m, tn, te, ti, dev).cpu().numpy()
    assert_forward_close(out32, ref, floor=pc.B_FLOOR, what=f"sorted attributes {kernel} {name}, back to f32")


# ================================================================== 2: every step, teacher-forced
@pytest.mark.parametrize("model", list(fc.STEP_MODELS))
@pytest.mark.parametrize("scene_name", list(fc.SCENES))
def test_2_every_step_of_a_rollout_in_the_envelope(dev, scene_name, model):
    from gnn_manip_amd import RolloutEngine
    hidden, kernel = fc.STEP_MODELS[model]
    p = fc.params(hidden)
    obs, traj = fc.rollout_scene(scene_name)
    n = obs.shape[1]
    m = load_model(p, fc.dims(hidden), dev, kernel, "f16")
    eng = RolloutEngine(m, graph_attr(fc.R), n, device=dev)
    a = _t(obs, dev)
    assert eng.set_scene(a) == traj.shape[1] > 0
    pred = torch.empty((n, 3), dtype=torch.float32, device=dev)
    fails = []
    print()
    for s in range(fc.STEPS):
        before = a.clone()
        eng.step(a, _t(traj[s], dev), pred_out=pred)
        edges = eng.status()
        ref, err_r, ref_edges, _ = fc.step_reference(p, before.cpu().numpy(), traj[s])
        assert edges == ref_edges, (s, edges, ref_edges)
        _in_envelope(fails, f"{scene_name} {model} step {s} ({edges} edges)", pred.cpu().numpy(), ref, err_r)
    assert not fails, fails
    m.set_precision("f32")
    again = before.clone()
    eng.step(again, _t(traj[fc.STEPS - 1], dev), pred_out=pred)
    assert eng.status() == ref_edges
    assert_forward_close(pred.cpu().numpy(), ref, floor=pc.B_FLOOR, what=f"{scene_name} {model} last step, back to f32")


# ================================================================== 3: compounding
@pytest.mark.parametrize("model", fc.COMPOUND_MODELS)
@pytest.mark.parametrize("scene_name", list(fc.SCENES))
def test_3_a_rollout_compounds_no_worse_than_its_restatement(dev, scene_name, model):
    from gnn_manip_amd import RolloutEngine
    hidden, kernel = fc.STEP_MODELS[model]
    obs, traj = fc.rollout_scene(scene_name)
    (end64, _), (end_r, _) = fc.compound_reference(scene_name, hidden)
    m = load_model(fc.params(hidden), fc.dims(hidden), dev, kernel, "f16")
    eng = RolloutEngine(m, graph_attr(fc.R), obs.shape[1], device=dev)
    end = eng.rollout(_t(obs, dev), _t(traj, dev), horizon=fc.HORIZON).cpu().numpy()
    d_dev, d_r = fc.end_deviation(end, end64, obs), fc.end_deviation(end_r, end64, obs)
    print(f"\n[f16 rollout] compound {scene_name} {model}: d(device) {d_dev:.3e}, d(restatement) {d_r:.3e}, ratio {d_dev / d_r:.2f} (bar {COMPOUND_C:g})")
    assert np.isfinite(end).all() and np.isfinite(d_dev)
    assert d_dev <= COMPOUND_C * d_r, (scene_name, model, d_dev, d_r)


# ================================================================== 4: the ranking
@pytest.mark.parametrize("kernel", fc.RANK_KERNELS)
def test_4_decided_pairs_are_ordered_as_in_float64(dev, kernel):
    from gnn_manip_amd import RolloutEngine
    from gnn_manip_amd.losses import SamplesLoss
    obs, trajs, desired = fc.rank_case()
    l64, nu, decided = fc.rank_reference()
    n = obs.shape[1]
    sand = _t(np.nonzero(fc.sand_rows(obs))[0], dev)
    loss = SamplesLoss(loss="sinkhorn", p=2, blur=fc.RANK_BLUR)
    print(f"\n[ranking] {kernel}: L64 {l64}, nu {nu}, {len(decided)} of 15 pairs decided")
    wrong = {}
    for precision in ("f16", "f32"):
        m = load_model(fc.params(128), fc.dims(128), dev, kernel, precision)
        eng = RolloutEngine(m, graph_attr(fc.R), n, device=dev, candidates=fc.RANK_B)
        out = eng.rollout_candidates(_t(obs, dev), _t(trajs, dev), horizon=fc.RANK_H)
        assert torch.isfinite(out).all()
        ends = out.cpu().numpy()
        host = np.array([fc.rank_loss(ends[c]) for c in range(fc.RANK_B)])
        clouds = out[:, -1].index_select(1, sand)[:, :, fc.CART[0]:fc.CART[0] + 3].contiguous()
        on_device = loss.batched(clouds, _t(desired, dev)).cpu().numpy().astype(np.float64)
        for what, losses in ((f"{kernel} {precision} rollout, float64 loss", host), (f"{kernel} {precision} rollout, SamplesLoss", on_device)):
            lines, bad = fc.rank_table(what, losses)
            print("\n".join(lines))
            assert np.isfinite(losses).all(), what
            if bad:
                wrong[what] = bad
    assert not wrong, wrong


# ================================================================== 5: raw rows at the kernels' scale
@pytest.mark.parametrize("name", fc.RAW_CASES)
@pytest.mark.parametrize("hidden", fc.RAW_HIDDEN)
def test_5_encoder_block_against_the_row_scale_restatement(dev, hidden, name):
    p, nodes, ea, _ = fc.raw_case(hidden, name)
    r64, g = fc.raw_reference(hidden, name)
    natural = fc.raw_restate(hidden, name, natural=True)
    m = load_model(p, lc.dims(hidden, fc.NL), dev, None, "f16")
    with torch.no_grad():
        h, e, _ = m.encoder(_t(nodes, dev), _t(ea, dev))
    got = {"encoder_h": h.cpu().numpy(), "encoder_e": e.cpu().numpy()}
    fails = []
    print()
    for out in fc.RAW_OUTPUTS:
        assert np.isfinite(got[out]).all(), out
        d = pc.rel_rms(got[out], r64[out])
        print(f"[f16 rollout] raw rows hidden {hidden} {name} {out}: against the row-scale restatement {d:.2e} (bar 3 g = {3 * g[out]:.2e}), "
              f"against the rows rounded as they stand {pc.rel_rms(got[out], natural[out]):.2e}")
        if not d <= 3 * g[out]:
            fails.append((out, d, 3 * g[out]))
    assert not fails, fails


@pytest.mark.parametrize("name", fc.RAW_CASES)
@pytest.mark.parametrize("kernel", fc.SORTED_KERNELS)
def test_5_sorted_route_in_the_envelope_of_the_row_scale_restatement(dev, kernel, name):
    p, nodes, ea, ei = fc.sorted_case(128, name)
    ref, err_r, err_natural = fc.raw_forward_reference(name)
    m = load_model(p, lc.dims(128, fc.NL), dev, kernel, "f16")
    out = _sorted_forward(m, _t(nodes, dev), _t(ea, dev), _t(ei, dev), dev).cpu().numpy()
    fails = []
    print()
    _in_envelope(fails, f"raw rows, sorted route {kernel} {name} (rows rounded as they stand: err {err_natural:.2e})", out, ref, err_r)
    assert not fails, fails
