"""The fp16 single-product inference mode on the device (``set_precision("f16")``; contract: include/gnn_manip_hip.h, "Numeric domain
of the fp16 mode"; cases and the numpy restatement: precision_cases.py).

A  one MLP deep, tight: both outputs of ``GraphIndependent.forward`` and ``e_out`` of ``InteractionNetwork.forward`` against the
   float64-accumulating restatement, rms of the difference over the rms of the output, at most 3 g per case (g: the same measure
   between the float32- and the float64-accumulating restatement, recomputed here; test_precision_cases.py shows that 3 g is below
   half the distance to the exact forward and to the variants with one operand left unrounded).
B  whole forward, envelope: err(x) = max |x - ref| / max(max |ref|, 1e-3) against oracle/torch_epd.py in float64;
   err(restatement) / 4 <= err(f16 forward) <= 4 err(restatement) -- the device and the restatement are two draws of one rounding
   noise -- and the same model set back to "f32" meets the float32 parity bar on the same inputs.  Systolic kernels on the shapes
   of test_gpu_edge_ticks.py (with and without node fusion), streamed kernels at three widths / depths and past the node kernel's
   switch to its four-block form.
C  plumbing, bit for bit.   D  the numeric domain in the mode."""
import ctypes as C

import numpy as np
import pytest
import torch

import precision_cases as pc
from conftest import BOUNDS, CART, CTRL, MAT, STATS, assert_forward_close
from gpu_support import dev, graph_attr, load_model as _model, poison_allocator as _poison, to_dev as _t

pytestmark = pytest.mark.gpu

R, K = 0.015, 20


# ================================================================== A: one MLP deep, tight
@pytest.mark.parametrize("hidden,nl", pc.A_CASES)
def test_a_one_mlp_deep_against_the_restatement(dev, hidden, nl):
    r64, g = pc.a_reference(hidden, nl)
    nodes, ea, h, e, ei = (_t(a, dev) for a in pc.a_inputs(hidden, nl))
    m = _model(pc.a_params(hidden, nl), (pc.NODE_DIM, pc.EDGE_DIM, pc.OUT_DIM, hidden, nl, 1), dev)
    got = {}
    for precision in ("f16", "f32"):
        m.set_precision(precision)
        assert m.encoder.precision == m.processor[0].precision == precision
        with torch.no_grad():
            eh, ee, _ = m.encoder(nodes, ea)
            _, be, _ = m.processor[0](h, e, ei)
        got[precision] = {"encoder_h": eh.cpu().numpy(), "encoder_e": ee.cpu().numpy(), "block_e": be.cpu().numpy()}
    ex = pc.a_restate(hidden, nl, round_w=False, round_x=False)
    fails = []
    for name in pc.A_OUTPUTS:
        d16, d32 = pc.rel_rms(got["f16"][name], r64[name]), pc.rel_rms(got["f32"][name], ex[name])
        print(f"hidden {hidden} layers {nl} {name}: f16 against the restatement {d16:.2e} (bar 3 g = {3 * g[name]:.2e}), "
              f"f16 against exact {pc.rel_rms(got['f16'][name], ex[name]):.2e}, f32 against exact {d32:.2e}")
        assert np.isfinite(got["f16"][name]).all(), name
        if not d16 <= 3 * g[name]:
            fails.append((name, d16, 3 * g[name]))
        assert d32 < 1e-5, (name, d32)   # the switch back is the float32 path
    assert not fails, fails


# ================================================================== B: whole forward, envelope
def _envelope(m, reference, nodes, ea, ei, what):
    ref, err_r = reference
    dev = next(m.parameters()).device
    tn, te, ti = _t(nodes, dev), _t(ea, dev), _t(ei, dev)
    m.set_precision("f16")
    with torch.no_grad():
        out16 = m.forward(tn, te, ti).cpu().numpy()
    assert m.status() == ei.shape[1]
    m.set_precision("f32")
    with torch.no_grad():
        out32 = m.forward(tn, te, ti).cpu().numpy()
    assert m.status() == ei.shape[1]
    err_g = pc.max_err(out16, ref, pc.B_FLOOR)
    print(f"{what}: err(f16 forward) = {err_g:.2e}, err(restatement) = {err_r:.2e}, ratio {err_g / err_r:.2f}; "
          f"err(f32 forward) = {pc.max_err(out32, ref, pc.B_FLOOR):.2e}")
    assert np.isfinite(out16).all(), what
    assert err_r / 4 <= err_g <= 4 * err_r, (what, err_g, err_r)
    assert_forward_close(out32, ref, floor=pc.B_FLOOR, what=f"{what}, back to f32")


@pytest.fixture(scope="module")
def sys_model(dev):
    return _model(pc.sys_params(), pc.SYS_DIMS, dev, "sys_all")


@pytest.mark.parametrize("fusion", [True, False])
@pytest.mark.parametrize("name", [c[0] for c in pc.SYS_GRAPHS])
def test_b_systolic_forward_in_the_envelope(dev, sys_model, name, fusion):
    sys_model.set_node_fusion(fusion)
    try:
        _envelope(sys_model, pc.sys_reference(name), *pc.sys_case(name), f"sys_all {name} fusion {fusion}")
    finally:
        sys_model.set_node_fusion(True)


@pytest.mark.parametrize("name", [c[0] for c in pc.HM_CASES])
def test_b_streamed_forward_in_the_envelope(dev, name):
    _, hidden, nl, ms, _, _ = next(c for c in pc.HM_CASES if c[0] == name)
    m = _model(pc.hm_params(name), (pc.NODE_DIM, pc.EDGE_DIM, pc.OUT_DIM, hidden, nl, ms), dev, "hm")
    _envelope(m, pc.hm_reference(name), *pc.hm_case(name), f"hm {name}")


# ================================================================== C: plumbing and invariants, bit for bit
C_DIMS = (pc.NODE_DIM, pc.EDGE_DIM, pc.OUT_DIM, 128, 2, 3)


def _c_params():
    from oracle import epd_oracle as orc
    return orc.init_params(*C_DIMS, 4242)


def _scene(n=700, seed=95, steps=2, b=1):
    from gnn_manip_amd import scene
    obs = scene.make_scene(n, seed=seed, side=0.075)
    trajs = np.stack([scene.rigid_drift_trajectory(obs, steps, seed=100 + c, step_size=3e-4) for c in range(b)])
    return obs, trajs


def _everything(m, dev):
    """forward, both stand-alone blocks and a 2-step rollout of `m` as it is set."""
    from gnn_manip_amd import RolloutEngine
    nodes, ea, ei = (_t(a, dev) for a in pc.sys_case("hub"))
    _, _, h, e, ei_a = (_t(a, dev) for a in pc.a_inputs(128, 2))
    obs, trajs = _scene()
    with torch.no_grad():
        out = {"forward": m.forward(nodes, ea, ei).clone()}
        m.status()
        out["encoder_h"], out["encoder_e"], _ = m.encoder(nodes, ea)
        out["block_h"], out["block_e"], _ = m.processor[0](h, e, ei_a)
        eng = RolloutEngine(m, graph_attr(R), obs.shape[1], device=dev)
        out["rollout"] = eng.rollout(_t(obs, dev), _t(trajs[0], dev), horizon=2).clone()
        eng.status()
    return out


@pytest.mark.parametrize("kernel", ["auto", "sys_all", "hm"])
def test_c_switching_back_gives_the_bits_of_a_model_never_switched_and_f16_repeats(dev, kernel):
    never = _everything(_model(_c_params(), C_DIMS, dev, kernel), dev)
    m = _model(_c_params(), C_DIMS, dev, kernel)
    m.set_precision("f16")
    assert m.precision == "f16"
    first = _everything(m, dev)
    _poison(dev, float("nan"))
    second = _everything(m, dev)
    _poison(dev, float("inf"))
    third = _everything(m, dev)
    m.set_precision("f32")
    assert m.precision == "f32"
    back = _everything(m, dev)
    for k in never:
        assert torch.isfinite(first[k]).all(), k
        assert torch.equal(never[k], back[k]), (k, "f16 then f32 against never switched", float((never[k] - back[k]).abs().max()))
        assert torch.equal(first[k], second[k]), (k, "f16 twice / NaN-poisoned workspaces", float((first[k] - second[k]).abs().max()))
        assert torch.equal(first[k], third[k]), (k, "inf-poisoned workspaces", float((first[k] - third[k]).abs().max()))
        assert not torch.equal(first[k], never[k]), (k, "the switch changed nothing")


@pytest.mark.parametrize("kernel", ["sys_all", "hm"])
def test_c_candidate_of_a_batch_equals_the_scene_alone(dev, kernel):
    from gnn_manip_amd import RolloutEngine
    n, steps, b = 700, 2, 3
    obs, trajs = _scene(n, 95, steps, b)
    m = _model(_c_params(), C_DIMS, dev, kernel, "f16")
    with torch.no_grad():
        out = RolloutEngine(m, graph_attr(R), n, device=dev, candidates=b).rollout_candidates(_t(obs, dev), _t(trajs, dev))
        one = RolloutEngine(m, graph_attr(R), n, device=dev).rollout(_t(obs, dev), _t(trajs[1], dev), horizon=steps)
    assert torch.isfinite(one).all()
    assert torch.equal(out[1], one), float((out[1] - one).abs().max())


@pytest.mark.parametrize("kernel", ["hm", "sys_all"])
def test_c_a_step_is_the_forward_on_its_own_features(dev, kernel):
    """gm_rollout_step in the mode against state_pre -> node features -> radius graph -> csr -> edge features (sorted order) ->
    gm_epd_forward through the stand-alone entry points on the same handle: the same prediction, bit for bit, and not the float32
    one."""
    from gnn_manip_amd import RolloutEngine
    from gnn_manip_amd._lib import ModelDesc, check, current_stream, lib
    from gnn_manip_amd.graph import make_feature_desc
    obs, trajs = _scene(700, 96, 1)
    n, D, k = obs.shape[1], obs.shape[2], obs.shape[0]
    cap = n * K
    m = _model(_c_params(), C_DIMS, dev, kernel, "f16")
    eng = RolloutEngine(m, graph_attr(R), n, device=dev)
    a, target = _t(obs, dev), _t(trajs[0][0], dev)
    assert eng.set_scene(a) == target.shape[0] > 0
    pred_step = torch.empty((n, 3), dtype=torch.float32, device=dev)
    eng.step(a, target, pred_out=pred_step)
    edges = eng.status()
    L, stream = lib(), (lambda: current_stream(dev))
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)
    u8 = lambda nb: torch.empty(max(int(nb), 256), dtype=torch.uint8, device=dev)
    fd = make_feature_desc(R, STATS, BOUNDS, CART, MAT, CTRL, k, D)
    md = ModelDesc(*m.model_desc())
    b = _t(obs, dev)
    check(L.gm_state_pre(p(b), n, C.byref(fd), p(eng.rigid_rank), p(target), stream()))
    x = torch.empty((n, C_DIMS[0]), dtype=torch.float32, device=dev)
    check(L.gm_node_features(p(b), n, C.byref(fd), p(x), stream()))
    last = (k - 1) * n * D + CART[0]
    gws, cws = u8(L.gm_graph_workspace_bytes(n, K)), u8(L.gm_csr_workspace_bytes(n, cap))
    check(L.gm_radius_graph_build(p(b, last), D, n, R, K, p(gws), gws.numel(), stream()))
    check(L.gm_csr_from_graph(p(gws), n, K, p(cws), cws.numel(), stream()))
    ea = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
    check(L.gm_edge_features_csr(p(b, last), D, p(cws), n, cap, R, p(ea), stream()))
    fws = u8(L.gm_forward_workspace_bytes(C.byref(md), n, cap))
    preds = {}
    for precision in ("f16", "f32"):
        m.set_precision(precision)
        preds[precision] = torch.empty((n, 3), dtype=torch.float32, device=dev)
        check(L.gm_epd_forward(m.device_handle(dev), p(x), n, p(ea), 1, p(cws), cap, p(preds[precision]), p(fws), fws.numel(), stream()))
    e_b = C.c_int64(-1)
    check(L.gm_csr_num_edges(p(cws), C.byref(e_b), stream()))
    assert e_b.value == edges > 0
    assert torch.isfinite(pred_step).all() and float(pred_step.abs().max()) > 0
    assert torch.equal(pred_step, preds["f16"]), float((pred_step - preds["f16"]).abs().max())
    assert not torch.equal(pred_step, preds["f32"])


def test_c_the_setting_survives_a_weight_update(dev):
    from oracle import epd_oracle as orc
    nodes, ea, ei = (_t(a, dev) for a in pc.sys_case("hub"))
    other = orc.init_params(*C_DIMS, 4243)
    m = _model(_c_params(), C_DIMS, dev, "auto", "f16")
    with torch.no_grad():
        before = m.forward(nodes, ea, ei).clone()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()}, strict=True)
        after = m.forward(nodes, ea, ei).clone()
        fresh16 = _model(other, C_DIMS, dev, "auto", "f16").forward(nodes, ea, ei)
        fresh32 = _model(other, C_DIMS, dev, "auto").forward(nodes, ea, ei)
    assert m.precision == "f16"
    assert torch.equal(after, fresh16), float((after - fresh16).abs().max())
    assert not torch.equal(after, fresh32) and not torch.equal(after, before)


def test_c_autograd_paths_do_not_read_the_switch(dev):
    """``forward`` under autograd is the training forward, and the backward of a differentiable rollout differentiates the float32
    step at the windows it is given: the same bits whatever the switch says.  (One step and a linear loss, so that neither the
    windows nor the gradient that enters the sweep depend on the mode of the inference forward; ``step_backward`` takes its window
    as an argument.)"""
    from gnn_manip_amd import RolloutEngine
    nodes, ea, ei = (_t(a, dev) for a in pc.sys_case("hub"))
    obs, trajs = _scene(700, 97, 1)
    w = torch.randn(obs.shape, generator=torch.Generator().manual_seed(5)).to(dev)
    got = {}
    for precision in ("f32", "f16"):
        m = _model(_c_params(), C_DIMS, dev, "auto", precision)
        x = nodes.clone().requires_grad_(True)
        out = m.forward(x, ea, ei)
        out.square().sum().backward()
        r = {"train_forward": out.detach().clone(), "d_nodes": x.grad.clone(),
             "d_weight": m.decoder[0].weight.grad.clone()}
        eng = RolloutEngine(m, graph_attr(R), obs.shape[1], device=dev)
        o0 = _t(obs, dev).requires_grad_(True)
        tr = _t(trajs[0], dev).requires_grad_(True)
        for sweep in ("autograd", "library"):
            o0.grad = tr.grad = None
            final = eng.differentiable_rollout(o0, tr, horizon=1, sweep=sweep)
            (final * w).sum().backward()
            r[f"{sweep}_d_obs0"], r[f"{sweep}_d_traj"] = o0.grad.clone(), tr.grad.clone()
        eng.set_scene(_t(obs, dev))
        r["vjp_d_obs"], r["vjp_d_target"] = eng.step_backward(_t(obs, dev), _t(trajs[0][0], dev), w.contiguous())
        got[precision] = r
    for k in got["f32"]:
        assert torch.isfinite(got["f32"][k]).all() and float(got["f32"][k].abs().max()) > 0, k
        assert torch.equal(got["f32"][k], got["f16"][k]), (k, float((got["f32"][k] - got["f16"][k]).abs().max()))


# ================================================================== D: domain
@pytest.mark.parametrize("kernel", ["sys", "hm"])
def test_d_unrepresentable_latents_are_reported_not_clamped_in_the_mode(dev, kernel):
    """The recipe of test_gpu_domain.py: a LayerNorm gain of 1e6 in the node encoder puts |h| beyond fp16.  In the mode such a
    value is a lone +-inf in the operand image (not an (inf, -inf) pair), its row's accumulators are +-inf or NaN, and the row
    check must take both: status() raises, the prediction is not finite anywhere."""
    from gnn_manip_amd import scene
    from gnn_manip_amd._lib import GMError
    from oracle import epd_oracle as orc
    obs = scene.make_scene(600, seed=31, side=0.07)
    nodes, ea, s, r, _ = orc.process(obs, None, control_idx=CTRL, stats=STATS, bounds=BOUNDS, conn_r=R, cartesian_idx=CART, material_idx=MAT)
    ei = np.stack((s, r))
    dims = (25, 4, 3, 128, 2, 2)
    p = orc.init_params(*dims, 600)
    p["encoder.phi_node.5.weight"] = (p["encoder.phi_node.5.weight"] * np.float32(1e6)).astype(np.float32)
    m = _model(p, dims, dev, kernel, "f16")
    with torch.no_grad():
        out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev))
    with pytest.raises(GMError, match="fp16 split range"):
        m.status()
    assert not torch.isfinite(out).any()
    m2 = _model(orc.init_params(*dims, 600), dims, dev, kernel, "f16")
    with torch.no_grad():
        out2 = m2.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev))
    assert m2.status() == ei.shape[1] and torch.isfinite(out2).all()


@pytest.mark.parametrize("hid", [128, 64, 100])
def test_d_standalone_encoder_turns_a_non_finite_input_row_into_a_nan_row_in_the_mode(dev, hid):
    from gnn_manip_amd import EncProcDecGNN
    torch.manual_seed(hid)
    m = EncProcDecGNN(25, 4, 3, hid, 2, 2).to(dev)
    m.set_precision("f16")
    n, e = 300, 2000
    x, ea = torch.randn(n, 25, device=dev), torch.randn(e, 4, device=dev)
    with torch.no_grad():
        h32 = _f32_encoder(m, x, ea)
        h0, e0, _ = m.encoder(x, ea)
        xb, eb = x.clone(), ea.clone()
        xb[7, 3] = float("nan"); xb[100, 24] = float("inf"); xb[299, 0] = float("-inf"); xb[20, 0] = 1e30
        eb[11, 1] = float("inf"); eb[1999, 3] = float("nan"); eb[64, 0] = -1e30
        h1, e1, _ = m.encoder(xb, eb)
    assert not torch.equal(h0, h32)   # the mode is on
    bad_n, bad_e = [7, 100, 299], [11, 1999]
    assert torch.isnan(h1[bad_n]).all() and torch.isnan(e1[bad_e]).all()
    keep_n = torch.ones(n, dtype=torch.bool, device=dev); keep_n[bad_n + [20]] = False
    keep_e = torch.ones(e, dtype=torch.bool, device=dev); keep_e[bad_e + [64]] = False
    assert torch.equal(h1[keep_n], h0[keep_n]) and torch.equal(e1[keep_e], e0[keep_e])
    assert torch.isfinite(h1[20]).all() and torch.isfinite(e1[64]).all()


def _f32_encoder(m, x, ea):
    m.set_precision("f32")
    h, _, _ = m.encoder(x, ea)
    m.set_precision("f16")
    return h.clone()
