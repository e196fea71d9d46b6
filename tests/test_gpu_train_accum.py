"""Mini-batches and gradient clipping in the library, on the MI355X (csrc/train_step.hip: gm_trainer_begin,
gm_train_step_accumulate, gm_train_rollout_accumulate, gm_trainer_apply, gm_trainer_accum_record, gm_grad_sumsq;
gnn_manip_amd/train.py: Trainer.zero_grad / accumulate / accumulate_rollout / apply, max_grad_norm, fit_epoch(accumulate=),
fit_rollout_epoch(batch_size=)).

Bounds.  gm_grad_sumsq: 1e-12 relative against math.fsum of the float64 squares -- derived, not measured: the terms are
non-negative, so the error is at most (elements per thread + the depths of the two trees) x 2^-53, below 3e-14 at every count here.
Weights, moments, records, scales and losses of an update: bit equality, with the existing single-sample entry points and with the
numpy restatements of tests/train_accum_cases.py.  The accumulated gradients against the float64 oracle's summed gradients: the rule
of tests/yardstick.py with the ReLU flip allowance.  The norm in the record against the float64 norm of the exported gradients:
1e-12.  Bit equality of the accumulated buffer with a float32 sum of separately computed gradients is not asserted: the backward may
add more than one partial per element.

The skip by an Inf in the gradient SUM behind finite losses is not tested: the L1 loss's gradient is +-1/count per output, so a
finite loss gives a bounded gradient at these weights; no honest input produces it."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
import grad_cases as gc
import train_accum_cases as ac
import train_rollout_cases as trc
import train_step_cases as sc
from gpu_support import dev, load_model, step_engine, to_dev
from grad_cases import L0
from yardstick import compare, same_bits

pytestmark = pytest.mark.gpu

LR = ac.LR
NAN = float("nan")
T = 3                                             # rollout steps of the rollout cases: the first three recorded frames


# ------------------------------------------------------------------------------------------ helpers
def _with_clip(t, max_grad_norm):
    t.max_grad_norm = max_grad_norm                # a plain attribute, like lr
    return t


def _trainer(dev, max_grad_norm=None):
    from gnn_manip_amd import Trainer
    m = load_model(ac.params(), ac.DIMS, dev)
    return _with_clip(Trainer(m, lr=LR), max_grad_norm), m


def _batch(i, dev):
    return tuple(to_dev(a, dev) for a in ac.sample(i))


def _state(t):
    from gnn_manip_amd import train
    return [t.export(w) for w in (train.PARAMS, train.EXP_AVG, train.EXP_AVG_SQ)]


def _same_state(a, b, what):
    for kind, ta, tb in zip(("weights", "exp_avg", "exp_avg_sq"), a, b):
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert same_bits(u, v), (what, kind, i)


def _slots(n, dev):
    return torch.full((n,), 7.0, dtype=torch.float64, device=dev)


def _bits64(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, np.float64)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _mini_batch(t, batches, dev, sample_losses=None):
    """zero_grad and one accumulate per batch; sample_losses: a float64 device tensor that receives the samples' losses."""
    t.zero_grad()
    for i, b in enumerate(batches):
        t.accumulate(*b, loss_out=None if sample_losses is None else sample_losses[i:i + 1])


def _rollout_setup(dev, max_grad_norm=None):
    """(trainer, engine after set_scene, obs0, frames [T, N, D]) on grad_cases' step scene at hidden 64."""
    from gnn_manip_amd import Trainer
    dims = (25, 4, 3, 64, 2, 2)
    m = load_model(orc.init_params(*dims, 845 + 64), dims, dev)
    eng = step_engine(m, dev)
    obs_np = gc.step_state("step_a")
    obs, frames = to_dev(obs_np, dev), to_dev(trc.step_frames("step_a")[:T], dev)
    assert eng.set_scene(obs) == len(gc.rigid_rows(obs_np, L0)) > 0
    return _with_clip(Trainer(m, lr=LR), max_grad_norm), eng, obs, frames


# ------------------------------------------------------------------------------------------ 1. gm_grad_sumsq
def _sumsq(x, dev, fill=NAN):
    """gm_grad_sumsq through ctypes in a workspace filled with `fill`: the float64 result as a [1] numpy array."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    need = L.gm_grad_sumsq_workspace_bytes(x.numel())
    assert need == 8 * ac.SUMSQ_GRID_MAX
    ws = torch.full((need // 8,), fill, dtype=torch.float64, device=dev)
    out = torch.full((1,), -3.0, dtype=torch.float64, device=dev)
    check(L.gm_grad_sumsq(ptr(x), x.numel(), ptr(out), ptr(ws), need, current_stream(dev)))
    return out.cpu().numpy()


@pytest.mark.parametrize("count", ac.SUMSQ_COUNTS)
def test_grad_sumsq_is_the_float64_sum(dev, count):
    x_np = ac.sumsq_case(count)
    x = to_dev(x_np, dev)
    want = ac.sumsq_exact(x_np)
    a, b, c = _sumsq(x, dev), _sumsq(x, dev), _sumsq(x, dev, fill=1e300)
    print(f"\n[grad sumsq] count {count}: {a[0]!r} exact {want!r} rel err {abs(a[0] - want) / want:.2e}")
    assert _bits64(a) == _bits64(b) == _bits64(c), (count, a, b, c)              # a run repeats itself, whatever the workspace held
    assert abs(a[0] - want) <= ac.SUMSQ_RTOL * want, (count, a[0], want)


def test_grad_sumsq_squares_in_float64_and_passes_non_finite_values_on(dev):
    # powers of two: every partial sum is a power of two times the square, so the float64 result is exact
    for count in (1024, 2 * 4 * ac.SUMSQ_WG * ac.SUMSQ_GRID_MAX):
        for value in (1e-30, 1e30):
            x = torch.full((count,), value, dtype=torch.float32, device=dev)
            want = float(count) * float(np.float32(value)) ** 2
            assert 0.0 < want < float("inf") and not 1e-45 < want < 3e38      # a float32 square would be 0 or inf
            got = _sumsq(x, dev)
            assert got[0] == want, (count, value, got[0], want)
    count = 1029                                                          # 257 float4 groups and a tail of one
    base = ac.sumsq_case(count, seed=3)
    for where in (0, 515, 1027, 1028):                                    # ..., the last float4, the tail: the last element
        for bad in (NAN, float("inf"), -float("inf")):
            x_np = base.copy()
            x_np[where] = bad
            got = _sumsq(to_dev(x_np, dev), dev)
            assert not math.isfinite(got[0]), (where, bad, got)
    assert math.isfinite(_sumsq(to_dev(base, dev), dev)[0])


def test_grad_sumsq_refusals(dev):
    from gnn_manip_amd._lib import current_stream, lib, ptr
    L = lib()
    err = lambda: L.gm_last_error().decode()
    x = to_dev(ac.sumsq_case(1000), dev)
    need = L.gm_grad_sumsq_workspace_bytes(1000)
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev)
    out = torch.full((1,), -3.0, dtype=torch.float64, device=dev)
    s = current_stream(dev)
    assert L.gm_grad_sumsq(None, 1000, ptr(out), ptr(ws), need, s) == -1 and err() == "gm_grad_sumsq: null pointer"
    assert L.gm_grad_sumsq(ptr(x), 1000, None, ptr(ws), need, s) == -1 and err() == "gm_grad_sumsq: null pointer"
    assert L.gm_grad_sumsq(ptr(x), 1000, ptr(out), None, need, s) == -1 and err() == "gm_grad_sumsq: null pointer"
    assert L.gm_grad_sumsq(ptr(x), 0, ptr(out), ptr(ws), need, s) == -1 and err() == "gm_grad_sumsq: count=0 out of range"
    assert L.gm_grad_sumsq(ptr(x), 1000, ptr(out), ptr(ws), need - 1, s) == -4 and err() == "gm_grad_sumsq: workspace %d < %d" % (need - 1, need)
    assert float(out) == -3.0                                             # nothing above reached the device


# ------------------------------------------------------------------------------------------ 2. one sample, no clip
def test_one_sample_without_a_clip_is_gm_train_step(dev):
    t, _ = _trainer(dev)
    twin, _ = _trainer(dev)
    got, own, want = _slots(3, dev), _slots(3, dev), _slots(3, dev)
    for i in range(3):                                                    # the three sizes, one after the other
        b = _batch(i, dev)
        t.zero_grad()
        t.accumulate(*b, loss_out=own[i:i + 1])
        t.apply(loss_out=got[i:i + 1])
        twin.step(*b, loss_out=want[i:i + 1])
        _same_state(_state(t), _state(twin), ("update", i))
        assert t.accum_record()["scale"] == 1.0
    assert t.record() == twin.record() and t.record()["steps_applied"] == 3
    assert np.array_equal(_bits64(got), _bits64(want)) and np.array_equal(_bits64(own), _bits64(want)) and np.isfinite(want.cpu().numpy()).all()
    rec = t.accum_record()
    assert (rec["samples"], rec["bad"], rec["sumsq"]) == (1, 0, 0.0) and math.isnan(rec["grad_norm"]) and rec["loss_sum"] == float(want[2])
    t.status()


def test_one_rollout_sample_without_a_clip_is_gm_train_rollout_step(dev):
    t, eng, obs, frames = _rollout_setup(dev)
    twin, eng2, _, _ = _rollout_setup(dev)
    got, own, want = _slots(3, dev), _slots(3, dev), _slots(3, dev)
    for i in range(3):
        t.zero_grad()
        t.accumulate_rollout(eng, obs, frames, pos_scale=trc.ACC_STD, loss_out=own[i:i + 1])
        t.apply(loss_out=got[i:i + 1])
        twin.step_rollout(eng2, obs, frames, pos_scale=trc.ACC_STD, loss_out=want[i:i + 1])
        _same_state(_state(t), _state(twin), ("rollout update", i))
    assert t.record() == twin.record() and t.record()["steps_applied"] == 3
    assert np.array_equal(_bits64(got), _bits64(want)) and np.array_equal(_bits64(own), _bits64(want)) and np.isfinite(want.cpu().numpy()).all()
    assert tuple(t.kept_windows().shape) == (T + 1, L0.k, gc.STEP_N, L0.D)


# ------------------------------------------------------------------------------------------ 3. three samples of three sizes
def test_three_samples_accumulate_the_oracles_summed_gradient(dev):
    from gnn_manip_amd import train
    t, m = _trainer(dev)
    batches = [_batch(i, dev) for i in range(3)]
    own = _slots(3, dev)
    _mini_batch(t, batches, dev, own)
    first = t.export(train.GRADS)
    _mini_batch(t, batches, dev)
    second = t.export(train.GRADS)
    for i, (a, b) in enumerate(zip(first, second)):
        assert same_bits(a, b), ("a second run", i)
    names = [k for k, _ in m.named_parameters()]
    ref_losses, r64 = ac.oracle_gradients()
    _, r32 = ac.oracle_gradients("float32")
    got = {k: g.cpu().numpy() for k, g in zip(names, first)}
    worst, worst2 = compare(got, r64, r32, ac.oracle_flip_allowance, what="accumulated gradients")
    print(f"\n[train accum] three samples: worst tensor {worst[0]} err {worst[2]:.3e} tol {worst[3]:.3e}; with allowance {worst2}")
    losses = own.cpu().numpy()
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-5)
    slot = _slots(1, dev)
    t.apply(loss_out=slot)
    want = ((losses[0] + losses[1]) + losses[2]) / 3.0
    assert _bits64(slot)[0] == _bits64(np.float64(want).reshape(1))[0] and want == ac.mean_loss(losses), (float(slot), want)
    rec = t.accum_record()
    assert (rec["samples"], rec["bad"]) == (3, 0) and rec["loss_sum"] == (losses[0] + losses[1]) + losses[2]
    assert rec["scale"] == float(np.float32(1.0 / 3.0))
    assert t.record()["steps_applied"] == 1
    t.status()


# ------------------------------------------------------------------------------------------ 4. the clip
@pytest.mark.parametrize("regime", ["active", "inactive"])
def test_clip_is_the_restated_scale_and_update(dev, regime):
    from gnn_manip_amd import train
    max_norm = {"active": ac.CLIP_ACTIVE, "inactive": ac.CLIP_INACTIVE}[regime]
    t, m = _trainer(dev, max_grad_norm=max_norm)
    plain, _ = _trainer(dev)                                              # the same mini-batch without a clip
    batches = [_batch(i, dev) for i in range(3)]
    w0 = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    for tr in (t, plain):
        _mini_batch(tr, batches, dev)
    grads = [g.cpu().numpy() for g in t.export(train.GRADS)]
    for g, h in zip(grads, plain.export(train.GRADS)):
        assert same_bits(g, h)
    t.apply()
    plain.apply()
    rec = t.accum_record()
    norm = ac.norm_of(grads, 3)
    print(f"\n[train accum] clip {regime}: max_grad_norm {max_norm}, norm {rec['grad_norm']!r} host {norm!r}, scale {rec['scale']!r}")
    assert abs(rec["grad_norm"] - norm) <= 1e-12 * norm, (rec["grad_norm"], norm)
    assert float(t.last_grad_norm) == rec["grad_norm"] and math.isnan(plain.accum_record()["grad_norm"])
    scale = ac.scale_of(rec["grad_norm"], 3, max_norm)
    assert rec["scale"] == float(scale), (rec["scale"], float(scale))
    assert rec["sumsq"] > 0 and abs(math.sqrt(rec["sumsq"]) / 3.0 - rec["grad_norm"]) <= 1e-15 * norm
    state = sc.adam_state(w0)
    w1 = ac.scaled_adam_restated(w0, grads, state, LR, np.float32(rec["scale"]))
    _same_state(_state(t), (w1, state["m"], state["v"]), regime)
    assert t.record() == plain.record() == dict(steps_applied=1, steps_skipped=0, beta1_pow=0.9, beta2_pow=0.999)
    assert float(t.last_loss) == float(plain.last_loss)
    if regime == "inactive":
        assert norm * 1.5 <= max_norm and rec["scale"] == float(np.float32(1.0 / 3.0))
        _same_state(_state(t), _state(plain), "an inactive clip is no clip")
        return
    assert norm >= 1.5 * max_norm and rec["scale"] < float(np.float32(1.0 / 3.0)) / 1.5
    # The clipped update moves no weight by more than the unclipped one.  exp_avg = o1 * (scale * g): monotone in the scale, exactly.
    # The step u = step * (m / ((sqrt(v) / s2) + e)) is monotone in |g| in exact arithmetic and passes through 8 float32 roundings
    # (m, two of v, sqrt, / s2, + e, the division, step *), each at most 2^-24 relative, in either update; p - u is rounded
    # monotonically: |moved clipped| <= |moved unclipped| * (1 + 16 * 2^-24) + one float32 spacing of the weight.
    for i, ((wc, mc, _), (wu, mu, _), p0) in enumerate(zip(zip(*_state(t)), zip(*_state(plain)), w0)):
        assert bool((mc.abs() <= mu.abs()).all()), ("exp_avg", i)
        moved_c = np.abs(wc.cpu().numpy().astype(np.float64) - p0)
        moved_u = np.abs(wu.cpu().numpy().astype(np.float64) - p0)
        assert (moved_c <= moved_u * (1.0 + 16.0 * 2.0 ** -24) + np.spacing(np.abs(p0))).all(), ("weights", i, float((moved_c - moved_u).max()))


# ------------------------------------------------------------------------------------------ 5. skips and refusals
@pytest.mark.parametrize("how", ["nan_target", "edge_index"])
def test_a_bad_sample_skips_its_mini_batch_and_leaves_no_trace(dev, how):
    from gnn_manip_amd._lib import GMError
    t, _ = _trainer(dev, max_grad_norm=ac.CLIP_ACTIVE)
    twin, _ = _trainer(dev, max_grad_norm=ac.CLIP_ACTIVE)
    b = [_batch(i, dev) for i in range(3)]
    for tr in (t, twin):
        _mini_batch(tr, b[:2], dev)
        tr.apply()
    before, rec0 = _state(t), t.record()
    x, ea, ei, y = b[1]
    if how == "nan_target":
        bad_y = y.clone()
        bad_y[5, 1] = NAN
        bad = (x, ea, ei, bad_y)
    else:
        bad_ei = ei.clone()
        bad_ei[1, 17] = x.shape[0]                                        # one entry out of range
        bad = (x, ea, bad_ei, y)
    own = _slots(2, dev)
    _mini_batch(t, [b[0], bad], dev, own)                                 # the second sample is the bad one
    slot = _slots(1, dev)
    t.apply(loss_out=slot)
    assert math.isnan(float(slot)) and math.isfinite(float(own[0])) and math.isnan(float(own[1]))
    _same_state(_state(t), before, how)
    assert t.record() == dict(rec0, steps_skipped=rec0["steps_skipped"] + 1) and rec0["steps_applied"] == 1
    rec = t.accum_record()
    assert (rec["samples"], rec["bad"]) == (2, 1)
    if how == "edge_index":                                               # the flag still surfaces through the tape header
        with pytest.raises(GMError, match="edge_index"):
            t.status()
    for tr in (t, twin):                                                  # the next mini-batch is the twin's, who never saw the bad one
        _mini_batch(tr, [b[2], b[0]], dev)
        tr.apply()
    _same_state(_state(t), _state(twin), (how, "the next mini-batch"))
    assert float(t.last_loss) == float(twin.last_loss) and float(t.last_grad_norm) == float(twin.last_grad_norm)
    assert twin.record() == dict(t.record(), steps_skipped=0) and t.record()["steps_applied"] == 2
    t.status()
    twin.status()


def test_apply_refuses_an_empty_mini_batch_and_a_nan_clip(dev):
    from gnn_manip_amd._lib import GMError, current_stream, lib
    t, _ = _trainer(dev)
    before = _state(t)
    L = lib()
    err = lambda: L.gm_last_error().decode()
    s = current_stream(dev)
    assert L.gm_trainer_apply(t._h, LR, 0.0, None, None, s) == -1 and err() == "gm_trainer_apply: no mini-batch begun (gm_trainer_begin)"
    t.zero_grad()
    assert L.gm_trainer_apply(t._h, LR, 0.0, None, None, s) == -1 and err() == "gm_trainer_apply: no sample accumulated"
    with pytest.raises(GMError, match="no sample accumulated"):
        t.apply()
    t.accumulate(*_batch(2, dev))
    assert L.gm_trainer_apply(t._h, LR, NAN, None, None, s) == -1 and err() == "gm_trainer_apply: max_grad_norm is NaN"
    assert L.gm_trainer_apply(t._h, NAN, 0.0, None, None, s) == -1 and err() == "gm_trainer_apply: lr is NaN"
    t.max_grad_norm = NAN
    with pytest.raises(ValueError, match="max_grad_norm"):
        t.apply()
    t.max_grad_norm = None
    _same_state(_state(t), before, "refusals")
    assert t.record() == dict(steps_applied=0, steps_skipped=0, beta1_pow=1.0, beta2_pow=1.0)
    t.apply()                                                             # the refusals left the pending sample alone
    assert t.record()["steps_applied"] == 1
    with pytest.raises(GMError, match="no mini-batch begun"):             # one update per mini-batch
        t.apply()
    with pytest.raises(GMError, match="no mini-batch begun"):
        t.accumulate(*_batch(2, dev))
    t.status()


# ------------------------------------------------------------------------------------------ 6. Python
def test_a_trainer_with_a_clip_steps_through_the_three_calls(dev):
    b = [_batch(i, dev) for i in range(3)]
    t, _ = _trainer(dev, max_grad_norm=ac.CLIP_ACTIVE)
    twin, _ = _trainer(dev, max_grad_norm=ac.CLIP_ACTIVE)
    got, want = _slots(3, dev), _slots(3, dev)
    for i in range(3):
        t.step(*b[i], loss_out=got[i:i + 1])
        twin.zero_grad()
        twin.accumulate(*b[i])
        twin.apply(loss_out=want[i:i + 1])
    _same_state(_state(t), _state(twin), "step with a clip")
    assert np.array_equal(_bits64(got), _bits64(want)) and t.record() == twin.record() and t.record()["steps_applied"] == 3
    assert float(t.last_grad_norm) == float(twin.last_grad_norm) > ac.CLIP_ACTIVE
    # ... and the rollout's
    t, eng, obs, frames = _rollout_setup(dev, max_grad_norm=1e-3)
    twin, eng2, _, _ = _rollout_setup(dev, max_grad_norm=1e-3)
    got, want = _slots(2, dev), _slots(2, dev)
    for i in range(2):
        t.step_rollout(eng, obs, frames, pos_scale=trc.ACC_STD, loss_out=got[i:i + 1])
        twin.zero_grad()
        twin.accumulate_rollout(eng2, obs, frames, pos_scale=trc.ACC_STD)
        twin.apply(loss_out=want[i:i + 1])
    _same_state(_state(t), _state(twin), "step_rollout with a clip")
    assert np.array_equal(_bits64(got), _bits64(want)) and t.record() == twin.record() and t.record()["steps_applied"] == 2
    norm = float(t.last_grad_norm)
    print(f"\n[train accum] step_rollout with max_grad_norm 1e-3: norm {norm!r}, scale {t.accum_record()['scale']!r}")
    assert norm == float(twin.last_grad_norm) and math.isfinite(norm) and norm > 0


@pytest.fixture(scope="module")
def g9_root(golden, tmp_path_factory):
    """The synthetic recordings of tests/golden/g9_dataset.npz as a dataset directory."""
    g = golden("g9_dataset.npz")
    root = str(tmp_path_factory.mktemp("g9_train_accum")) + "/"
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")
    return root


def _two_sizes(g9_root, dev):
    """The two recordings as a resident dataset, the second without its first twelve rows: 60 and 48 nodes, ten rigid rows each."""
    from gnn_manip_amd import CoffeeDataset
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    sims = [ds.sims[0], ds.sims[1][:, 12:].contiguous()]
    assert [tuple(s.shape) for s in sims] == [(9, 60, 5), (9, 48, 5)] and all(int((s[0][:, 1] == 1).sum()) == 10 for s in sims)
    return CoffeeDataset.from_recordings(sims, 6, 0.015, ds.stats, ds.bounds, ds.cartesian_idx, ds.material_id, ds.control_idx, noise=3e-4,
                                         use_control=True)


def test_fit_rollout_epoch_in_mini_batches_of_two_sizes(dev, g9_root):
    from gnn_manip_amd import RolloutEngine, Trainer
    ds = _two_sizes(g9_root, dev)
    dims = (25, 4, 3, 64, 2, 2)
    params = orc.init_params(*dims, 309)
    scale = [float(v) for v in ds.stats["acceleration_std"]]
    starts = [0, 1, 2, 3, 4]                                              # three windows of 60 nodes, then two of 48
    assert [ds.index[i][0] for i in starts] == [0, 0, 0, 1, 1]

    def fresh(max_grad_norm):
        m = load_model(params, dims, dev)
        engines = {n: RolloutEngine(m, ds.graph_attr, n, k_steps=6, data_dim=8, device=dev) for n in (60, 48)}
        return _with_clip(Trainer(m, lr=LR, sand_only=True, material_col=sc.MATERIAL_COL), max_grad_norm), engines

    for max_norm in (None, 0.05):
        manual, engines = fresh(max_norm)
        losses, norms = _slots(3, dev), torch.full((3,), NAN, dtype=torch.float64, device=dev)
        groups = [[0, 1], [2, 3], [4]]
        scene = None
        for u, group in enumerate(groups):
            manual.zero_grad()
            for start in group:
                window, frames = ds.rollout_sample(start, 1, seed=5, stream=start)
                eng = engines[int(window.shape[1])]
                if scene != ds.index[start][0]:
                    eng.set_scene(window)
                    scene = ds.index[start][0]
                manual.accumulate_rollout(eng, window, frames, 1, pos_scale=scale)
            manual.apply(loss_out=losses[u:u + 1], norm_out=norms[u:u + 1] if max_norm else None)
        want, want_norms = losses.cpu().numpy(), norms.cpu().numpy()
        t, engines = fresh(max_norm)
        got = t.fit_rollout_epoch(ds, engines, 1, starts=starts, seed=5, pos_scale=scale, batch_size=2)
        print(f"\n[train accum] fit_rollout_epoch batch_size=2 max_grad_norm={max_norm}: {got} norms {t.last_epoch_grad_norms}")
        assert got.dtype == np.float64 and got.shape == (3,) and np.isfinite(got).all() and np.array_equal(_bits64(got), _bits64(want))
        assert t.last_epoch_grad_norms.shape == (3,) and np.array_equal(_bits64(t.last_epoch_grad_norms), _bits64(want_norms))
        assert np.isnan(want_norms).all() if max_norm is None else (want_norms > 0).all()
        _same_state(_state(t), _state(manual), ("fit_rollout_epoch", max_norm))
        assert t.record() == manual.record() and t.record()["steps_applied"] == 3


def test_epoch_defaults_are_the_single_sample_calls(dev, g9_root):
    from gnn_manip_amd import RolloutEngine, Trainer
    ds = _two_sizes(g9_root, dev)
    dims = (25, 4, 3, 64, 2, 2)
    params = orc.init_params(*dims, 309)

    def fresh():
        m = load_model(params, dims, dev)
        return Trainer(m, lr=LR), RolloutEngine(m, ds.graph_attr, 60, k_steps=6, data_dim=8, device=dev)

    starts = [0, 1, 2]
    twin, eng = fresh()
    want = _slots(3, dev)
    for i, start in enumerate(starts):
        window, frames = ds.rollout_sample(start, 1, seed=5, stream=start)
        if i == 0:
            eng.set_scene(window)
        twin.step_rollout(eng, window, frames, 1, loss_out=want[i:i + 1])
    t, eng = fresh()
    got = t.fit_rollout_epoch(ds, eng, 1, starts=starts, seed=5)
    assert got.shape == (3,) and np.array_equal(_bits64(got), _bits64(want)) and np.isfinite(got).all()
    assert t.last_epoch_grad_norms.shape == (3,) and np.isnan(t.last_epoch_grad_norms).all()
    _same_state(_state(t), _state(twin), "fit_rollout_epoch with its defaults")
    assert t.record() == twin.record() and t.record()["steps_applied"] == 3
    # shuffle: the same samples in the seed's order
    t, eng = fresh()
    order = [starts[i] for i in np.random.default_rng(5).permutation(3)]
    got = t.fit_rollout_epoch(ds, eng, 1, starts=starts, seed=5, shuffle=True)
    t2, eng2 = fresh()
    want2 = t2.fit_rollout_epoch(ds, eng2, 1, starts=order, seed=5)
    assert np.array_equal(_bits64(got), _bits64(want2))
    _same_state(_state(t), _state(t2), "shuffle")


def test_fit_epoch_accumulates_and_synchronises_once(dev, g9_root, monkeypatch):
    from gnn_manip_amd import CoffeeDataset, GraphLoader, Trainer
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    dims = (25, 4, 3, 64, 2, 2)
    params = orc.init_params(*dims, 307)
    loader = lambda: GraphLoader(ds, batch_size=2, seed=2, fused=True, prefetch=1)
    kw = dict(lr=LR, sand_only=True, material_col=sc.MATERIAL_COL)
    manual = _with_clip(Trainer(load_model(params, dims, dev), **kw), 0.5)
    batches = list(loader())
    assert len(batches) == 3
    losses, norms = _slots(2, dev), _slots(2, dev)
    for u, group in enumerate((batches[:2], batches[2:])):
        manual.zero_grad()
        for batch in group:
            manual.accumulate(batch)
        manual.apply(loss_out=losses[u:u + 1], norm_out=norms[u:u + 1])
    want, want_norms = losses.cpu().numpy(), norms.cpu().numpy()
    assert np.isfinite(want).all() and (want_norms > 0).all()
    t = _with_clip(Trainer(load_model(params, dims, dev), **kw), 0.5)
    epoch_loader = loader()
    calls = []

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(torch.cuda, "synchronize", spy("torch.cuda.synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("Stream.synchronize", torch.cuda.Stream.synchronize))
    got = t.fit_epoch(epoch_loader, accumulate=2)
    assert calls == ["Stream.synchronize"], calls
    monkeypatch.undo()
    assert got.dtype == np.float64 and np.array_equal(_bits64(got), _bits64(want)), (got, want)
    assert np.array_equal(_bits64(t.last_epoch_grad_norms), _bits64(want_norms))
    _same_state(_state(t), _state(manual), "fit_epoch(accumulate=2) against the manual loop")
    assert t.record() == manual.record() and t.record()["steps_applied"] == 2
    t.status()
