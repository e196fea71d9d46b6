"""GPU: rollouts of scenes of different sizes as one ragged batch (gm_rollout_step_ragged, gm_rollout_ragged,
gm_rollout_recorded_ragged, gm_rollout_errors_ragged, RolloutEngine(sizes=...), evaluate_rollout(ragged=True)) against the same
scenes rolled ALONE through the single-scene entry points.  Every comparison is bit for bit (yardstick.same_bits / torch.equal):
the cases of tests/ragged_rollout_cases.py put the scenes' boundaries where a shared block plan, a shared neighbour workgroup or
a shared scatter-add group would show.  All graphs of every case lie below the node path's size threshold (the one condition of
the batch invariance, include/gnn_manip_hip.h)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from gpu_support import dev, feature_desc, graph_attr, load_model, poison_allocator, rollout_engine, to_dev
from yardstick import same_bits
import ragged_rollout_cases as rrc

pytestmark = pytest.mark.gpu
L = rrc.L


def _lib():
    from gnn_manip_amd import _lib
    return _lib


@functools.lru_cache(maxsize=None)
def _model(name, dev):
    dims, params, kernel, precision = rrc.model(name)
    return load_model(params, dims, dev, kernel=kernel, precision=precision)


def _single_engine(m, n, dev, max_nb, **kw):
    return rollout_engine(m, rrc.R, L, n, dev, max_neighbours=max_nb, renumber=False, **kw)


def _ragged_engine(m, sizes, dev, max_nb):
    from gnn_manip_amd import RolloutEngine
    return RolloutEngine(m, graph_attr(rrc.R, L), k_steps=L.k, data_dim=L.D, device=dev, max_neighbours=max_nb, sizes=list(sizes))


@functools.lru_cache(maxsize=None)
def _scripted_alone(case_name, model_name, dev):
    """Per scene (final state, records, edge count of the last step) of gm_rollout on the scene alone: computed once, shared."""
    c, m = rrc.case(case_name), _model(model_name, dev)
    out = []
    with torch.no_grad():
        for s, traj in zip(c.scenes, c.trajectories()):
            eng = _single_engine(m, s.n, dev, c.max_nb)
            final, recs = eng.rollout(to_dev(s.window(), dev), to_dev(traj, dev), horizon=rrc.STEPS, record=True)
            out.append((final, recs, eng.status()))
    return out


@functools.lru_cache(maxsize=None)
def _recorded_alone(case_name, model_name, dev):
    """Per scene (final state, records, predictions) of gm_rollout_recorded on the scene alone."""
    c, m = rrc.case(case_name), _model(model_name, dev)
    out = []
    with torch.no_grad():
        for s in c.scenes:
            eng = _single_engine(m, s.n, dev, c.max_nb)
            obs = to_dev(s.window(), dev)
            eng.set_scene(obs)
            recs, preds = eng.run_recorded(obs, to_dev(s.frames(), dev), rrc.STEPS, record=True, record_pred=True)
            eng.status()
            out.append((obs, recs, preds))
    return out


def _scripted_batch(eng, c, dev):
    final, recs = eng.rollout(to_dev(c.window(), dev), to_dev(c.trajectory(), dev), horizon=rrc.STEPS, record=True)
    return final, recs, eng.status()


def _assert_rows_are_the_scenes(c, batch, alone, what):
    """batch: tensors [.., N, ..] with the node axis second; alone[g]: the same tensors of scene g."""
    for g in range(len(c.sizes)):
        for i, (got, want) in enumerate(zip(batch, alone[g])):
            assert same_bits(got[:, c.rows(g)], want), (what, c.name, g, i, float((got[:, c.rows(g)] - want).abs().max()))


# ------------------------------------------------------------------------------------------ the scripted rollout
@pytest.mark.parametrize("case_name,model_name", rrc.FORWARD)
def test_scripted_rollout_rows_are_each_scene_alone(dev, case_name, model_name):
    c, m = rrc.case(case_name), _model(model_name, dev)
    alone = _scripted_alone(case_name, model_name, dev)
    with torch.no_grad():
        eng = _ragged_engine(m, c.sizes, dev, c.max_nb)
        assert eng.ragged and eng.renumber is False and eng.offsets == [int(o) for o in c.offsets] and eng.rows(0) == c.rows(0)
        final, recs, edges = _scripted_batch(eng, c, dev)
        assert eng.n_rigid == sum(int(s.rigid.sum()) for s in c.scenes)
        _assert_rows_are_the_scenes(c, (final, recs), [a[:2] for a in alone], "scripted")
        assert edges == sum(a[2] for a in alone)
        again = _scripted_batch(eng, c, dev)                                           # twice on the same engine
        assert torch.equal(again[0], final) and torch.equal(again[1], recs) and again[2] == edges
        poison_allocator(dev, float("nan"))
        poisoned = _scripted_batch(_ragged_engine(m, c.sizes, dev, c.max_nb), c, dev)  # its workspace comes up full of NaN
        assert torch.equal(poisoned[0], final) and torch.equal(poisoned[1], recs)
    f = final.cpu().numpy()
    assert np.isfinite(f).all() and not np.array_equal(f[-1][:, L.cart_idx], c.window()[-1][:, L.cart_idx])


def test_equal_sizes_are_the_nodes_per_graph_engine(dev):
    c = rrc.case("equal")
    for model_name in rrc.CASE_MODELS["equal"]:
        m = _model(model_name, dev)
        with torch.no_grad():
            ragged = _scripted_batch(_ragged_engine(m, c.sizes, dev, c.max_nb), c, dev)
            batched = _scripted_batch(_single_engine(m, c.sizes[0], dev, c.max_nb, candidates=len(c.sizes)), c, dev)
        assert torch.equal(ragged[0], batched[0]) and torch.equal(ragged[1], batched[1]) and ragged[2] == batched[2], model_name


def test_one_graph_is_the_plain_call(dev):
    c = rrc.case("one")
    for model_name in rrc.CASE_MODELS["one"]:
        m = _model(model_name, dev)
        with torch.no_grad():
            ragged = _scripted_batch(_ragged_engine(m, c.sizes, dev, c.max_nb), c, dev)
            plain = _scripted_batch(_single_engine(m, c.sizes[0], dev, c.max_nb), c, dev)
        assert torch.equal(ragged[0], plain[0]) and torch.equal(ragged[1], plain[1]) and ragged[2] == plain[2], model_name


def test_steps_one_by_one_are_the_loop(dev):
    """gm_rollout_step_ragged step by step, with the prediction handed out, against gm_rollout_ragged; the predictions' rows
    against gm_rollout_step on each scene alone."""
    c, m = rrc.case("mixed"), _model("h128_sys", dev)
    with torch.no_grad():
        eng = _ragged_engine(m, c.sizes, dev, c.max_nb)
        final, _, _ = _scripted_batch(eng, c, dev)
        obs, traj = to_dev(c.window(), dev), to_dev(c.trajectory(), dev)
        eng.set_scene(obs)
        preds = torch.full((rrc.STEPS, eng.n, 3), float("nan"), device=dev)
        for t in range(rrc.STEPS):
            eng.step(obs, traj[t], pred_out=preds[t])
        eng.status()
        assert torch.equal(obs, final)
        for g, (s, tr) in enumerate(zip(c.scenes, c.trajectories())):
            one = _single_engine(m, s.n, dev, c.max_nb)
            o, tr = to_dev(s.window(), dev), to_dev(tr, dev)
            one.set_scene(o)
            for t in range(rrc.STEPS):
                p = torch.empty((s.n, 3), device=dev)
                one.step(o, tr[t], pred_out=p)
                assert same_bits(preds[t][c.rows(g)], p), (g, t)


# ------------------------------------------------------------------------------------------ the recorded rollout and its error sums
def _errors_ragged(rec, pred, sim, first, steps, offsets, fd, dev, sums=None):
    lb = _lib()
    off = (C.c_int64 * len(offsets))(*offsets)
    if sums is None:
        sums = torch.full((steps, len(offsets) - 1, 4), float("nan"), dtype=torch.float64, device=dev)
    rc = lb.lib().gm_rollout_errors_ragged(lb.ptr(rec), lb.ptr(pred), lb.ptr(sim), sim.shape[0], first, steps, off, len(offsets) - 1,
                                           C.byref(fd), lb.ptr(sums), lb.current_stream(dev))
    return rc, sums


@pytest.mark.parametrize("case_name,model_name", [("mixed", "h64"), ("mixed", "h128_sys"), ("single_row", "h128_sys"), ("clump", "h128_sys")])
def test_recorded_rollout_and_error_sums_are_each_scene_alone(dev, case_name, model_name):
    lb = _lib()
    c, m = rrc.case(case_name), _model(model_name, dev)
    alone = _recorded_alone(case_name, model_name, dev)
    fd = feature_desc(rrc.R, L)
    with torch.no_grad():
        eng = _ragged_engine(m, c.sizes, dev, c.max_nb)
        obs, frames = to_dev(c.window(), dev), to_dev(c.frames(), dev)
        eng.set_scene(obs)
        recs, preds = eng.run_recorded(obs, frames, rrc.STEPS, record=True, record_pred=True)
        eng.status()
        _assert_rows_are_the_scenes(c, (obs, recs, preds), alone, "recorded")
        plain = to_dev(c.window(), dev)
        assert eng.run_recorded(plain, frames, rrc.STEPS) == (None, None) and torch.equal(plain, obs)      # without records: the same
        sim = to_dev(c.recording(), dev)
        rc, sums = _errors_ragged(recs, preds, sim, L.k - 1, rrc.STEPS, [int(o) for o in c.offsets], fd, dev)
        assert rc == 0, lb.lib().gm_last_error()
        for g, s in enumerate(c.scenes):
            one = torch.full((rrc.STEPS, 1, 4), float("nan"), dtype=torch.float64, device=dev)
            rc = lb.lib().gm_rollout_errors(lb.ptr(alone[g][1]), lb.ptr(alone[g][2]), lb.ptr(to_dev(s.sim, dev)), s.sim.shape[0], L.k - 1,
                                            rrc.STEPS, s.n, C.byref(fd), lb.ptr(one), lb.current_stream(dev))
            assert rc == 0, lb.lib().gm_last_error()
            assert torch.equal(sums[:, g], one[:, 0]), (g, sums[:, g], one[:, 0])      # float64 sums in the same order: the same bits
        assert bool(torch.isfinite(sums).all()) and bool((sums[:, :, 0] >= sums[:, :, 1]).all())


# ------------------------------------------------------------------------------------------ evaluate_rollout
def test_evaluate_rollout_ragged_is_the_default_call(dev):
    from gnn_manip_amd import evaluate_rollout
    import gnn_manip_amd.rollout as ro
    scenes = rrc.eval_sims()
    assert len({s.n for s in scenes}) == 2
    m, ga = _model("h128_sys", dev), graph_attr(rrc.R, L)
    sims = [to_dev(np.ascontiguousarray(s.sim[:, :, :5]), dev) for s in scenes]          # as the dataset holds them: no control columns
    default = evaluate_rollout(sims, m, ga, k_steps=L.k)
    engines = []
    made = ro.RolloutEngine

    def counting(*a, **kw):
        engines.append(made(*a, **kw))
        return engines[-1]
    ro.RolloutEngine = counting
    try:
        ragged = evaluate_rollout(sims, m, ga, k_steps=L.k, ragged=True)
    finally:
        ro.RolloutEngine = made
    assert len(engines) == 1 and engines[0].sizes == [s.n for s in scenes]               # one group, one engine
    assert len(default) == len(ragged) == len(scenes)
    for i, (a, b) in enumerate(zip(default, ragged)):
        assert set(a) == set(b)
        for key in a:
            if isinstance(a[key], torch.Tensor):
                assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), (i, key)
            else:
                assert isinstance(b[key], float) and a[key] == b[key], (i, key)
        assert a["prediction"].shape[1] == scenes[i].n and np.isfinite(a["mean_sinkhorn"])


# ------------------------------------------------------------------------------------------ refusals
GM_ERR_INVALID_ARGUMENT, GM_ERR_WORKSPACE = -1, -4
ENTRIES = ("gm_rollout_step_ragged", "gm_rollout_ragged", "gm_rollout_recorded_ragged", "gm_rollout_errors_ragged")


@pytest.mark.parametrize("entry", ENTRIES)
def test_refusals_leave_the_outputs_untouched(dev, entry):
    lb = _lib()
    lib = lb.lib()
    c, m = rrc.case("mixed"), _model("h64", dev)
    n, steps = sum(c.sizes), rrc.STEPS
    eng = _ragged_engine(m, c.sizes, dev, c.max_nb)
    obs0 = to_dev(c.window(), dev)
    eng.set_scene(obs0)
    handle = m.device_handle(dev)
    frames, traj, sim = to_dev(c.frames(), dev), to_dev(c.trajectory(), dev), to_dev(c.recording(), dev)
    for name, (offsets, n_per, short) in rrc.refusals(c.sizes).items():
        if entry == "gm_rollout_errors_ragged" and name == "workspace":
            continue                                                                     # it has no workspace
        off = (C.c_int64 * len(offsets))(*offsets)
        G = len(offsets) - 1
        fd = feature_desc(rrc.R, L, n_per)
        obs = obs0.clone()
        outs = [torch.full((steps, n, L.D), -7.0, device=dev), torch.full((steps, n, 3), -7.0, device=dev),
                torch.full((steps, max(G, 1), 4), -7.0, dtype=torch.float64, device=dev)]
        ws, stream = eng.ws, lb.current_stream(dev)
        if entry == "gm_rollout_step_ragged":
            rc = lib.gm_rollout_step_ragged(handle, lb.ptr(obs), off, G, C.byref(fd), c.max_nb, lb.ptr(eng.rigid_rank), lb.ptr(traj[0]),
                                            lb.ptr(outs[1][0]), lb.ptr(ws), ws.numel() - short, stream)
        elif entry == "gm_rollout_ragged":
            rc = lib.gm_rollout_ragged(handle, lb.ptr(obs), off, G, C.byref(fd), c.max_nb, lb.ptr(eng.rigid_rank), lb.ptr(traj), steps,
                                       eng.n_rigid, steps, lb.ptr(outs[0]), lb.ptr(ws), ws.numel() - short, stream)
        elif entry == "gm_rollout_recorded_ragged":
            rc = lib.gm_rollout_recorded_ragged(handle, lb.ptr(obs), off, G, C.byref(fd), c.max_nb, lb.ptr(eng.rigid_rank), lb.ptr(frames),
                                                steps, lb.ptr(outs[0]), lb.ptr(outs[1]), lb.ptr(ws), ws.numel() - short, stream)
        else:
            rc = lib.gm_rollout_errors_ragged(lb.ptr(outs[0]), lb.ptr(outs[1]), lb.ptr(sim), sim.shape[0], L.k - 1, steps, off, G,
                                              C.byref(fd), lb.ptr(outs[2]), stream)
        assert rc == (GM_ERR_WORKSPACE if name == "workspace" else GM_ERR_INVALID_ARGUMENT), (entry, name, rc, lib.gm_last_error())
        assert lib.gm_last_error().startswith(entry.encode() + b": "), (entry, name, lib.gm_last_error())
        torch.cuda.synchronize(dev)
        assert torch.equal(obs, obs0) and all(bool((o == -7.0).all()) for o in outs), (entry, name)


def test_the_engine_refuses_what_a_ragged_batch_has_not(dev):
    from gnn_manip_amd import RolloutEngine
    m, ga = _model("h64", dev), graph_attr(rrc.R, L)
    kw = dict(k_steps=L.k, data_dim=L.D, device=dev)
    for bad in (dict(sizes=[5, 6], renumber=True), dict(sizes=[5, 6], candidates=2), dict(sizes=[]), dict(sizes=[5, 0]), dict(sizes=[1] * 65), {}):
        with pytest.raises(ValueError):
            RolloutEngine(m, ga, **kw, **bad)
    with pytest.raises(ValueError):
        RolloutEngine(m, ga, 11, sizes=[5, 6], **kw)
    eng = RolloutEngine(m, ga, sizes=[5, 6], **kw)
    obs = torch.zeros((L.k, 11, L.D), device=dev)
    eng.set_scene(obs)
    for call in (lambda: eng.differentiable_step(obs), lambda: eng.differentiable_rollout(obs, None, 1),
                 lambda: eng.differentiable_rollout(obs, None, 1, sweep="autograd"),
                 lambda: eng.rollout_candidates(obs, torch.zeros((1, 1, 0, 3), device=dev))):
        with pytest.raises(ValueError):
            call()
    plain = RolloutEngine(m, ga, 11, **kw)
    assert not plain.ragged and plain.offsets is None
    with pytest.raises(ValueError):
        plain.rows(0)


# ------------------------------------------------------------------------------------------ the loss of a ragged batch
def _loss_ragged(b, fd, dev, with_grads=True, frames=None):
    """gm_rollout_l1_loss_ragged through ctypes on a loss_batch: (status, losses [G], rows counted [G], d_records, d_final)."""
    lb = _lib()
    lib = lb.lib()
    G, n = len(b["sizes"]), sum(b["sizes"])
    windows, final = to_dev(b["windows"], dev), to_dev(b["final"], dev)
    frames = [to_dev(f, dev) for f in (b["frames"] if frames is None else frames)]
    rank = None if b["rank"] is None else to_dev(b["rank"], dev)
    off = (C.c_int64 * (G + 1))(*[int(o) for o in np.r_[0, np.cumsum(b["sizes"])]])
    views = (C.c_void_p * G)(*[f.data_ptr() for f in frames])
    scale = None if b["pos_scale"] is None else (C.c_double * 3)(*b["pos_scale"])
    steps, k = b["windows"].shape[:2]
    losses = torch.full((G,), -7.0, dtype=torch.float64, device=dev)
    counted = torch.full((G,), -7, dtype=torch.int64, device=dev)
    d_rec = torch.full((steps, n, b["windows"].shape[3]), float("nan"), device=dev) if with_grads else None
    d_fin = torch.full(tuple(b["final"].shape), float("nan"), device=dev) if with_grads else None
    need = lib.gm_rollout_l1_loss_ragged_workspace_bytes(G)
    ws = torch.full((need,), 0xAB, dtype=torch.uint8, device=dev)
    rc = lib.gm_rollout_l1_loss_ragged(lb.ptr(windows), lb.ptr(final), views, int(frames[0].shape[2]), steps, off, G, C.byref(fd), lb.ptr(rank),
                                       b["material_col"], scale, lb.ptr(losses), lb.ptr(counted), lb.ptr(d_rec), lb.ptr(d_fin), lb.ptr(ws), need,
                                       lb.current_stream(dev))
    return rc, losses, counted, d_rec, d_fin


def _loss_single(p, fd, dev):
    """gm_rollout_l1_loss on one graph's case alone: (loss, d_records, d_final)."""
    lb = _lib()
    lib = lb.lib()
    windows, final, frames = (to_dev(p[key], dev) for key in ("windows", "final", "frames"))
    rank = None if p["rank"] is None else to_dev(p["rank"], dev)
    steps, k, n, D = p["windows"].shape
    scale = None if p["pos_scale"] is None else (C.c_double * 3)(*p["pos_scale"])
    loss = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    d_rec, d_fin = torch.full((steps, n, D), float("nan"), device=dev), torch.full((k, n, D), float("nan"), device=dev)
    need = lib.gm_rollout_l1_loss_workspace_bytes(n, steps)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    rc = lib.gm_rollout_l1_loss(lb.ptr(windows), lb.ptr(final), lb.ptr(frames), int(frames.shape[2]), steps, n, C.byref(fd), lb.ptr(rank),
                                p["material_col"], scale, lb.ptr(loss), None, lb.ptr(d_rec), lb.ptr(d_fin), lb.ptr(ws), need,
                                lb.current_stream(dev))
    assert rc == 0, lib.gm_last_error()
    return loss, d_rec, d_fin


def _bits64(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, np.float64)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("mask", ["none", "rigid", "rigid_material", "empty"])
@pytest.mark.parametrize("frame_dim", [L.D, L.D - 3])
def test_ragged_loss_per_graph(dev, mask, frame_dim):
    import train_rollout_cases as trc
    b = rrc.loss_batch(L.k, frame_dim, mask)
    fd = feature_desc(rrc.R, L)
    rc, losses, counted, d_rec, d_fin = _loss_ragged(b, fd, dev)
    assert rc == 0, _lib().lib().gm_last_error()
    want = rrc.rollout_l1_restated_ragged(b["windows"], b["final"], b["frames"], b["sizes"], trc.LOSS_CART, b["rank"], b["material_col"],
                                          b["pos_scale"])
    got = losses.cpu().numpy()
    print(f"\n[ragged loss] {mask} frame_dim {frame_dim}: losses {got} restated {want[0]} rows {counted.cpu().numpy()}")
    assert np.array_equal(counted.cpu().numpy(), want[1])
    if mask == "empty":
        assert np.isnan(got).all()
    else:
        assert (np.abs(got - want[0]) <= rrc.LOSS_RTOL * np.abs(want[0])).all(), (got, want[0])
    assert same_bits(d_rec, want[2]) and same_bits(d_fin, want[3])
    off = np.r_[0, np.cumsum(b["sizes"])]
    for g, p in enumerate(b["parts"]):                                   # the single call on graph g alone: the same bits, the loss included
        loss, dr, df = _loss_single(p, fd, dev)
        rows = slice(int(off[g]), int(off[g + 1]))
        assert same_bits(d_rec[:, rows], dr) and same_bits(d_fin[:, rows], df), (mask, g)
        assert np.array_equal(_bits64(losses[g:g + 1]), _bits64(loss)), (mask, g, float(losses[g]), float(loss))
    rc2, only, _, none_r, none_f = _loss_ragged(b, fd, dev, with_grads=False)           # the loss alone
    assert rc2 == 0 and none_r is None and np.array_equal(_bits64(only), _bits64(losses))


@pytest.mark.parametrize("mask", rrc.LOSS_SHAPE_MASKS)
@pytest.mark.parametrize("frame_dim", [L.D, L.D - 3])
@pytest.mark.parametrize("shape", list(rrc.LOSS_SHAPES))
def test_ragged_loss_at_the_shapes_one_kernel_set_can_miss(dev, shape, frame_dim, mask):
    """test_ragged_loss_per_graph's assertions at ragged_rollout_cases.LOSS_SHAPES: a graph past one pass of the grid beside a
    one-row graph, and the table at its cap with graphs that count no row."""
    import train_rollout_cases as trc
    b = rrc.loss_shape(shape, L.k, frame_dim, mask)
    fd = feature_desc(rrc.R, L)
    rc, losses, counted, d_rec, d_fin = _loss_ragged(b, fd, dev)
    assert rc == 0, _lib().lib().gm_last_error()
    want = rrc.rollout_l1_restated_ragged(b["windows"], b["final"], b["frames"], b["sizes"], trc.LOSS_CART, b["rank"], b["material_col"],
                                          b["pos_scale"])
    got = losses.cpu().numpy()
    assert np.array_equal(counted.cpu().numpy(), want[1])
    some = want[1] > 0
    empty = tuple(int(g) for g in np.nonzero(~some)[0])
    assert empty == (rrc.LOSS_CAP_EMPTY if (shape, mask) == ("cap", "rigid_material") else ())
    err = np.abs(got[some] - want[0][some]) / np.abs(want[0][some])
    print(f"\n[ragged loss] {shape} {mask} frame_dim {frame_dim}: worst loss error / bound {(err / rrc.loss_rtol(rrc.LOSS_STEPS, want[1][some])).max():.3g}")
    assert np.isnan(got[~some]).all() and (err <= rrc.loss_rtol(rrc.LOSS_STEPS, want[1][some])).all(), (got, want[0])
    assert same_bits(d_rec, want[2]) and same_bits(d_fin, want[3])
    off = np.r_[0, np.cumsum(b["sizes"])]
    for g, p in enumerate(b["parts"]):                                   # the single call on graph g alone: the same bits, a NaN loss included
        loss, dr, df = _loss_single(p, fd, dev)
        rows = slice(int(off[g]), int(off[g + 1]))
        assert same_bits(d_rec[:, rows], dr) and same_bits(d_fin[:, rows], df), (shape, mask, g)
        assert np.array_equal(_bits64(losses[g:g + 1]), _bits64(loss)), (shape, mask, g, float(losses[g]), float(loss))
        if g in empty:
            assert not d_rec[:, rows].any() and not d_fin[:, rows].any(), g
    rc2, only, _, none_r, none_f = _loss_ragged(b, fd, dev, with_grads=False)           # the loss alone
    assert rc2 == 0 and none_r is None and np.array_equal(_bits64(only), _bits64(losses))


def test_a_scale_that_underflows_on_one_axis_leaves_the_other_axes(dev):
    """pos_scale[0] = 1e300: (float)(1 / ((scale_0 * steps) * count)) is zero, so axis 0's gradient elements are signed zeros while
    axes 1 and 2 keep theirs -- whether a graph counts any row is decided by its count, not by a scale.  The restatement, the
    single call and the batch agree bit for bit."""
    import train_rollout_cases as trc
    b = rrc.loss_batch(L.k, L.D, "rigid")
    b["pos_scale"] = (1e300, 2.0, 3.0)
    for p in b["parts"]:
        p["pos_scale"] = b["pos_scale"]
    fd = feature_desc(rrc.R, L)
    rc, losses, counted, d_rec, d_fin = _loss_ragged(b, fd, dev)
    assert rc == 0, _lib().lib().gm_last_error()
    want = rrc.rollout_l1_restated_ragged(b["windows"], b["final"], b["frames"], b["sizes"], trc.LOSS_CART, b["rank"], b["material_col"],
                                          b["pos_scale"])
    c0 = trc.LOSS_CART
    assert np.float32(1.0 / ((1e300 * rrc.LOSS_STEPS) * 1)) == 0 and (want[1] > 0).all()
    assert not want[3][-1][:, c0].any() and np.signbit(want[3][-1][:, c0]).any()               # axis 0: zeros of both signs
    assert all(np.count_nonzero(want[3][-1][:, c0 + ax]) >= int(want[1].sum()) - len(b["sizes"]) for ax in (1, 2))   # (one sign 0 per graph)
    assert same_bits(d_rec, want[2]) and same_bits(d_fin, want[3])
    got = losses.cpu().numpy()
    assert (np.abs(got - want[0]) <= rrc.LOSS_RTOL * np.abs(want[0])).all(), (got, want[0])
    off = np.r_[0, np.cumsum(b["sizes"])]
    for g, p in enumerate(b["parts"]):
        loss, dr, df = _loss_single(p, fd, dev)
        rows = slice(int(off[g]), int(off[g + 1]))
        assert same_bits(d_rec[:, rows], dr) and same_bits(d_fin[:, rows], df), g
        assert np.array_equal(_bits64(losses[g:g + 1]), _bits64(loss)), g


def test_a_nan_frame_stays_in_its_graph(dev):
    import train_rollout_cases as trc
    b = rrc.loss_batch(L.k, L.D, "rigid")
    fd = feature_desc(rrc.R, L)
    _, clean, _, _, _ = _loss_ragged(b, fd, dev)
    frames = [f.copy() for f in b["frames"]]
    row = int(np.nonzero(trc.counted_rows(b["parts"][1]["windows"], b["parts"][1]["rank"], -1))[0][0])
    frames[1][0, row, trc.LOSS_CART] = np.nan
    rc, losses, _, d_rec, d_fin = _loss_ragged(b, fd, dev, frames=frames)
    assert rc == 0
    got, want = losses.cpu().numpy(), clean.cpu().numpy()
    assert np.isnan(got[1]) and np.array_equal(_bits64(got[[0, 2]]), _bits64(want[[0, 2]])) and np.isfinite(want).all()
    assert rrc.batch_loss(got)[1] == 1 and np.isnan(rrc.batch_loss(got)[0])


# ------------------------------------------------------------------------------------------ the reverse sweep
def _sweep_setup(dev):
    import grad_cases as gc
    import rollout_grad_cases as rgc_
    c = rrc.case(rrc.SWEEP_CASE)
    m = load_model(rgc_.params(), gc.STEP_DIMS, dev)
    eng = _ragged_engine(m, c.sizes, dev, c.max_nb)
    return c, m, eng, rgc_.params()


def test_ragged_sweep_against_the_restated_sweep_per_graph(dev):
    """gm_rollout_backward_train_ragged: d_obs0 and d_trajectory of graph g against the float64 restated sweep
    (rollout_train_cases.reverse_sweep) of scene g alone on the device's edge lists, the parameter gradients against the sum over
    the graphs of those sweeps' -- the rule of tests/yardstick.py, the ReLU flip allowance of each scene's own input where the
    plain bound fails, summed over the scenes for a parameter."""
    import grad_cases as gc
    import rollout_train_cases as tc
    from gnn_manip_amd import get_connectivity
    from yardstick import compare, lazy, within
    c, m, eng, params = _sweep_setup(dev)
    steps, n = rrc.SWEEP_STEPS, sum(c.sizes)
    traj_np = c.trajectory(steps)
    w_final, w_records = gc.weights((L.k, n, L.D), rrc.W_FINAL_SEED), gc.weights((steps, n, L.D), rrc.W_RECORD_SEED)
    obs0 = to_dev(c.window(), dev)
    traj = to_dev(traj_np, dev)
    # the forward under autograd's library sweep: the Python surface of the ragged engine
    for p in m.parameters():
        p.grad = None
    leaf = obs0.clone().requires_grad_(True)
    tr_leaf = traj.clone().requires_grad_(True)
    final, recs = eng.differentiable_rollout(leaf, tr_leaf, horizon=steps, sweep="library", record=True, params=True)
    ((final * to_dev(w_final, dev)).sum() + (recs * to_dev(w_records, dev)).sum()).backward()
    d_obs0, d_traj = leaf.grad.cpu().numpy(), tr_leaf.grad.cpu().numpy()
    grads = {name: p.grad.detach().cpu().numpy() for name, p in m.named_parameters()}
    # the same forward's windows, and the device's own edge lists of every pre-step window, cut into the graphs'
    with torch.no_grad():
        obs = obs0.clone()
        eng.set_scene(obs)
        eis = []
        for t in range(steps):
            s, r = get_connectivity(obs[-1][:, L.cart:L.cart + 3].contiguous(), rrc.R, c.max_nb, graph_sizes=list(c.sizes))
            eis.append(torch.stack((s, r)).cpu().numpy())
            eng.step(obs, traj[t])
        assert torch.equal(obs, final.detach())
    at = np.r_[0, np.cumsum([int(s.rigid.sum()) for s in c.scenes])]
    sum64, sum32, allow_p = None, None, []
    for g, scene in enumerate(c.scenes):
        rows = c.rows(g)
        own = []
        for ei in eis:
            keep = (ei[0] >= rows.start) & (ei[0] < rows.stop)
            assert np.array_equal(keep, (ei[1] >= rows.start) & (ei[1] < rows.stop))          # no edge joins two graphs
            own.append(ei[:, keep] - rows.start)
        tg = traj_np[:, at[g]:at[g + 1]] if at[g + 1] > at[g] else None
        args = (params, scene.window(), tg, own, w_final[:, rows], w_records[:, rows])
        r64, r32 = tc.reverse_sweep(*args), tc.reverse_sweep(*args, dtype=torch.float32)

        def allowance(args=args, tg=tg, own=own):
            p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in args[0].items()}
            o = gc.t64(args[1], True)
            poses = None if tg is None else [gc.t64(t, True) for t in tg]

            def run(fwd):
                fin, rec = tc.unrolled(p, o, poses, own, forward=fwd)
                return tc.loss_of(fin, rec, args[4], args[5])
            bounds, units = gc.flip_allowance(run, [o] + (poses or []) + list(p.values()))
            nt = len(poses or [])
            return dict(obs=bounds[0], targets=bounds[1:1 + nt], params=dict(zip(p, bounds[1 + nt:])), units=units)
        allow = lazy(allowance)
        allow_p.append(allow)
        gc.split(f"ragged sweep graph {g}", d_obs0[:, rows], r64[2], r32[2], lambda a=allow: ([a()["obs"]], a()["units"]))
        if tg is not None:
            for t in range(steps):
                within(f"ragged sweep graph {g} d_trajectory[{t}]", d_traj[t, at[g]:at[g + 1]], r64[3][t], r32[3][t],
                       lambda a=allow, t=t: (a()["targets"][t], a()["units"]))
        sum64 = r64[4] if sum64 is None else {k: sum64[k] + v for k, v in r64[4].items()}
        sum32 = r32[4] if sum32 is None else {k: sum32[k] + v for k, v in r32[4].items()}
    worst, worst2 = compare(grads, sum64, sum32, lambda: ({k: sum(np.abs(a()["params"][k]).max() for a in allow_p) for k in sum64},
                                                          sum(a()["units"] for a in allow_p)), what="ragged sweep parameter gradients")
    print(f"\n[ragged sweep] parameters: worst tensor {worst[0]} err {worst[2]:.3e} tol {worst[3]:.3e}; with allowance {worst2}")


def test_ragged_sweep_input_gradients_are_each_scene_alone(dev):
    """Every launch of the sweep is per row or per edge: without parameter gradients, graph g's d_obs0 and d_trajectory have the
    bits of gm_rollout_backward_train on scene g alone; step_backward likewise; both extra inputs NULL gives the plain sweep."""
    import grad_cases as gc
    c, m, eng, _ = _sweep_setup(dev)
    steps, n = rrc.SWEEP_STEPS, sum(c.sizes)
    w_final, w_records = gc.weights((L.k, n, L.D), rrc.W_FINAL_SEED), gc.weights((steps, n, L.D), rrc.W_RECORD_SEED)
    at = np.r_[0, np.cumsum([int(s.rigid.sum()) for s in c.scenes])]

    def sweep(engine, window, traj, wf, wr):
        leaf, tl = to_dev(window, dev).requires_grad_(True), (None if traj is None else to_dev(traj, dev).requires_grad_(True))
        final, recs = engine.differentiable_rollout(leaf, tl, horizon=steps, sweep="library", record=True)
        loss = (final * to_dev(wf, dev)).sum() + (0.0 if wr is None else (recs * to_dev(wr, dev)).sum())
        loss.backward()
        return leaf.grad, (None if tl is None else tl.grad)
    d_obs0, d_traj = sweep(eng, c.window(), c.trajectory(steps), w_final, w_records)
    plain_obs0, _ = sweep(eng, c.window(), c.trajectory(steps), w_final, None)
    assert not torch.equal(plain_obs0, d_obs0)
    for g, s in enumerate(c.scenes):
        rows = c.rows(g)
        one = _single_engine(m, s.n, dev, c.max_nb)
        tg = c.trajectory(steps)[:, at[g]:at[g + 1]]
        a_obs, a_traj = sweep(one, s.window(), tg if tg.shape[1] else None, w_final[:, rows], w_records[:, rows])
        assert same_bits(d_obs0[:, rows], a_obs), g
        if tg.shape[1]:
            assert same_bits(d_traj[:, at[g]:at[g + 1]], a_traj), g
        b_obs, _ = sweep(one, s.window(), tg if tg.shape[1] else None, w_final[:, rows], None)
        assert same_bits(plain_obs0[:, rows], b_obs), g
    # one step through step_backward
    obs, tgt = to_dev(c.window(), dev), to_dev(c.trajectory(steps)[0], dev)
    eng.set_scene(obs)
    g_after = to_dev(w_final, dev)
    d_before, d_tgt, edges = eng.step_backward(obs, tgt, g_after, return_edge_count=True)
    total = 0
    for g, s in enumerate(c.scenes):
        rows = c.rows(g)
        one = _single_engine(m, s.n, dev, c.max_nb)
        o = to_dev(s.window(), dev)
        one.set_scene(o)
        t1 = tgt[at[g]:at[g + 1]].contiguous() if at[g + 1] > at[g] else None
        a, b, e = one.step_backward(o, t1, g_after[:, rows].contiguous(), return_edge_count=True)
        total += e
        assert same_bits(d_before[:, rows], a) and (t1 is None or same_bits(d_tgt[at[g]:at[g + 1]], b)), g
    assert edges == total                                                          # one edge count, the whole batch's


# ------------------------------------------------------------------------------------------ a training mini-batch as one rollout
LR = 1e-3


def _train_setup(dev, max_grad_norm=None, sand_only=True):
    from gnn_manip_amd import Trainer
    import train_step_cases as tsc
    c = rrc.case(rrc.SWEEP_CASE)
    dims, params, _, _ = rrc.model("h64")
    m = load_model(params, dims, dev)
    t = Trainer(m, lr=LR, sand_only=sand_only, material_col=tsc.MATERIAL_COL)
    t.max_grad_norm = max_grad_norm
    eng = _ragged_engine(m, c.sizes, dev, c.max_nb)
    obs0 = to_dev(c.window(), dev)
    eng.set_scene(obs0)
    frames = [to_dev(np.ascontiguousarray(s.sim[L.k:L.k + rrc.SWEEP_STEPS]), dev) for s in c.scenes]     # the frame that FOLLOWS each step
    return c, m, t, eng, obs0, frames


def _state(t):
    from gnn_manip_amd import train
    return [t.export(w) for w in (train.PARAMS, train.EXP_AVG, train.EXP_AVG_SQ)]


def _same_state(a, b, what):
    for kind, ta, tb in zip(("weights", "exp_avg", "exp_avg_sq"), a, b):
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert same_bits(u, v), (what, kind, i)


@pytest.mark.parametrize("max_grad_norm", [None, 1e-3])
def test_accumulate_rollout_batch_and_apply(dev, max_grad_norm):
    from conftest import STATS
    from gnn_manip_amd import train
    import train_accum_cases as ac
    import train_step_cases as tsc
    scale = [float(v) for v in STATS["acceleration_std"]]
    c, m, t, eng, obs0, frames = _train_setup(dev, max_grad_norm)
    G = len(c.sizes)
    w0 = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    before = _state(t)
    evaluated = torch.full((G,), -7.0, dtype=torch.float64, device=dev)
    t.evaluate_rollout_batch(eng, obs0, frames, rrc.SWEEP_STEPS, pos_scale=scale, losses_out=evaluated)       # no mini-batch begun: none needed
    _same_state(_state(t), before, "evaluate_rollout_batch changes nothing")
    own = torch.full((G,), -7.0, dtype=torch.float64, device=dev)
    t.zero_grad()
    t.accumulate_rollout_batch(eng, obs0, frames, rrc.SWEEP_STEPS, pos_scale=scale, losses_out=own)
    assert np.array_equal(_bits64(own), _bits64(evaluated)) and np.isfinite(own.cpu().numpy()).all()
    rec = t.accum_record()
    losses = own.cpu().numpy()
    assert (rec["samples"], rec["bad"]) == (G, 0) and rec["loss_sum"] == rrc.batch_loss(losses)[0]
    grads = [g.cpu().numpy() for g in t.export(train.GRADS)]
    assert any(g.any() for g in grads)
    slot, norm = torch.full((1,), -7.0, dtype=torch.float64, device=dev), torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    t.apply(loss_out=slot, norm_out=norm if max_grad_norm else None)
    want = rrc.batch_loss(losses)[0] / float(G)
    assert _bits64(slot)[0] == _bits64(np.float64(want).reshape(1))[0] and want == ac.mean_loss(losses), (float(slot), want)
    rec = t.accum_record()
    if max_grad_norm:
        host = ac.norm_of(grads, G)
        assert abs(rec["grad_norm"] - host) <= 1e-12 * host and rec["scale"] == float(ac.scale_of(rec["grad_norm"], G, max_grad_norm))
        assert host >= 1.5 * max_grad_norm                                                 # the clip is in force
    else:
        assert rec["scale"] == float(np.float32(1.0 / G))
    state = tsc.adam_state(w0)
    w1 = ac.scaled_adam_restated(w0, grads, state, LR, np.float32(rec["scale"]))
    _same_state(_state(t), (w1, state["m"], state["v"]), ("apply", max_grad_norm))
    assert t.record()["steps_applied"] == 1 and t.record()["steps_skipped"] == 0
    # each scene's loss is accumulate_rollout's on that scene alone
    single = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    for g, s in enumerate(c.scenes):
        one = _single_engine(m, s.n, dev, c.max_nb)
        o = to_dev(s.window(), dev)
        one.set_scene(o)
        fresh = _train_setup(dev)[2]
        fresh.evaluate_rollout(one, o, frames[g], rrc.SWEEP_STEPS, pos_scale=scale, loss_out=single)
        assert np.array_equal(_bits64(single), _bits64(own[g:g + 1])), g


def test_one_bad_graph_skips_the_whole_update(dev):
    c, m, t, eng, obs0, frames = _train_setup(dev)
    before = _state(t)
    bad = [f.clone() for f in frames]
    coffee = int(np.nonzero(~c.scenes[2].rigid)[0][0])
    bad[2][0, coffee, L.cart] = float("nan")
    own = torch.full((len(c.sizes),), -7.0, dtype=torch.float64, device=dev)
    t.zero_grad()
    t.accumulate_rollout_batch(eng, obs0, bad, rrc.SWEEP_STEPS, losses_out=own)
    rec = t.accum_record()
    got = own.cpu().numpy()
    assert (rec["samples"], rec["bad"]) == (len(c.sizes), 1) and np.isnan(got[2]) and np.isfinite(got[:2]).all()
    slot = torch.full((1,), -7.0, dtype=torch.float64, device=dev)
    t.apply(loss_out=slot)
    assert np.isnan(float(slot))
    _same_state(_state(t), before, "a skipped update")
    assert t.record()["steps_applied"] == 0 and t.record()["steps_skipped"] == 1


@pytest.mark.parametrize("max_grad_norm", [None, 1e-3])
def test_a_batch_of_one_scene_is_accumulate_rollout(dev, max_grad_norm):
    """A ragged batch of ONE scene through accumulate_rollout_batch + apply against accumulate_rollout + apply on a plain engine:
    the loss, the mini-batch's record, the gradients before apply and the state after it, bit for bit."""
    from conftest import STATS
    from gnn_manip_amd import Trainer, train
    import train_step_cases as tsc
    scale = [float(v) for v in STATS["acceleration_std"]]
    c = rrc.case(rrc.SWEEP_CASE)
    s = c.scenes[0]
    dims, params, _, _ = rrc.model("h64")

    def run(batched):
        m = load_model(params, dims, dev)
        t = Trainer(m, lr=LR, sand_only=True, material_col=tsc.MATERIAL_COL)
        t.max_grad_norm = max_grad_norm
        eng = _ragged_engine(m, (s.n,), dev, c.max_nb) if batched else _single_engine(m, s.n, dev, c.max_nb)
        obs0 = to_dev(s.window(), dev)
        assert eng.set_scene(obs0) > 0
        frames = to_dev(np.ascontiguousarray(s.sim[L.k:L.k + rrc.SWEEP_STEPS]), dev)
        loss, slot, norm = (torch.full((1,), -7.0, dtype=torch.float64, device=dev) for _ in range(3))
        t.zero_grad()
        if batched:
            t.accumulate_rollout_batch(eng, obs0, [frames], rrc.SWEEP_STEPS, pos_scale=scale, losses_out=loss)
        else:
            t.accumulate_rollout(eng, obs0, frames, rrc.SWEEP_STEPS, pos_scale=scale, loss_out=loss)
        t.accum_record()
        accumulated = t._pin_accum.numpy().copy()                          # the 48 bytes of the record
        grads = t.export(train.GRADS)
        t.apply(loss_out=slot, norm_out=norm if max_grad_norm else None)
        t.accum_record()
        return dict(loss=loss, accumulated=accumulated, grads=grads, slot=slot, norm=norm, applied=t._pin_accum.numpy().copy(),
                    state=_state(t), record=t.record())

    a, b = run(True), run(False)
    assert np.isfinite(float(a["loss"])) and any(bool(g.any()) for g in a["grads"])
    for key in ("loss", "slot", "norm"):
        assert np.array_equal(_bits64(a[key]), _bits64(b[key])), (key, float(a[key]), float(b[key]))
    assert np.array_equal(a["accumulated"], b["accumulated"]) and np.array_equal(a["applied"], b["applied"])
    assert int(a["accumulated"][0]) == 1 and int(a["accumulated"][1]) == 0                  # one sample, none of them bad
    for i, (u, v) in enumerate(zip(a["grads"], b["grads"])):
        assert same_bits(u, v), ("gradients", i)
    _same_state(a["state"], b["state"], ("apply", max_grad_norm))
    assert a["record"] == b["record"] and a["record"]["steps_applied"] == 1


def test_batch_methods_check_their_arguments(dev):
    c, m, t, eng, obs0, frames = _train_setup(dev)
    plain = _single_engine(m, sum(c.sizes), dev, c.max_nb)
    plain.set_scene(obs0)
    t.zero_grad()
    for call in (lambda: t.accumulate_rollout_batch(plain, obs0, frames), lambda: t.accumulate_rollout_batch(eng, obs0, frames[:2]),
                 lambda: t.accumulate_rollout_batch(eng, obs0, frames[::-1]), lambda: t.evaluate_rollout_batch(eng, obs0, frames, steps=9),
                 lambda: t.evaluate_rollout_batch(eng, obs0, frames, losses_out=torch.zeros(2, dtype=torch.float64, device=dev))):
        with pytest.raises(ValueError):
            call()
    fresh = _train_setup(dev)[2]
    from gnn_manip_amd._lib import GMError
    with pytest.raises(GMError, match="no mini-batch begun"):
        fresh.accumulate_rollout_batch(eng, obs0, frames)


# ------------------------------------------------------------------------------------------ an epoch of batched mini-batches
@pytest.fixture(scope="module")
def two_sizes(golden, dev, tmp_path_factory):
    """The recordings of tests/golden/g9_dataset.npz as a resident dataset, the second without its first twelve rows: 60 and 48
    nodes, ten rigid rows each (as test_gpu_train_accum.py builds them)."""
    import os
    from gnn_manip_amd import CoffeeDataset
    g = golden("g9_dataset.npz")
    root = str(tmp_path_factory.mktemp("g9_ragged_rollout")) + "/"
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")
    ds = CoffeeDataset(root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    sims = [ds.sims[0], ds.sims[1][:, 12:].contiguous()]
    assert [tuple(s.shape) for s in sims] == [(9, 60, 5), (9, 48, 5)]
    return CoffeeDataset.from_recordings(sims, 6, 0.015, ds.stats, ds.bounds, ds.cartesian_idx, ds.material_id, ds.control_idx, noise=3e-4,
                                         use_control=True)


@pytest.mark.parametrize("max_grad_norm", [None, 0.05])
def test_fit_rollout_epoch_batched(dev, two_sizes, max_grad_norm):
    from gnn_manip_amd import RolloutEngine, Trainer
    from oracle import epd_oracle as orc
    import train_step_cases as tsc
    ds = two_sizes
    dims = (25, 4, 3, 64, 2, 2)
    params = orc.init_params(*dims, 309)
    scale = [float(v) for v in ds.stats["acceleration_std"]]
    starts = [0, 1, 2, 3, 4]                                              # three windows of 60 nodes, then two of 48
    groups = [[0, 1], [2, 3], [4]]                                         # sizes (60, 60), (60, 48), (48,)

    def fresh():
        m = load_model(params, dims, dev)
        t = Trainer(m, lr=LR, sand_only=True, material_col=tsc.MATERIAL_COL)
        t.max_grad_norm = max_grad_norm
        return m, t
    # the manual loop: zero_grad / one cat / a ragged engine / set_scene / accumulate_rollout_batch / apply
    m, manual = fresh()
    losses, norms = torch.full((3,), -7.0, dtype=torch.float64, device=dev), torch.full((3,), float("nan"), dtype=torch.float64, device=dev)
    per_sample = []
    for u, group in enumerate(groups):
        samples = [ds.rollout_sample(start, 1, seed=5, stream=start) for start in group]
        eng = RolloutEngine(m, ds.graph_attr, k_steps=6, data_dim=8, device=dev, sizes=[int(w.shape[1]) for w, _ in samples])
        obs0 = torch.cat([w for w, _ in samples], dim=1).contiguous()
        eng.set_scene(obs0)
        own = torch.full((len(group),), -7.0, dtype=torch.float64, device=dev)
        manual.zero_grad()
        manual.accumulate_rollout_batch(eng, obs0, [f for _, f in samples], 1, pos_scale=scale, losses_out=own)
        manual.apply(loss_out=losses[u:u + 1], norm_out=norms[u:u + 1] if max_grad_norm else None)
        per_sample.append(own.cpu().numpy())
    want, want_norms = losses.cpu().numpy(), norms.cpu().numpy()
    _, t = fresh()
    got = t.fit_rollout_epoch(ds, None, 1, starts=starts, seed=5, pos_scale=scale, batch_size=2, batched=True)
    print(f"\n[ragged rollout] fit_rollout_epoch batched max_grad_norm={max_grad_norm}: {got} norms {t.last_epoch_grad_norms}")
    assert got.dtype == np.float64 and got.shape == (3,) and np.isfinite(got).all() and np.array_equal(_bits64(got), _bits64(want))
    assert t.last_epoch_grad_norms.shape == (3,) and np.array_equal(_bits64(t.last_epoch_grad_norms), _bits64(want_norms))
    assert np.isnan(want_norms).all() if max_grad_norm is None else (want_norms > 0).all()
    _same_state(_state(t), _state(manual), ("fit_rollout_epoch batched", max_grad_norm))
    assert t.record() == manual.record() and t.record()["steps_applied"] == 3
    # the unbatched epoch: its first update runs on the same weights, so its loss is the same per-sample losses added in the same order
    m2, plain = fresh()
    engines = {n: RolloutEngine(m2, ds.graph_attr, n, k_steps=6, data_dim=8, device=dev) for n in (60, 48)}
    unbatched = plain.fit_rollout_epoch(ds, engines, 1, starts=starts, seed=5, pos_scale=scale, batch_size=2)
    assert _bits64(unbatched[:1])[0] == _bits64(got[:1])[0], (unbatched, got)
    assert got[0] == (per_sample[0][0] + per_sample[0][1]) / 2.0
    np.testing.assert_allclose(got, unbatched, rtol=1e-3)                  # later updates: weights that differ by summation order
    # batched=False is the unbatched path, untouched
    m3, again = fresh()
    engines3 = {n: RolloutEngine(m3, ds.graph_attr, n, k_steps=6, data_dim=8, device=dev) for n in (60, 48)}
    same = again.fit_rollout_epoch(ds, engines3, 1, starts=starts, seed=5, pos_scale=scale, batch_size=2, batched=False)
    assert np.array_equal(_bits64(same), _bits64(unbatched))
    _same_state(_state(again), _state(plain), "batched=False")
