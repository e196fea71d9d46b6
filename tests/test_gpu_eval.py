"""GPU: the evaluation path against the restatements of tests/eval_cases.py -- the recorded drive as stand-alone row kernels
(gm_state_recorded) and fused into the rollout loop (gm_rollout_recorded), the deterministic error sums (gm_rollout_errors) and
the public function on top (evaluate_rollout).  Copies of float32 values are compared bit for bit; the float64 sums at
eval_cases.SUM_RTOL; the renumbered loop at the bar of gm_rollout's renumbering tests; the loop against the float32 oracle at
the 2e-5 of the ground-truth test of tests/test_gpu_dataset.py."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

from conftest import STATS
from oracle import epd_oracle as orc
from gpu_support import dev, feature_desc, graph_attr, load_model, poison_allocator, rollout_engine, to_dev
import eval_cases as ec
import width_cases as wc

pytestmark = pytest.mark.gpu


def _lib():
    from gnn_manip_amd import _lib
    return _lib


def _state_recorded(obs, fd, rank, frame, row_map, what, dev):
    L = _lib()
    return L.lib().gm_state_recorded(L.ptr(obs), obs.shape[1], C.byref(fd), L.ptr(rank), L.ptr(frame), L.ptr(row_map), what, L.current_stream(dev))


# ------------------------------------------------------------------------------------------ row kernels
@pytest.mark.parametrize("case", ec.ROW_CASES, ids=ec.row_case_id)
def test_state_recorded_bit_for_bit(dev, case):
    n, k, rigid, mapped = case
    L = ec.ROW_LAYOUTS[k]
    obs, frame, row_map = ec.row_inputs(n, k, mapped)
    rank = ec.rigid_rank(n, rigid)
    fd = feature_desc(ec.R, L)
    for what in (ec.GM_RECORDED_CONTROL, ec.GM_RECORDED_POSE):
        o = to_dev(obs, dev)
        rc = _state_recorded(o, fd, to_dev(rank, dev), to_dev(frame, dev), None if row_map is None else to_dev(row_map, dev), what, dev)
        assert rc == 0, _lib().lib().gm_last_error()
        got = o.cpu().numpy()
        assert np.array_equal(got, ec.state_recorded(obs, L, rank, frame, row_map, what))
        assert np.array_equal(got[:-1], obs[:-1])                      # frames other than the last one are untouched


def test_state_recorded_refuses_control_without_control_columns(dev):
    L = wc.LAYOUTS["no_control"]
    obs = to_dev(np.zeros((L.k, 5, L.D), np.float32), dev)
    rank, frame = to_dev(np.zeros(5, np.int32), dev), to_dev(np.ones((5, L.D), np.float32), dev)
    fd = feature_desc(ec.R, L)
    assert _state_recorded(obs, fd, rank, frame, None, ec.GM_RECORDED_CONTROL, dev) == -1
    assert _lib().lib().gm_last_error() == b"gm_state_recorded: descriptor has no control columns"
    assert _state_recorded(obs, fd, rank, frame, None, ec.GM_RECORDED_POSE, dev) == 0
    assert not obs[:-1].any() and torch.equal(obs[-1][:, L.cart:L.cart + 3], torch.ones((5, 3), device=dev))


# ------------------------------------------------------------------------------------------ fused against the chain
def _engine(name, route, dev, candidates=1, **kw):
    L = wc.LAYOUTS[name]
    dims, params = ec.model_params(L, *ec.FUSED_MODELS[route])
    return rollout_engine(load_model(params, dims, dev), ec.R, L, ec.FUSED_N, dev, candidates=candidates, **kw)


def _chain(eng, obs0, frames, steps, dev):
    """Per step: gm_state_recorded(CONTROL), a copy of the last frame, gm_rollout_step(rigid_rank = NULL, pred_acc_out),
    gm_state_recorded(POSE)."""
    obs = obs0.clone()
    eng.set_scene(obs)
    recs, preds = [], []
    for i in range(steps):
        if eng.fdesc.control_col >= 0:
            assert _state_recorded(obs, eng.fdesc, eng.rigid_rank, frames[i], None, ec.GM_RECORDED_CONTROL, dev) == 0
        recs.append(obs[-1].clone())
        p = torch.empty((eng.n, 3), device=dev)
        eng.step(obs, None, pred_out=p, use_rigid=False)
        preds.append(p)
        assert _state_recorded(obs, eng.fdesc, eng.rigid_rank, frames[i], None, ec.GM_RECORDED_POSE, dev) == 0
    assert eng.status() > 10 * eng.n
    return obs, torch.stack(recs), torch.stack(preds)


def _fused(eng, obs0, frames, steps):
    obs = obs0.clone()
    eng.set_scene(obs)
    recs, preds = eng.run_recorded(obs, frames, steps, record=True, record_pred=True)
    assert eng.status() > 10 * eng.n
    return obs, recs, preds


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,route", ec.FUSED_CASES)
def test_recorded_rollout_is_the_chain_bit_for_bit(dev, name, route):
    rec = ec.fused_recording(name)
    steps = ec.FUSED_STEPS
    obs0, frames = to_dev(rec.window(), dev), to_dev(rec.frames(steps), dev)
    with torch.no_grad():
        eng = _engine(name, route, dev)
        assert eng.n_rigid == 0 and eng.renumber is False
        traj = to_dev(wc.drift_trajectory(rec.window(), rec.L, 2, 880), dev)
        scripted_before = eng.rollout(obs0, traj, horizon=2, record=True)
        chain = _chain(eng, obs0, frames, steps, dev)
        assert eng.n_rigid == int(rec.rigid.sum()) > 0
        fused = _fused(eng, obs0, frames, steps)
        assert _same(fused, chain), [float((a - b).abs().max()) for a, b in zip(fused, chain)]
        assert _same(_fused(eng, obs0, frames, steps), fused)                       # twice
        poison_allocator(dev, float("nan"))
        poisoned = _engine(name, route, dev)                                         # its workspace comes up full of NaN
        assert _same(_fused(poisoned, obs0, frames, steps), fused)
        scripted_after = eng.rollout(obs0, traj, horizon=2, record=True)
        assert _same(scripted_after, scripted_before)                                # the unchanged gm_rollout on the same engine
        # without records the rollout is the same
        plain = obs0.clone()
        assert eng.run_recorded(plain, frames, steps) == (None, None) and torch.equal(plain, fused[0])
    final, recs, preds = (x.cpu().numpy() for x in fused)
    assert np.isfinite(final).all() and np.isfinite(preds).all() and preds.any()
    assert np.array_equal(recs[0], rec.frames(1)[0] if rec.L.ctrl >= 0 else rec.window()[-1])
    ci = rec.L.cart_idx
    assert np.array_equal(final[-1][rec.rigid][:, ci], rec.frames(steps)[-1][rec.rigid][:, ci])      # the pose of the LAST frame read
    assert not np.array_equal(final[-1][~rec.rigid][:, ci], rec.frames(steps)[-1][~rec.rigid][:, ci])


def test_recorded_batch_of_three_is_three_single_rollouts(dev):
    name, route, steps = "default", "systolic", ec.FUSED_STEPS
    recs = [ec.fused_recording(name, c) for c in range(3)]
    n = ec.FUSED_N
    with torch.no_grad():
        one = _engine(name, route, dev)
        singles = [_fused(one, to_dev(r.window(), dev), to_dev(r.frames(steps), dev), steps) for r in recs]
        obs0 = to_dev(np.concatenate([r.window() for r in recs], axis=1), dev)
        frames = to_dev(np.concatenate([r.frames(steps) for r in recs], axis=1), dev)
        batch = _fused(_engine(name, route, dev, candidates=3), obs0, frames, steps)
    for c in range(3):
        for got, want in zip(batch, singles[c]):
            assert torch.equal(got[:, c * n:(c + 1) * n], want), c
    assert not torch.equal(singles[0][1], singles[1][1])


def test_renumbered_recorded_rollout(dev):
    """renumber_every = 2 over five steps against the plain loop: rows in grid-cell order sum a node's messages in another order
    (float32 rounding, 2e-6 of the frame's largest coordinate as for gm_rollout); records and predictions come back in the
    caller's numbering.  A prediction p enters a position as p * acc_std next to the two frames before it, so predictions that
    give positions inside the bar lie inside 4 bars / acc_std of each other."""
    name, route, steps = "default", "systolic", ec.RENUMBER_STEPS
    rec = ec.fused_recording(name)
    perm = np.random.default_rng(890).permutation(rec.n)               # rigid rows scattered over the caller's numbering
    window, frames_np = rec.window()[:, perm], rec.frames(steps)[:, perm]
    obs0, frames = to_dev(window, dev), to_dev(frames_np, dev)
    with torch.no_grad():
        plain = _fused(_engine(name, route, dev, renumber=False), obs0, frames, steps)
        ren = _engine(name, route, dev, renumber=True)
        ren.RENUMBER_EVERY = ec.RENUMBER_EVERY
        got = _fused(ren, obs0, frames, steps)
        assert ren.renumber and _same(_fused(ren, obs0, frames, steps), got)
    L = rec.L
    other = [c for c in range(L.D) if c not in L.cart_idx]
    names = ("final", "records", "predictions")
    (f0, r0, p0), (f1, r1, p1) = ([x.cpu().numpy() for x in t] for t in (plain, got))
    bar = ec.RENUMBER_BAR * float(np.abs(f0[..., L.cart_idx]).max())
    for what, a, b in zip(names, (f1, r1), (f0, r0)):
        err = float(np.abs(a[..., L.cart_idx] - b[..., L.cart_idx]).max())
        print(f"renumbered recorded {what}: max |renumbered - plain| = {err:.3e} (bar {bar:.3e})")
        assert err <= bar, (what, err, bar)
        assert np.array_equal(a[..., other], b[..., other]), what
    err_p = float(np.abs(p1 - p0).max())
    bar_p = 4.0 * bar / min(STATS["acceleration_std"])
    print(f"renumbered recorded predictions: max |renumbered - plain| = {err_p:.3e} (bar {bar_p:.3e}), |pred| <= {np.abs(p0).max():.3e}")
    assert err_p <= bar_p
    # step 0 starts from identical states: its prediction differs by summation order alone (each within the forward's 1e-5 of the
    # exact value, so within 1e-4 of each other with room) -- in the CALLER's numbering, not in another one
    assert np.abs(p1[0] - p0[0]).max() <= 1e-4 * np.abs(p0[0]).max() < np.abs(p1[0] - p0[0][::-1]).max()


# ------------------------------------------------------------------------------------------ against the reference loop
def _write_dataset(g, root):
    """The synthetic dataset fixture G9 was generated from (the bytes tests/golden/make_golden.py wrote)."""
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")


@pytest.fixture(scope="module")
def g9(golden, dev, tmp_path_factory):
    from gnn_manip_amd import CoffeeTestDataset
    g = golden("g9_dataset.npz")
    root = str(tmp_path_factory.mktemp("g9")) + "/"
    _write_dataset(g, root)
    ds = CoffeeTestDataset(root, 6, 0.015, split="train", device=dev, use_control=True, sim_id=1)
    params = orc.init_params(25, 4, 3, 128, 2, 2, 44)
    params["decoder.4.weight"] = params["decoder.4.weight"] * 1e-2
    return g, ds, params, load_model(params, (25, 4, 3, 128, 2, 2), dev)


def test_run_recorded_against_the_reference_loop(dev, g9):
    g, ds, params, m = g9
    meta = json.loads(bytes(g["meta_json"]).decode())
    data_dim, T, cart, ctrl, mat, bounds, stats = orc.read_metadata(meta)
    obs_list, _ = orc.dataset_samples([g["sims"][0].reshape(-1, data_dim)], T, data_dim, 6, cart, mat, True)
    L = wc.LAYOUTS["default"]
    steps = T - 6
    rigid = obs_list[0][-1][:, mat] == 1
    frames = np.stack([obs_list[i][-1] for i in range(steps)])
    _, ref_recs, ref_preds = ec.recorded_loop(ec.oracle_predict(params, L, 2, 2, stats, bounds, 0.015), obs_list[0], frames, L, rigid, steps)
    from gnn_manip_amd import RolloutEngine
    from gnn_manip_amd.rollout import extract_groundtruth
    with torch.no_grad():
        obs0, _ = ds[0]
        eng = RolloutEngine(m, ds.graph_attr, obs0.shape[1], k_steps=6, data_dim=obs0.shape[2], device=dev)
        obs = obs0.clone().contiguous()
        eng.set_scene(obs)
        gt = extract_groundtruth(ds, steps).contiguous()
        assert np.array_equal(gt.cpu().numpy(), frames)
        recs, preds = eng.run_recorded(obs, gt, record=True, record_pred=True)
        eng.status()
    err = float(np.abs(recs.cpu().numpy() - ref_recs).max())
    print(f"run_recorded records against the oracle loop: max |diff| = {err:.3e}")
    np.testing.assert_allclose(recs.cpu().numpy(), ref_recs, rtol=0, atol=2e-5)
    assert preds.shape == ref_preds.shape and np.isfinite(preds.cpu().numpy()).all()


def test_compute_rollout_keeps_the_bits_of_the_python_loop(dev, g9):
    """compute_rollout(cma_traj=None) is one gm_rollout_recorded call; the loop it replaced -- eng.step between tensor-indexing
    overwrites, restated here -- gives the same bits."""
    from gnn_manip_amd import RolloutEngine
    from gnn_manip_amd.rollout import compute_rollout, extract_groundtruth
    g, ds, params, m = g9
    got = compute_rollout(ds, m, types.SimpleNamespace(cma_traj=None, k_steps=6, device=dev, plot=False))
    with torch.no_grad():
        obs0, _ = ds[0]
        k, n, dd = obs0.shape
        nof_steps = ds.time_steps - 6
        eng = RolloutEngine(m, ds.graph_attr, n, k_steps=k, data_dim=dd, max_neighbours=20, device=dev)
        obs = obs0.clone().contiguous()
        eng.set_scene(obs)
        rigid = obs[0, :, ds.material_id] == 1
        c0, u0 = ds.cartesian_idx[0], ds.control_idx[0]
        groundtruth = extract_groundtruth(ds, nof_steps)
        prediction = []
        for i in range(nof_steps):
            obs[-1, rigid, u0:u0 + 3] = groundtruth[i, rigid, u0:u0 + 3]
            prediction.append(obs[-1].clone())
            eng.step(obs, None, use_rigid=False)
            new_rigid = prediction[-1][rigid].clone()
            new_rigid[:, c0:c0 + 3] = groundtruth[i, rigid, c0:c0 + 3]
            obs[-1, rigid] = new_rigid
        eng.status()
        want = torch.stack(prediction).cpu().numpy().astype(np.float64)
    assert got.dtype == want.dtype and got.shape == want.shape == (nof_steps, n, dd) and nof_steps >= 2
    assert np.array_equal(got, want), float(np.abs(got - want).max())
    assert 0 < int(rigid.sum()) < n


# ------------------------------------------------------------------------------------------ gm_rollout_errors
def _errors(rec, pred, sim, first, steps, fd, dev, sums=None):
    L = _lib()
    n = rec.shape[1]
    graphs = n // fd.nodes_per_graph if fd.nodes_per_graph else 1
    if sums is None:
        sums = torch.full((steps, graphs, 4), float("nan"), dtype=torch.float64, device=dev)
    rc = L.lib().gm_rollout_errors(L.ptr(rec), L.ptr(pred), L.ptr(sim), sim.shape[0], first, steps, n, C.byref(fd), L.ptr(sums),
                                   L.current_stream(dev))
    return rc, sums


def _assert_sums(got, want):
    got = got.cpu().numpy()
    assert np.array_equal(got[..., 3], want[..., 3])                   # counts are exact
    np.testing.assert_allclose(got[..., :3], want[..., :3], rtol=ec.SUM_RTOL, atol=0)


@pytest.mark.parametrize("case", ec.ERR_CASES, ids=lambda c: "rows%d-G%d-steps%d" % c)
def test_rollout_errors_against_float64_numpy(dev, case):
    rows, graphs, steps = case
    rec, pred, sim, first = ec.error_inputs(rows, graphs, steps)
    fd = feature_desc(ec.R, ec.ERR_L, rows if graphs > 1 else 0)
    want = ec.error_sums(rec, pred, sim, first, steps, rows, ec.ERR_L)
    assert (want[..., :3] > 0).all() or rows < 63
    d = [to_dev(a, dev) for a in (rec, pred, sim)]
    rc, got = _errors(d[0], d[1], d[2], first, steps, fd, dev)
    assert rc == 0, _lib().lib().gm_last_error()
    _assert_sums(got, want)
    rc, again = _errors(d[0], d[1], d[2], first, steps, fd, dev)
    assert rc == 0 and torch.equal(again, got)                         # two calls, the same bits
    rc, no_pred = _errors(d[0], None, d[2], first, steps, fd, dev)
    assert rc == 0 and torch.equal(no_pred[..., [0, 1, 3]], got[..., [0, 1, 3]]) and not no_pred[..., 2].any()


def test_rollout_errors_without_coffee_rows(dev):
    rec, pred, sim, first = ec.error_inputs(65, 3, 5, coffee=False)
    rc, got = _errors(to_dev(rec, dev), to_dev(pred, dev), to_dev(sim, dev), first, 5, feature_desc(ec.R, ec.ERR_L, 65), dev)
    assert rc == 0
    _assert_sums(got, ec.error_sums(rec, pred, sim, first, 5, 65, ec.ERR_L))
    assert (got[..., 0] > 0).all() and not got[..., 1:].any()


def test_rollout_errors_keep_a_nan_to_its_step_and_graph(dev):
    rows, graphs, steps = 257, 3, 5
    rec, pred, sim, first = ec.error_inputs(rows, graphs, steps)
    want = ec.error_sums(rec, pred, sim, first, steps, rows, ec.ERR_L)
    coffee_row = rows + int(np.nonzero(sim[0, rows:2 * rows, ec.ERR_L.mat] == 0)[0][0])       # a coffee row of graph 1
    for value in (np.nan, np.inf):
        bad = rec.copy()
        bad[2, coffee_row, ec.ERR_L.cart + 1] = value
        rc, got = _errors(to_dev(bad, dev), to_dev(pred, dev), to_dev(sim, dev), first, steps, feature_desc(ec.R, ec.ERR_L, rows), dev)
        assert rc == 0
        got = got.cpu().numpy()
        hit = np.zeros((steps, graphs), bool)
        hit[2, 1] = True
        assert not np.isfinite(got[hit][:, :2]).any() and np.isfinite(got[hit][:, 2:]).all()
        assert np.isfinite(got[~hit]).all()
        np.testing.assert_allclose(got[~hit], want[~hit], rtol=ec.SUM_RTOL, atol=0)


@pytest.mark.parametrize("first,steps,with_pred", [(0, 1, True), (1, 7, True), (3, 5, True), (7, 1, True), (0, 9, False), (4, 5, False),
                                                   (9, 0, False), (-1, 2, False)])
def test_rollout_errors_refuses_out_of_range_frames(dev, first, steps, with_pred):
    rec, pred, sim, _ = ec.error_inputs(64, 1, 5)                      # a recording of 8 frames
    assert sim.shape[0] == 8
    room = max(steps, 1)
    rec_d = to_dev(np.zeros((room,) + rec.shape[1:], np.float32), dev)
    pred_d = to_dev(np.zeros((room,) + pred.shape[1:], np.float32), dev) if with_pred else None
    sums = torch.full((room, 1, 4), -7.0, dtype=torch.float64, device=dev)
    rc, _ = _errors(rec_d, pred_d, to_dev(sim, dev), first, steps, feature_desc(ec.R, ec.ERR_L), dev, sums)
    assert rc == -1 and _lib().lib().gm_last_error().startswith(b"gm_rollout_errors: ")
    torch.cuda.synchronize(dev)
    assert bool((sums == -7.0).all())                                  # refused before anything ran


# ------------------------------------------------------------------------------------------ evaluate_rollout
EVAL_STEPS = 5


@pytest.fixture(scope="module")
def evaluation(dev):
    """Three recordings, two of equal N (one batch) and one smaller (a group of its own), evaluated together once."""
    from gnn_manip_amd import evaluate_rollout
    L = wc.LAYOUTS["default"]
    recs = [ec.Recording("default", n, L.k + EVAL_STEPS, 950 + i, side=0.04) for i, n in enumerate((151, 151, 120))]
    dims, params = ec.model_params(L, 128, 2, 2)
    m = load_model(params, dims, dev)
    ga = graph_attr(ec.R, L)
    sims = [to_dev(np.ascontiguousarray(r.sim[:, :, :5]), dev) for r in recs]       # as the dataset holds them: no control columns
    return recs, m, ga, sims, evaluate_rollout(sims, m, ga, k_steps=L.k)


def test_evaluate_rollout_scalars_and_records(dev, evaluation):
    recs, m, ga, sims, out = evaluation
    L = wc.LAYOUTS["default"]
    assert len(out) == 3
    for rec, res in zip(recs, out):
        pred, gt, acc = (res[key].cpu().numpy() for key in ("prediction", "groundtruth", "acceleration"))
        assert pred.shape == gt.shape == (EVAL_STEPS, rec.n, L.D) and acc.shape == (EVAL_STEPS, rec.n, 3)
        assert np.array_equal(gt, rec.frames(EVAL_STEPS))                # control columns included, as the dataset's windows have them
        assert np.array_equal(pred[0], gt[0])
        assert not np.array_equal(pred[1][:, L.cart_idx], gt[1][:, L.cart_idx])
        want = ec.error_sums(pred, acc, rec.sim, L.k - 1, EVAL_STEPS, rec.n, L)[:, 0]
        sums = res["sums"].numpy()
        assert sums.dtype == np.float64 and np.array_equal(sums[:, 3], want[:, 3]) and sums[0, 3] == rec.coffee.sum() > 0
        np.testing.assert_allclose(sums[:, :3], want[:, :3], rtol=ec.SUM_RTOL, atol=0)
        scalars = [res["rmse_position"], res["rmse_position_coffee"], res["rmse_acceleration"]]
        np.testing.assert_allclose(scalars, ec.rmse_from_sums(want, rec.n), rtol=1e-12, atol=0)
        assert all(isinstance(v, float) and v > 0 for v in scalars)


def test_evaluate_rollout_sinkhorn_is_the_single_call(dev, evaluation):
    from gnn_manip_amd import evaluate_rollout
    from gnn_manip_amd.losses import SamplesLoss
    recs, m, ga, sims, out = evaluation
    L = wc.LAYOUTS["default"]
    loss = SamplesLoss("sinkhorn", p=2, blur=0.05)
    blocked = evaluate_rollout(sims, m, ga, k_steps=L.k, pair_block=2)
    for rec, res, res2 in zip(recs, out, blocked):
        s = res["sinkhorn"]
        assert s.shape == (EVAL_STEPS,) and s.dtype == torch.float32 and s.device == dev
        coffee = to_dev(np.nonzero(rec.coffee)[0], dev)
        for i in (0, EVAL_STEPS // 2, EVAL_STEPS - 1):
            gt_i = res["groundtruth"][i][coffee][:, L.cart:L.cart + 3].contiguous()
            pred_i = res["prediction"][i][coffee][:, L.cart:L.cart + 3].contiguous()
            assert torch.equal(s[i], loss(gt_i, pred_i)), i
        assert torch.equal(res2["sinkhorn"], s) and torch.equal(res2["prediction"], res["prediction"])
        assert abs(float(s[0])) < 1e-6                                      # the first record is the ground truth: S(x, x) = 0
        assert res["mean_sinkhorn"] == float(s.double().mean()) and np.isfinite(res["mean_sinkhorn"])


def test_evaluate_rollout_groups_match_stand_alone_evaluations(dev, evaluation):
    from gnn_manip_amd import evaluate_rollout
    recs, m, ga, sims, out = evaluation
    for i, res in enumerate(out):
        alone = evaluate_rollout([sims[i]], m, ga, k_steps=wc.LAYOUTS["default"].k)[0]
        for key in ("prediction", "groundtruth", "acceleration", "sinkhorn", "sums"):
            assert torch.equal(alone[key], res[key]), (i, key)
        for key in ("rmse_position", "rmse_position_coffee", "rmse_acceleration", "mean_sinkhorn"):
            assert alone[key] == res[key], (i, key)


def test_evaluate_rollout_takes_a_dataset_and_skips_sinkhorn(dev, g9):
    from gnn_manip_amd import evaluate_rollout
    from gnn_manip_amd.rollout import compute_rollout
    g, ds, params, m = g9
    res, = evaluate_rollout(ds, m, sinkhorn=False)
    assert "sinkhorn" not in res
    want = compute_rollout(ds, m, types.SimpleNamespace(cma_traj=None, k_steps=6, device=dev, plot=False))
    assert np.array_equal(res["prediction"].cpu().numpy().astype(np.float64), want)
