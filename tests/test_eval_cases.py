"""CPU: the restatements of tests/eval_cases.py against independent formulations, and the regimes of its cases.  The recorded
loop reproduces, on fixture G9's simulation, the loop that tests/test_gpu_dataset.py::test_compute_rollout_both_modes spells out
(copied here, not imported); the float64 sums give the RMSEs a direct np.sqrt(np.mean(...)) gives."""
import json

import numpy as np
import pytest

from oracle import epd_oracle as orc
import eval_cases as ec
import width_cases as wc


def test_recorded_loop_is_the_ground_truth_loop_of_the_dataset_test(golden):
    g = golden("g9_dataset.npz")
    meta = json.loads(bytes(g["meta_json"]).decode())
    data_dim, T, cart, ctrl, mat, bounds, stats = orc.read_metadata(meta)
    params = orc.init_params(25, 4, 3, 128, 2, 2, 44)
    params["decoder.4.weight"] = params["decoder.4.weight"] * 1e-2
    obs_list, _ = orc.dataset_samples([g["sims"][0].reshape(-1, data_dim)], T, data_dim, 6, cart, mat, True)
    rigid = obs_list[0][-1][:, mat] == 1
    steps = T - 6
    # --- the loop of test_compute_rollout_both_modes
    want = []
    cur = obs_list[0].copy()
    ci, ui = list(cart), list(ctrl)
    for i in range(steps):
        gt = obs_list[i][-1]
        new_rigid = cur[-1][rigid].copy()
        new_rigid[:, ui] = gt[rigid][:, ui]
        cur[-1][rigid] = new_rigid
        want.append(cur[-1].copy())
        nodes, ea, s, r, _ = orc.process(cur, None, stats, bounds, 0.015, cart, [mat], ctrl)
        acc = orc.epd_forward(params, nodes, ea, np.stack((s, r)), 2, 2)
        nxt = orc.get_position_from_prediction(stats, cart, acc, cur)
        cur[:-1] = cur[1:].copy()
        cur[-1][:, ci] = nxt
        new_rigid[:, ci] = gt[rigid][:, ci]
        cur[-1][rigid] = new_rigid
    # --- the restatement
    L = wc.LAYOUTS["default"]
    assert (L.cart_idx, [L.mat], L.ctrl_idx, L.D) == (ci, [mat], ui, obs_list[0].shape[2])
    frames = np.stack([obs_list[i][-1] for i in range(steps)])
    final, recs, preds = ec.recorded_loop(ec.oracle_predict(params, L, 2, 2, stats, bounds, 0.015), obs_list[0], frames, L, rigid, steps)
    assert steps >= 2 and 0 < rigid.sum() < len(rigid)
    assert np.array_equal(recs, np.stack(want)) and np.array_equal(final, cur)
    assert preds.shape == (steps, len(rigid), 3)
    assert np.array_equal(recs[0], frames[0])                              # the first record is the first recorded frame
    assert not np.array_equal(recs[1][~rigid][:, ci], frames[1][~rigid][:, ci])   # ... and later ones are predictions
    assert np.array_equal(recs[1][rigid][:, ci], frames[0][rigid][:, ci])  # the pose lags the window by one step


@pytest.mark.parametrize("case", ec.ROW_CASES, ids=ec.row_case_id)
def test_state_recorded_restatement(case):
    n, k, rigid, mapped = case
    L = ec.ROW_LAYOUTS[k]
    obs, frame, row_map = ec.row_inputs(n, k, mapped)
    rank = ec.rigid_rank(n, rigid)
    assert (rank >= 0).sum() == {"none": 0, "one": 1, "all": n}[rigid]
    assert (row_map is None) != mapped and (row_map is None or np.array_equal(np.sort(row_map), np.arange(n)))
    for what, cols in ((ec.GM_RECORDED_CONTROL, L.ctrl_idx), (ec.GM_RECORDED_POSE, L.cart_idx)):
        out = ec.state_recorded(obs, L, rank, frame, row_map, what)
        assert np.array_equal(out[:-1], obs[:-1])
        for j in range(n):                                             # row by row, the plain way
            row = obs[-1][j].copy()
            if rank[j] >= 0:
                row[cols] = frame[j if row_map is None else row_map[j]][cols]
            assert np.array_equal(out[-1][j], row)


def test_row_cases_cover_the_launch_edges():
    assert set(ec.SIZES) >= {1, 63, 64, 65, 257, 1000} and set(ec.KS) == {2, 6} and set(ec.RIGID) == {"none", "one", "all"}
    assert len(ec.ROW_CASES) == len(ec.SIZES) * 2 * 3 * 2
    for k, L in ec.ROW_LAYOUTS.items():
        assert L.k == k and L.ctrl >= 0


@pytest.mark.parametrize("name,route", ec.FUSED_CASES)
def test_fused_cases_are_in_their_regime(name, route):
    recs = [ec.fused_recording(name, c) for c in range(3)]
    hidden, nl, ms = ec.FUSED_MODELS[route]
    assert (hidden, nl) == (128, 2) if route == "systolic" else hidden == 64
    assert (recs[0].L.ctrl < 0) == (name == "no_control")
    for rec in recs:
        assert rec.n == ec.FUSED_N and 256 < rec.n < 512 and rec.n % 64                       # two workgroups, the last one ragged
        assert rec.T > rec.L.k + max(ec.FUSED_STEPS, ec.RENUMBER_STEPS)
        assert 0 < rec.rigid.sum() < rec.n and rec.coffee.sum() > 0 and (rec.rigid | rec.coffee).all()   # mixed
        assert ec.frames_are_tie_free(rec, ec.RENUMBER_STEPS)
        if rec.L.ctrl >= 0:
            ctl = rec.sim[:, :, rec.L.ctrl_idx]
            assert ctl[:-1][:, rec.rigid].any() and not ctl[:, ~rec.rigid].any()
    assert len({r.n for r in recs}) == 1 and not np.array_equal(recs[0].sim, recs[1].sim)        # a batch: equal N, different scenes


@pytest.mark.parametrize("case", ec.ERR_CASES, ids=lambda c: "rows%d-G%d-steps%d" % c)
def test_error_sums_give_the_direct_rmse(case):
    rows, graphs, steps = case
    L = ec.ERR_L
    rec, pred, sim, first = ec.error_inputs(rows, graphs, steps)
    assert rec.shape == (steps, rows * graphs, L.D) and first >= 1 and first + steps <= sim.shape[0] - 1
    sums = ec.error_sums(rec, pred, sim, first, steps, rows, L)
    assert sums.shape == (steps, graphs, 4) and sums.dtype == np.float64
    for g in range(graphs):
        sl = slice(g * rows, (g + 1) * rows)
        gt = sim[first:first + steps, sl]
        coffee = gt[0, :, L.mat] == 0
        assert np.array_equal(sums[:, g, 3], np.full(steps, coffee.sum()))
        d = rec[:, sl][:, :, L.cart_idx].astype(np.float64) - gt[:, :, L.cart_idx].astype(np.float64)
        a = np.stack([ec.acceleration_target(sim, first + i, L)[sl] for i in range(steps)])
        da = pred[:, sl].astype(np.float64) - a
        got = ec.rmse_from_sums(sums[:, g], rows)
        want = [np.sqrt(np.mean((d ** 2).sum(axis=-1))),
                np.sqrt(np.mean((d[:, coffee] ** 2).sum(axis=-1))) if coffee.any() else np.nan,
                np.sqrt(np.mean((da[:, coffee] ** 2).sum(axis=-1))) if coffee.any() else np.nan]
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0, equal_nan=True)
    # the target is the training target: compute_acceleration of the float32 oracle, to float32 rounding of its own
    p = lambda t: sim[t][:, L.cart_idx]
    a32 = ((p(first + 1) - p(first)) - (p(first) - p(first - 1)) - np.asarray(ec.STATS["acceleration_mean"], np.float32)) \
        / np.asarray(ec.STATS["acceleration_std"], np.float32)
    np.testing.assert_allclose(ec.acceleration_target(sim, first, L), a32, rtol=0, atol=2e-3 * np.abs(a32).max())


def test_error_case_without_coffee_has_none():
    rec, pred, sim, first = ec.error_inputs(65, 3, 5, coffee=False)
    assert not (sim[:, :, ec.ERR_L.mat] == 0).any() and (sim[:, :, ec.ERR_L.mat] == 1).any()
    sums = ec.error_sums(rec, pred, sim, first, 5, 65, ec.ERR_L)
    assert (sums[:, :, 0] > 0).all() and not sums[:, :, 1:].any()
    assert np.isnan(ec.rmse_from_sums(sums[:, 0], 65)[1:]).all()


def test_error_cases_cover_the_launch_edges():
    assert set(ec.ERR_ROWS) >= {1, 63, 64, 65, 257, 1000} and set(ec.ERR_GRAPHS) == {1, 3} and set(ec.ERR_STEPS) == {1, 5}
    assert max(ec.ERR_ROWS) <= 1000              # the bound behind SUM_RTOL: at most 1e3 terms per sum
    assert ec.SUM_RTOL == 1e-12
