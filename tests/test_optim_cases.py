"""CPU: the cases of tests/optim_cases.py hold what they are named for, the restated drive is sensitive to the treatments the
contract rules out, and it agrees with float64 torch -- what tests/test_gpu_optim.py holds the kernels to, bit for bit, is checked
here first.

Bounds.  The conditions on the schedules are conditions on the INPUTS (fractions of denormal or inf entries of the restatement's
own state), with seeds chosen so that each holds with room to spare.  Sensitivity: a wrong treatment changes at least 1 % of the
words of a state array.  Against float64 ``torch.optim.Adam``: the rule of test_adam_restatement_against_float64_torch, an error
of at most 4 x float32 torch's own.  The beta powers: bit equality."""
import numpy as np
import pytest
import torch

import optim_cases as oc
import train_step_cases as sc

LR = 1e-3


def _run(name, lay, steps=oc.STEPS, world=1, samples=1, wrong=None, eps=1e-8, max_grad_norm=None):
    """The restated drive over a schedule: (final state, the weights after every step, the records)."""
    rows = oc.rank_rows(name, lay, steps, world)
    state = oc.start_state(lay)
    weights, recs = [state["p"]], []
    for k in range(steps):
        recs.append(oc.drive_restated(state, rows[k], oc.tails_of(samples, world, state["steps"]), samples, LR, max_grad_norm, eps=eps,
                                      wrong=wrong))
        weights.append(state["p"])
    return state, weights, recs


# ---------------------------------------------------------------------------------------------- the layout
def test_layout_is_the_flat_buffers():
    tails = []
    for dims in oc.TAIL_MODELS + (oc.BIG,):
        lay = oc.Layout(dims)
        assert lay.count == sc.flat_count(dims) and lay.alloc == (lay.count + 3) // 4 * 4 and lay.alloc - lay.count < 4
        assert all(o % 4 == 0 for o in lay.offsets) and int(lay.used.sum()) == sum(lay.counts)
        tails.append(lay.count % 4)
    assert tails[:4] == [1, 2, 3, 0]
    big = oc.Layout(oc.BIG)
    assert oc.GRID_PASS == 2_097_152 and oc.GRID_PASS < big.count < 2 * oc.GRID_PASS and big.count % 4 == 3
    beyond = big.beyond(oc.GRID_PASS)
    assert len(beyond) >= 4 and sum(big.counts[i] for i in beyond) > 50_000 and max(big.counts[i] for i in beyond) >= 65_536
    from gnn_manip_amd import EncProcDecGNN
    for dims in oc.TAIL_MODELS + (oc.BIG,):
        assert [tuple(p.shape) for p in EncProcDecGNN(*dims).parameters()] == oc.Layout(dims).shapes
    lay = oc.Layout(oc.OD3)
    tensors = [np.full(s, i + 1, np.float32) for i, s in enumerate(lay.shapes)]
    flat = lay.to_flat(tensors)
    assert flat.shape == (lay.alloc,) and not flat[~lay.used].any() and flat[lay.used].all()
    assert all(np.array_equal(a, b) for a, b in zip(lay.from_flat(flat), tensors))
    assert np.array_equal(lay.packed(flat), np.concatenate([a.reshape(-1) for a in tensors]))
    for name in oc.SCHEDULES:
        g = oc.schedule(name, lay, 4)
        assert g.shape == (4, lay.alloc) and g.dtype == np.float32 and not g[:, ~lay.used].any()


# ---------------------------------------------------------------------------------------------- the schedules
def test_each_schedule_has_the_property_it_is_named_for():
    lay = oc.Layout(oc.OD3)
    n = int(lay.used.sum())
    for name in ("mixed", "tiny", "huge", "decay"):
        state, weights, recs = _run(name, lay)
        c = oc.census(state, lay)
        print(f"\n[optim cases] {name}: {n} elements after {oc.STEPS} steps, (denormal, inf, NaN) entries: weights {c['p']}, "
              f"exp_avg {c['m']}, exp_avg_sq {c['v']}")
        assert state["steps"] == oc.STEPS and not any(r["skipped"] for r in recs)
        if name == "tiny":
            assert c["v"][0] >= 0.05 * n and c["p"][2] == 0, c                     # denormal second moments; no NaN weight at eps 1e-8
            assert c["v"][0] >= 0.075 * n                                         # ... with room to spare
        elif name == "huge":
            assert c["v"][1] >= 0.5 * n and c["p"][2] == 0, c                      # second moments at inf; no NaN weight
            assert c["v"][1] >= 0.75 * n and c["m"][1] == 0 and np.isfinite(lay.packed(state["p"])).all()
        elif name == "decay":
            moved = lay.packed(weights[1]) != lay.packed(weights[0])
            assert moved.sum() >= 0.85 * n
            for k in range(2, oc.STEPS + 1):                                       # steps 2 and later: zero gradients, decaying moments
                assert (lay.packed(weights[k])[moved] != lay.packed(weights[k - 1])[moved]).all(), k
            assert (lay.packed(weights[-1])[~moved] == lay.packed(weights[0])[~moved]).all()
        else:
            assert c["p"][0] == c["m"][0] == c["v"][0] == 0, c                     # no denormal
            g = oc.schedule(name, lay)
            live = (g != 0).cumsum(axis=0) > 0                                     # the element has had a gradient by that step
            assert ((g[1:] == 0) & live[:-1])[:, lay.used].any(axis=0).sum() >= 0.5 * n      # zero at some step while its moments are not
            assert (g[:, :oc.ALWAYS_ZERO] == 0).all() and (lay.packed(state["p"])[:oc.ALWAYS_ZERO] == lay.packed(weights[0])[:oc.ALWAYS_ZERO]).all()
            mag = np.abs(g[g != 0])
            assert mag.min() < 2e-6 and mag.max() > 5
    # spike: mixed, and two non-finite elements at one step -- one in the 16-byte groups, one in the scalar tail
    g, base = oc.schedule("spike", lay), oc.schedule("mixed", lay)
    where_inf, where_nan = oc.spike_places(lay)
    bad = ~np.isfinite(g)
    assert bad.sum() == 2 and np.isposinf(g[oc.SPIKE_STEP, where_inf]) and np.isnan(g[oc.SPIKE_STEP, where_nan])
    assert np.array_equal(g[~bad], base[~bad]) and where_nan >= lay.count // 4 * 4 and where_inf < lay.count // 4 * 4 and lay.used[where_inf]


def test_the_drive_applies_the_skip_rule():
    lay = oc.Layout(oc.OD3)
    rows = oc.rank_rows("spike", lay, oc.SPIKE_STEP + 1, 1)[oc.SPIKE_STEP]
    for kw, skipped in ((dict(max_grad_norm=1.0), True), (dict(want_norm=True), True), (dict(), False), (dict(max_grad_norm=float("inf")), False)):
        state = oc.start_state(lay)
        before = {k: state[k] for k in ("p", "m", "v")}
        rec = oc.drive_restated(state, rows, oc.tails_of(1, 1, 0), 1, LR, **kw)
        assert rec["skipped"] == skipped, kw
        if skipped:
            assert all(state[k] is before[k] for k in before) and (state["steps"], state["skipped"]) == (0, 1) and np.isnan(rec["loss"])
        else:
            c = oc.census(state, lay)
            print(f"\n[optim cases] spike without a requested norm {kw}: (denormal, inf, NaN) entries: weights {c['p']}, exp_avg {c['m']}, exp_avg_sq {c['v']}")
            assert (state["steps"], state["skipped"]) == (1, 0) and c["p"][1:] == (0, 2) and c["m"][1:] == (1, 1) and c["v"][1:] == (1, 1)
            assert np.isnan(rec["grad_norm"]) and rec["scale"] == 1.0
    state = oc.start_state(lay)                                    # a bad sample, a wrong sample count, replicas out of step
    for tails, total in (([(1, 1, 0.5, 0)], 1), ([(1, 0, 0.5, 0)], 2), ([(1, 0, 0.5, 0), (1, 0, 0.5, 1)], 2)):
        good = oc.rank_rows("mixed", lay, 1, len(tails))[0]
        assert oc.drive_restated(state, good, tails, total, LR)["skipped"]
    assert (state["steps"], state["skipped"]) == (0, 3)


# ---------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("wrong,name,world", [("m_once", "mixed", 1), ("v_order", "mixed", 1), ("flush", "tiny", 1), ("reversed", "mixed", 3)])
def test_a_wrong_treatment_shows_in_the_bits(wrong, name, world):
    lay = oc.Layout(oc.OD3)
    n = int(lay.used.sum())
    right, _, _ = _run(name, lay, world=world, samples=world)
    other, _, _ = _run(name, lay, world=world, samples=world, wrong=wrong)
    diff = {k: oc.words_differing(lay.packed(right[k]), lay.packed(other[k])) for k in ("p", "m", "v")}
    print(f"\n[optim cases] {wrong} on {name}: words differing of {n}: weights {diff['p']}, exp_avg {diff['m']}, exp_avg_sq {diff['v']}")
    assert max(diff.values()) >= 0.01 * n, diff


def test_the_variant_without_a_wrong_treatment_is_the_restatement():
    lay = oc.Layout(oc.OD3)
    g = oc.schedule("mixed", lay, 3)
    a, b = oc.start_state(lay), oc.start_state(lay)
    inner = {"m": [b["m"]], "v": [b["v"]], "b1p": 1.0, "b2p": 1.0, "steps": 0}
    p = [b["p"]]
    for k in range(3):
        oc.adam_variant(a["p"], g[k], a, LR, (0.9, 0.999), 1e-8)
        p = sc.adam_restated(p, [g[k]], inner, LR)
    assert oc.words_differing(a["p"], p[0]) == 0 and oc.words_differing(a["m"], inner["m"][0]) == 0 and oc.words_differing(a["v"], inner["v"][0]) == 0
    assert (a["b1p"], a["b2p"], a["steps"]) == (inner["b1p"], inner["b2p"], 3)


# ---------------------------------------------------------------------------------------------- against float64 torch
@pytest.mark.parametrize("name", ["mixed", "decay"])
def test_restated_drive_against_float64_torch(name):
    lay = oc.Layout(oc.OD3)
    steps = 20
    g = oc.schedule(name, lay, steps)
    p0 = oc.start_weights(lay)

    def torch_run(dtype):
        p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
        opt = torch.optim.Adam([p], lr=LR)
        for row in g:
            p.grad = torch.tensor(row, dtype=dtype)
            opt.step()
        s = opt.state[p]
        return [a.detach().numpy().astype(np.float64) for a in (p, s["exp_avg"], s["exp_avg_sq"])]

    ref64, ref32 = torch_run(torch.float64), torch_run(torch.float32)
    state = oc.start_state(lay)
    for k in range(steps):
        assert not oc.drive_restated(state, g[k:k + 1], oc.tails_of(1, 1, k), 1, LR)["skipped"]
    assert state["steps"] == steps
    for what, a, r64, r32 in zip(("weights", "exp_avg", "exp_avg_sq"), (state["p"], state["m"], state["v"]), ref64, ref32):
        scale = np.abs(r64).max()
        err, e32 = np.abs(a.astype(np.float64) - r64).max() / scale, np.abs(r32 - r64).max() / scale
        print(f"\n[optim cases] {name}, {what}: err {err:.3e}, float32 torch {e32:.3e}, ratio {err / e32:.2f}")
        assert e32 > 0 and err <= 4.0 * e32, (what, err, e32)


# ---------------------------------------------------------------------------------------------- the beta powers
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.99), (0.5, 0.5), (0.0, 0.0)])
def test_running_powers_stop_at_their_fixed_point(betas):
    for steps in (0, 1, 5, 1000, 737_741, 2_000_000):
        plain, fixed = oc.running_powers(*betas, steps), oc.running_powers_fixed(*betas, steps)
        assert np.array_equal(np.array(plain).view(np.uint64), np.array(fixed).view(np.uint64)), (betas, steps, plain, fixed)
    end = oc.running_powers_fixed(*betas, 1 << 40)                # the fixed point itself: reached long before
    assert end == oc.running_powers(*betas, 2_000_000) and all(p * b == p for p, b in zip(end, betas))
    if betas[0] > 0.5:
        assert end[0] > 0 and end[1] > 0 and end[0] < 1e-300 and 1.0 - end[0] == 1.0, end
    else:
        assert end == (0.0, 0.0)
    if betas == (0.9, 0.999):
        assert end == (2.47e-323, 2.465e-321) and oc.running_powers(*betas, 737_741) == end != oc.running_powers(*betas, 737_740)
