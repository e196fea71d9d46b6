"""CPU: the update rule of the trajectory refinement (gnn_manip_amd.planner.projected_adam, refine_starts) driven by stub
objectives -- tests/plan_refine_cases.py.  The library's loop against the numpy restatement of Adam + clamp: both are float64
evaluations of the same formulas, so the bar is 1e-12 relative, the project's bar for its float64 restatements."""
import socket

import numpy as np
import pytest
import torch.multiprocessing as mp

import plan_refine_cases as pc
from gnn_manip_amd.planner import projected_adam, refine_starts


@pytest.mark.parametrize("lr", [0.01, 0.1])
def test_projected_adam_is_adam_and_the_clamp(lr):
    iters = 40
    X0 = pc.starts(3)
    x_best, f_best, info = projected_adam(pc.quadratic, X0, pc.HALF_WIDTHS, iters=iters, lr=lr)
    assert info["x"].shape == (3, iters + 1, pc.DIM) and info["f"].shape == (3, iters + 1)
    for p in range(3):
        want = pc.adam_reference(lambda x: pc.quadratic(x[None])[1][0], X0[p], pc.HALF_WIDTHS, iters, lr)
        err = np.abs(info["x"][p] - want).max() / np.abs(want).max()
        print(f"\n[plan refine] lr {lr} start {p}: iterates against the restatement, max err / max |x| {err:.3e}")
        assert np.abs(info["x"][p] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(info["x"][p, 0], X0[p])                                # a start inside the box is iterate 0 itself
        assert np.array_equal(info["f"][p], pc.quadratic(info["x"][p])[0])          # value k belongs to iterate k
    assert (np.abs(info["x"]) <= pc.HALF_WIDTHS).all()                               # every iterate lies inside the box
    if lr == 0.1:   # 40 steps of about 0.1 half-widths each reach the bound from anywhere in the box
        assert (info["x"][:, -1, pc.OUTSIDE] == pc.HALF_WIDTHS[pc.OUTSIDE]).all()    # the outside minimiser: ON the bound, exactly
    assert (f_best <= info["f"][:, 0]).all() and (f_best < info["f"][:, 0]).any()


def test_best_iterate_is_tracked_by_the_full_objective():
    iters = 6
    X0 = pc.starts(3)
    _, _, plain = projected_adam(pc.quadratic, X0, pc.HALF_WIDTHS, iters=iters, lr=0.01)
    assert (np.argmin(plain["f"], axis=1) == iters).all()        # without a penalty the last iterate is the best one of every start
    x_best, f_best, info = projected_adam(pc.PenalisedAt(iters), X0, pc.HALF_WIDTHS, iters=iters, lr=0.01)
    assert np.array_equal(info["f"][:, :iters], plain["f"][:, :iters]) and np.array_equal(info["f"][:, iters], plain["f"][:, iters] + pc.PENALTY)
    assert np.array_equal(f_best, info["f"].min(axis=1))
    assert np.array_equal(x_best, info["x"][:, iters - 1]) and not np.array_equal(x_best, info["x"][:, iters])
    # a penalty in the middle: the iteration goes on through it (the gradient does not see it) and that iterate is not returned
    x_mid, f_mid, info_mid = projected_adam(pc.PenalisedAt(3), X0, pc.HALF_WIDTHS, iters=iters, lr=0.01)
    assert np.array_equal(info_mid["x"], plain["x"]) and np.array_equal(f_mid, info_mid["f"].min(axis=1))
    assert np.array_equal(x_mid, plain["x"][:, iters])


def test_no_iterations_evaluates_and_returns_the_starts():
    X0 = pc.starts(4)
    obj = pc.Counting()
    x_best, f_best, info = projected_adam(obj, X0, pc.HALF_WIDTHS, iters=0)
    assert len(obj.calls) == 1 and np.array_equal(obj.calls[0], X0)
    assert np.array_equal(x_best, X0) and np.array_equal(f_best, pc.quadratic(X0)[0]) and info["f"].shape == (4, 1)


def test_two_calls_return_the_same_bits():
    X0 = pc.starts(3)
    a = projected_adam(pc.quadratic, X0, pc.HALF_WIDTHS, iters=10, lr=0.03)
    b = projected_adam(pc.quadratic, X0.copy(), pc.HALF_WIDTHS, iters=10, lr=0.03)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[2]["f"], b[2]["f"]) and np.array_equal(a[2]["x"], b[2]["x"])
    # starts do not interact: a start refined alone gives the row it gives in the batch
    alone = projected_adam(pc.quadratic, X0[1:2], pc.HALF_WIDTHS, iters=10, lr=0.03)
    assert np.array_equal(alone[0][0], a[0][1]) and np.array_equal(alone[2]["f"][0], a[2]["f"][1])


def test_a_start_outside_the_box_is_moved_onto_it_first():
    X0 = pc.starts(2)
    X0[0, 1] = -3.0 * pc.HALF_WIDTHS[1]
    X0[1, 4] = 1.5 * pc.HALF_WIDTHS[4]
    obj = pc.Counting()
    _, _, info = projected_adam(obj, X0, pc.HALF_WIDTHS, iters=2, lr=0.01)
    clamped = np.clip(X0, -pc.HALF_WIDTHS, pc.HALF_WIDTHS)
    assert clamped[0, 1] == -pc.HALF_WIDTHS[1] and clamped[1, 4] == pc.HALF_WIDTHS[4]
    assert np.array_equal(obj.calls[0], clamped) and np.array_equal(info["x"][:, 0], clamped)
    assert np.array_equal(info["f"][:, 0], pc.quadratic(clamped)[0])
    with pytest.raises(ValueError):
        projected_adam(obj, X0, pc.HALF_WIDTHS[:-1])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_refine_starts_sharded_over_gloo_world2():
    """3 starts over 2 ranks, ragged 2 + 1: every rank receives exactly the single-process result, and its objective saw only its
    own block, once per iterate."""
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=pc.gloo_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    out = sorted([q.get(timeout=120) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    X0 = pc.starts(3)
    x1, f1, info1 = refine_starts(pc.quadratic, X0, pc.HALF_WIDTHS, iters=pc.GLOO_ITERS, lr=pc.GLOO_LR)    # no process group here: one process
    for (rank, x, f, fs, calls), (lo, hi) in zip(out, ((0, 2), (2, 3))):
        assert np.array_equal(x, x1) and np.array_equal(f, f1) and np.array_equal(fs, info1["f"]), rank
        assert len(calls) == pc.GLOO_ITERS + 1 and all(len(c) == hi - lo for c in calls), (rank, calls)
        assert calls[0] == X0[lo:hi, 0].tolist()
