"""Batched trajectory gradients and their optimiser on the MI355X: TrajectoryCMAsolver.population_loss_and_grad (every row bit-equal
to loss_and_grad's, whatever the block it was evaluated in), refine (projected Adam: decreases the objective, reports
cma_objective's values) and optimize_trajectory(refine=...).  The scene is the step scene of tests/test_gpu_rollout_grad.py
(N = 400, hidden 128, 2 message-passing steps, 4 rollout steps, 2 trajectory points).  The update rule itself is held on the CPU
(tests/test_plan_refine_cases.py).  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from gpu_support import dev, step_solver as _solver

pytestmark = pytest.mark.gpu

# The step size of test_refine_decreases_the_objective, in half-widths of the box per iteration (refine's unit): refine's default,
# chosen among 0.003 / 0.01 / 0.03 / 0.1 on the device.  Measured objective sequences, 8 iterations from the sample trajectory
# (start 0; the sequences from 1.1 x the sample trajectory run parallel to these, 0.0044 higher at iterate 0):
#   lr 0.003: 1.921889357 1.921872344 1.921307378 1.920686016 1.920041030 1.919384017 1.918719761 1.918050745 1.917378957
#   lr 0.01:  1.921889357 1.921864022 1.920001728 1.917957405 1.915847544 1.913712105 1.911572204 1.909440070 1.907325684
#   lr 0.03:  1.921889357 1.922107939 1.916791092 1.911120858 1.905616372 1.900648023 1.896533581 1.893224252 1.890100761
#   lr 0.1:   1.921889357 1.927064464 1.917801339 1.909870341 1.896190776 1.884125402 1.892256731 1.897467198 1.897576257
# 0.003 and 0.01 decrease at every iterate; 0.03 and 0.1 rise at the first one (Adam's first step is lr in EVERY variable, whatever
# the size of its gradient entry) and 0.1 turns around after five.  All four end below the start.
LR = 0.01


def _x0(s):
    return np.concatenate((s.sample_traj[:, 0], s.sample_traj[:, 1]))


@pytest.mark.parametrize("sweep", ["autograd", "library"])
def test_population_of_one_is_loss_and_grad(dev, sweep):
    s = _solver(dev)[0]
    x = 1.1 * _x0(s)
    loss, grad = s.loss_and_grad(x, sweep=sweep)
    losses, grads = s.population_loss_and_grad([x], sweep=sweep)
    print(f"\n[plan refine] {sweep}: loss_and_grad {loss!r} {grad}, population of one {losses[0]!r} {grads[0]}")
    assert losses.dtype == np.float64 and grads.dtype == np.float64 and losses.shape == (1,) and grads.shape == (1, len(x))
    assert losses[0] == loss and np.array_equal(grads[0], grad)
    assert np.count_nonzero(grad) == len(x)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("sweep", ["autograd", "library"])
def test_ragged_blocks_are_the_single_calls(dev, sweep, frozen):
    """Three candidates at candidates_per_gpu = 2: a block of two on _engine(2) and a block of one.  One of them has a rotation
    increment beyond the limit: its row is the clipped single call's, with a gradient of exactly 0 in that variable."""
    s = _solver(dev)[0]
    s.model.requires_grad_(not frozen)
    x0 = _x0(s)
    clipped = 1.1 * x0
    clipped[1] = -1.5 * s.max_rot
    X = [1.1 * x0, clipped, 0.9 * x0]
    single = [s.loss_and_grad(x, sweep=sweep) for x in X]
    s.candidates_per_gpu = 2
    losses, grads = s.population_loss_and_grad(X, sweep=sweep)
    assert sorted(s._engines) == [1, 2]
    assert losses.shape == (3,) and grads.shape == (3, len(x0))
    for p, (loss, grad) in enumerate(single):
        print(f"\n[plan refine] {sweep} candidate {p}: single {loss!r} {grad}, in its block {losses[p]!r} {grads[p]}")
        assert losses[p] == loss and np.array_equal(grads[p], grad), p
    assert grads[1, 1] == 0.0 and np.count_nonzero(grads) == grads.size - 1
    assert all(q.requires_grad != frozen and q.grad is None for q in s.model.parameters())


def test_refine_decreases_the_objective(dev):
    s = _solver(dev)[0]
    s.candidates_per_gpu = 2
    x0 = _x0(s)
    X0 = np.stack((x0, 1.1 * x0))
    x_best, f_best, info = s.refine(X0, iters=8, lr=LR)
    assert x_best.shape == X0.shape and f_best.shape == (2,) and info["f"].shape == (2, 9)
    assert (np.abs(x_best) <= s.box_half_widths()).all()
    values = [s.cma_objective(x) for x in x_best]
    for p in range(2):
        print(f"\n[plan refine] start {p}: objective sequence " + " ".join(f"{v:.9e}" for v in info["f"][p]))
        print(f"[plan refine] start {p}: f_best {f_best[p]:.9e}, cma_objective(x_best) {values[p]:.9e}")
    for p in range(2):
        assert abs(f_best[p] - values[p]) <= 1e-5 * abs(values[p])  # test_loss_and_grad's bar between the two forwards
        assert f_best[p] == info["f"][p].min() and f_best[p] < info["f"][p, 0]
    assert info["f"][0, 0] == s.loss_and_grad(x0, sweep="library")[0]   # iterate 0 is the start
    again = s.refine(X0, iters=8, lr=LR)
    assert np.array_equal(again[0], x_best) and np.array_equal(again[1], f_best) and np.array_equal(again[2]["f"], info["f"])
    x_none, f_none, info_none = s.refine(X0, iters=0)
    assert np.array_equal(x_none, X0) and np.array_equal(f_none, info["f"][:, 0]) and info_none["f"].shape == (2, 1)


def test_optimize_trajectory_with_refinement(dev):
    def solver():
        s = _solver(dev)[0]
        s.cma_options["maxiter"], s.cma_options["popsize"] = 1, 4
        s.candidates_per_gpu = 2
        return s
    desired = solver().desired_pos
    x_plain, es_plain = solver().optimize_trajectory(desired)
    x_none, es_none = solver().optimize_trajectory(desired, refine=None)
    assert np.array_equal(x_plain, x_none) and es_plain.result.fbest == es_none.result.fbest and not hasattr(es_none, "refined")
    s = solver()
    x, es = s.optimize_trajectory(desired, refine=dict(iters=3, lr=LR, sweep="library"))
    value = s.cma_objective(x)
    print(f"\n[plan refine] optimize_trajectory: fbest {es.result.fbest:.9e}, refined " + " ".join(f"{v:.9e}" for v in es.refined["f"])
          + f", returned point {value:.9e}")
    assert es.result.fbest == es_plain.result.fbest and value <= es.result.fbest
    assert es.refined["x"].shape == (2, len(x)) and es.refined["f"].shape == (2,) and es.refined["info"]["f"].shape == (2, 4)
    assert np.array_equal(es.refined["f"], es.refined["info"]["f"].min(axis=1))


def test_interpolated_solver_has_no_population_gradient(dev):
    from gnn_manip_amd.planner import InterpolatedCMAsolver
    s = _solver(dev, InterpolatedCMAsolver)[0]
    with pytest.raises(NotImplementedError):
        s.population_loss_and_grad([np.zeros(4)])
    with pytest.raises(NotImplementedError):
        s.refine([np.zeros(4)])
