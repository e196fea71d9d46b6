"""CPU: the references of tests/rollout_grad_cases.py.  The float64 restatements of the rigid transform's transpose, of the torch
interpolate_trajectory and of the velocity / acceleration terms agree with central finite differences and with the values of the
numpy functions in gnn_manip_amd/planner.py; the reverse sweep over grad_cases.step equals plain autograd through the unrolled
chain; the rollout cases are in the regime the GPU tests need.

Finite differences: float64 central differences on smooth functions of magnitude <= 1 with step 1e-6 carry a truncation error of
about h^2 = 1e-12 and a rounding error of about 2^-52 / h = 2e-10 of the function's magnitude: the bound is 1e-7 of the largest
gradient entry (the clip's kinks are kept 1e-3 away from every sample)."""
import types

import numpy as np
import pytest
import torch

import grad_cases as gc
import rollout_grad_cases as rc

F64 = torch.float64


def _fd(f, x, h=1e-6):
    g = np.zeros(x.numel())
    flat = x.detach().flatten()
    for c in range(x.numel()):
        xp, xm = flat.clone(), flat.clone()
        xp[c] += h
        xm[c] -= h
        g[c] = (float(f(xp.view_as(x))) - float(f(xm.view_as(x)))) / (2 * h)
    return g.reshape(tuple(x.shape))


def _grad(f, x):
    x = x.clone().requires_grad_(True)
    return torch.autograd.grad(f(x), x)[0].numpy()


@pytest.mark.parametrize("nr", [0, 1, 5, 65])
def test_rigid_transform_transpose_is_the_gradient(nr):
    rng = np.random.default_rng(nr)
    init = (0.4 + 0.2 * rng.random((nr, 3))).astype(np.float32)
    rot = rng.uniform(2.5, 3.5, 3)
    cst = torch.tensor(np.stack((np.cos(rot), np.sin(rot), 0.5 + 1e-3 * rng.standard_normal(3)), axis=1), dtype=F64)
    w = rng.standard_normal((3, nr, 3))
    f = lambda c: (rc.rigid_transform(gc.t64(init), c, rc.TY_INIT) * gc.t64(w)).sum()
    d, a = rc.rigid_transform_transpose(init, rc.TY_INIT, w)
    g = _grad(f, cst)
    assert np.abs(d - g).max() <= 1e-12 * max(a.max(), 1.0) if nr else not d.any() and not g.any()
    assert np.abs(_fd(f, cst) - g).max() <= 1e-7 * max(np.abs(g).max(), 1e-30) if nr else True
    assert (a >= np.abs(d) - 1e-15).all()


def test_rigid_transform_restatement_has_the_oracles_values():
    """Against oracle/epd_oracle.rigid_body_trajectory (float32 like the device): a pose is three float32 roundings of values <= 1."""
    from oracle import epd_oracle as orc
    rng = np.random.default_rng(2)
    init = (0.4 + 0.2 * rng.random((40, 3))).astype(np.float32)
    rot, ty = rng.uniform(2.5, 3.5, 4), 1e-3 * rng.standard_normal(4)
    got = rc.poses(gc.t64(rot), gc.t64(ty), rc.TY_INIT, gc.t64(init)).numpy()
    ref = orc.rigid_body_trajectory(rot, ty, 4, list(rc.TY_INIT), init)
    assert np.abs(got - ref).max() <= 8 * 2.0 ** -24


X_CASES = {"inside": [0.4, -0.7, 0.2, 0.3, -0.5, 0.1], "rotation clipped": [0.4, 2.5, -0.2, 0.3, -0.5, 0.1],
           "translation clipped": [0.4, -0.7, 0.2, 0.3, -3.0, 0.1]}


@pytest.mark.parametrize("what", list(X_CASES))
def test_torch_interpolation_is_numpys_and_differentiates(what):
    """max_rot = 1, max_ty = 1e-3, scale_ty = 1e-3: an increment beyond a limit is clipped -- numpy's value, a zero gradient."""
    from gnn_manip_amd.planner import interpolate_trajectory, interpolate_trajectory_torch
    args = (3, np.deg2rad(180.0), 1.0, 1e-3, 1.0, 1e-3)
    x = np.asarray(X_CASES[what])
    rot, ty = interpolate_trajectory_torch(gc.t64(x), *args)
    ref_rot, ref_ty = interpolate_trajectory(x, *args)
    assert np.abs(rot.numpy() - ref_rot).max() <= 4 * 2.0 ** -52 * 4 and np.abs(ty.numpy() - ref_ty).max() <= 4 * 2.0 ** -52 * 4e-3
    w = gc.t64(np.random.default_rng(1).standard_normal((2, 4)))
    f = lambda v: (torch.stack(interpolate_trajectory_torch(v, *args)) * w).sum()
    g = _grad(f, gc.t64(x))
    assert np.abs(_fd(f, gc.t64(x)) - g).max() <= 1e-7 * np.abs(g).max()
    clipped = np.array([abs(v) > 1.0 for v in x[:3]] + [abs(v) > 1.0 for v in x[3:]])
    assert np.array_equal(g == 0.0, clipped), (g, clipped)


def test_velocity_and_acceleration_terms_are_numpys_and_differentiate():
    from gnn_manip_amd.planner import TrajectoryCMAsolver as S
    rng = np.random.default_rng(3)
    actions = np.stack((3.1 + 0.01 * rng.standard_normal(6), 1e-4 * rng.standard_normal(6)), axis=1)
    limits = types.SimpleNamespace(max_rot=0.03, max_ty=6.67e-4)
    vel, acc = S.compute_vel_acc(actions)
    v, a = rc.velocity_acceleration_terms(gc.t64(actions), limits.max_rot, limits.max_ty)
    assert abs(float(v) - S.compute_vel_loss(limits, vel)) <= 1e-14 * float(v)
    assert abs(float(a) - S.compute_acc_loss(limits, acc)) <= 1e-14 * float(a)
    for k in (0, 1):
        f = lambda x: rc.velocity_acceleration_terms(x, limits.max_rot, limits.max_ty)[k]
        g = _grad(f, gc.t64(actions))
        assert np.abs(_fd(f, gc.t64(actions), h=1e-8) - g).max() <= 1e-6 * np.abs(g).max()


@pytest.mark.parametrize("with_trajectory", [True, False])
def test_reverse_sweep_is_autograd_through_the_unrolled_chain(with_trajectory):
    obs = gc.step_state("step_a")
    tr = rc.trajectory("step_a") if with_trajectory else None
    eis = rc.oracle_edge_lists("step_a", with_trajectory)
    assert len(eis) == rc.T == 4
    end = rc.weighted_sum()
    final, g_obs, g_tr = rc.reference(obs, tr, eis, F64, end)
    final2, s_obs, s_tr = rc.reverse_sweep(obs, tr, eis, end)
    assert np.array_equal(final, final2)
    scale = np.abs(g_obs).max()
    assert np.abs(s_obs - g_obs).max() <= 1e-12 * scale
    if with_trajectory:
        assert np.abs(g_tr).max(axis=(1, 2)).min() > 0                 # every step's pose matters
        assert np.abs(s_tr - g_tr).max() <= 1e-12 * np.abs(g_tr).max()


@pytest.mark.parametrize("name,with_trajectory", [("step_a", True), ("step_a", False), ("step_b", True)])
def test_rollout_cases_are_in_their_regime(name, with_trajectory):
    """What the GPU tests' yardstick needs of a case: plain float32 PyTorch on the same edge lists is itself within GRAD_TOL of
    float64 in most gradient tensors (no ReLU unit sits on the rounding edge there, so the bound the device is held to is
    GRAD_TOL and not a multiple of a large float32 error); the rollout stays bounded; rigid and fluid rows both take part."""
    obs = gc.step_state(name)
    tr = rc.trajectory(name) if with_trajectory else None
    eis = rc.oracle_edge_lists(name, with_trajectory)
    end = rc.weighted_sum()
    final, g_obs, g_tr = rc.reference(obs, tr, eis, F64, end)
    _, h_obs, h_tr = rc.reference(obs, tr, eis, torch.float32, end)
    c, u = slice(rc.L0.cart, rc.L0.cart + 3), slice(rc.L0.ctrl, rc.L0.ctrl + 3)
    tensors = [(g_obs[:, :, c], h_obs[:, :, c]), (g_obs[:, :, u], h_obs[:, :, u])]
    if with_trajectory:
        tensors += [(g_tr[t], h_tr[t]) for t in range(rc.T)]
    errs = [np.abs(h - g).max() / np.abs(g).max() for g, h in tensors]
    print(name, with_trajectory, ["%.2e" % e for e in errs])
    assert sum(e <= rc.GRAD_TOL for e in errs) > len(errs) / 2, errs
    assert np.isfinite(final).all() and np.abs(final[-1][:, c] - obs[-1][:, c]).max() < 0.05
    assert all(ei.shape[1] > obs.shape[1] for ei in eis)          # more than the self edges at every step
    assert len(gc.rigid_rows(obs, rc.L0)) > 0
