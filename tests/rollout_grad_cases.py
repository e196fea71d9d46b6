"""Cases and float64 references of the differentiable rollout and of the map from a planner's search vector to the cup's poses
(tests/test_rollout_grad_cases.py checks them on the CPU, tests/test_gpu_rollout_grad.py holds the HIP paths to them).

The rollout is tests/grad_cases.step unrolled on given edge lists (the radius graph is a constant of each step).  `reverse_sweep`
restates the algorithm of RolloutEngine.differentiable_rollout over that step -- forward without a graph keeping each step's
pre-step window, backward re-running one step at a time -- so that the CPU test can hold it to plain autograd through the unrolled
chain: that pins the algorithm, the GPU tests pin the kernels.  The rigid transform, its transpose and the planner's velocity /
acceleration terms are restated here in float64; the CPU test holds each to central finite differences and to the numpy functions
of gnn_manip_amd/planner.py."""
import functools

import numpy as np
import torch

from oracle import epd_oracle as orc
import grad_cases as gc
from sinkhorn_cases import sinkhorn_grad_ref
from yardstick import GRAD_TOL  # noqa: F401  (the CPU regime test reads it from here)

L0 = gc.L0
T = 4
MODEL_SEED = 841
TY_INIT = (0.5, 0.5, 0.4)
F64 = torch.float64


# ------------------------------------------------------------------------------------------ rigid transform (traj_utils.py:167-194)
def rigid_transform(init, cst, ty_init):
    """[T, Nr, 3] poses from init [Nr, 3] and the per-step rows cst [T, 3] = (cos, sin, ty_init[1] + translation): the rotation
    about X in the cup frame with the y / z axis swap, in the dtype of `cst`.  ty_init enters as the float32 numbers the device
    is handed."""
    tx, ty, tz = (float(np.float32(v)) for v in ty_init)
    i0, i1, i2 = tx - init[:, 0], ty - init[:, 2], tz - init[:, 1]
    c, s, typ = cst[:, 0:1], cst[:, 1:2], cst[:, 2:3]
    p0 = (i0 + tx)[None].expand(cst.shape[0], -1)
    p1 = c * i1[None] - s * i2[None] + typ
    p2 = c * i2[None] + s * i1[None] + tz
    return torch.stack((p0, p2, p1), dim=2)


def rigid_transform_transpose(init, ty_init, g):
    """The transpose of `rigid_transform` w.r.t. cst, written out: (d_cst [T, 3], abs [T, 3]) in numpy float64, `abs` the sum of
    the absolute values of the terms of each entry (what a float32 summation's error is proportional to).  init and ty_init are
    taken as the float32 numbers the device holds."""
    init = np.asarray(init, np.float32).astype(np.float64)
    g = np.asarray(g, np.float64)
    ty, tz = float(np.float32(ty_init[1])), float(np.float32(ty_init[2]))
    i1, i2 = ty - init[:, 2], tz - init[:, 1]
    g1, g2 = g[:, :, 1], g[:, :, 2]
    terms = ((g2 * i1, g1 * i2), (-g2 * i2, g1 * i1), (g2,))
    d = np.stack([sum(t).sum(axis=1) for t in terms], axis=1)
    a = np.stack([sum(np.abs(x) for x in t).sum(axis=1) for t in terms], axis=1)
    return d, a


def poses(rot, ty, ty_init, init):
    """rot, ty [T] float64 tensors -> [T, Nr, 3] float64 poses: planner.rigid_body_trajectory in float64 throughout."""
    return rigid_transform(init, torch.stack((torch.cos(rot), torch.sin(rot), float(ty_init[1]) + ty), dim=1), ty_init)


def velocity_acceleration_terms(actions, max_rot, max_ty):
    """traj_utils.py:161-165,261-273 for a [T, 2] float64 tensor of (rotation, translation) per step: the Frobenius norms of the
    first and second differences, each column over its limit."""
    lim = torch.tensor([max_rot, max_ty], dtype=actions.dtype)
    vel = actions[1:] - actions[:-1]
    acc = actions[2:] - 2 * actions[1:-1] + actions[:-2]
    return torch.linalg.norm(vel / lim), torch.linalg.norm(acc / lim)


# ------------------------------------------------------------------------------------------ the rollout on given edge lists
@functools.lru_cache(maxsize=None)
def params():
    return orc.init_params(*gc.STEP_DIMS, MODEL_SEED)


def p_of(dtype):
    return {k: torch.tensor(v, dtype=dtype) for k, v in params().items()}


@functools.lru_cache(maxsize=None)
def trajectory(name, seed=3, steps=T):
    """[steps, n_rigid, 3] float32 scripted poses for step_state(name): the rigid rows moved a little further every step along
    seeded directions (grad_cases.rigid_target)."""
    obs = gc.step_state(name)
    tr = np.stack([gc.rigid_target(obs, L0, seed + t, step_size=3e-4 * (t + 1)) for t in range(steps)])
    tr.setflags(write=False)
    return tr


def unrolled(p, obs, targets, edge_lists):
    """grad_cases.step applied len(edge_lists) times; targets: a list of [n_rigid, 3] tensors, or None."""
    rows = torch.tensor(gc.rigid_rows(obs.detach().numpy(), L0))
    cur = obs
    for t, ei in enumerate(edge_lists):
        cur, _ = gc.step(p, cur, L0, rows, None if targets is None else targets[t], torch.as_tensor(ei), gc.STEP_DIMS[4],
                         gc.STEP_DIMS[5])
    return cur


@functools.lru_cache(maxsize=None)
def oracle_edge_lists(name, with_trajectory=True, steps=T):
    """The oracle's radius graph of every step of the float64 rollout of step_state(name) (CPU tests; the GPU tests use the lists
    the device returns)."""
    p = p_of(F64)
    obs = gc.t64(gc.step_state(name))
    rows = torch.tensor(gc.rigid_rows(obs.numpy(), L0))
    tr = trajectory(name) if with_trajectory else None
    out = []
    with torch.no_grad():
        for t in range(steps):
            s, r = orc.get_connectivity(obs[-1][:, L0.cart:L0.cart + 3].numpy().astype(np.float32), gc.R, 20)
            ei = np.ascontiguousarray(np.stack((s, r)).astype(np.int64))
            out.append(ei)
            obs, _ = gc.step(p, obs, L0, rows, None if tr is None else gc.t64(tr[t]), torch.tensor(ei), gc.STEP_DIMS[4], gc.STEP_DIMS[5])
    return tuple(out)


def reference(obs_np, traj_np, edge_lists, dtype, end_grad):
    """Plain autograd through the unrolled chain: (final state, d obs, d trajectory [T, n_rigid, 3] or None) as numpy, for the loss
    whose gradient w.r.t. the final state is end_grad(final state as numpy)."""
    obs = gc.t64(obs_np, True, dtype)
    tg = None if traj_np is None else [gc.t64(t, True, dtype) for t in traj_np]
    final = unrolled(p_of(dtype), obs, tg, edge_lists)
    final.backward(gradient=torch.tensor(end_grad(final.detach().numpy()), dtype=dtype))
    return final.detach().numpy(), obs.grad.numpy(), None if tg is None else np.stack([t.grad.numpy() for t in tg])


def reverse_sweep(obs_np, traj_np, edge_lists, end_grad, dtype=F64):
    """RolloutEngine.differentiable_rollout's algorithm over grad_cases.step: the forward runs without a graph and keeps every
    step's pre-step window; the backward walks the steps in reverse, re-runs step t on its window with grad enabled, feeds it the
    gradient w.r.t. the window after it and takes the gradient w.r.t. the window before it and step t's pose."""
    p = p_of(dtype)
    rows = torch.tensor(gc.rigid_rows(obs_np, L0))
    cur = gc.t64(obs_np, dtype=dtype)
    windows = []
    with torch.no_grad():
        for t, ei in enumerate(edge_lists):
            windows.append(cur)
            cur, _ = gc.step(p, cur, L0, rows, None if traj_np is None else gc.t64(traj_np[t], dtype=dtype), torch.as_tensor(ei),
                             gc.STEP_DIMS[4], gc.STEP_DIMS[5])
    final = cur.numpy()
    d_window = torch.tensor(end_grad(final), dtype=dtype)
    d_traj = None if traj_np is None else np.zeros(np.shape(traj_np))
    for t in range(len(edge_lists) - 1, -1, -1):
        w = windows[t].clone().requires_grad_(True)
        pose = None if traj_np is None else gc.t64(traj_np[t], True, dtype)
        nxt, _ = gc.step(p, w, L0, rows, pose, torch.as_tensor(edge_lists[t]), gc.STEP_DIMS[4], gc.STEP_DIMS[5])
        grads = torch.autograd.grad(nxt, [w] if pose is None else [w, pose], grad_outputs=d_window)
        d_window = grads[0]
        if pose is not None:
            d_traj[t] = grads[1].numpy()
    return final, d_window.numpy(), d_traj


def weighted_sum(seed=6):
    """end_grad of the loss (final * w).sum() with seeded float32 w."""
    w = gc.weights(gc.step_state("step_a").shape, seed)
    return lambda final: w


def desired_cloud(obs_np):
    """The fluid rows and their desired cloud for a SamplesLoss behind the rollout: the fluid moved by (0.03, -0.02, 0.05) with a
    seeded per-particle offset, as in tests/test_gpu_input_grads.py (a loss of about 1.9e-3, which float32 carries to 1e-5)."""
    fluid = np.nonzero(obs_np[-1][:, L0.mat] == 0)[0]
    shift = np.array([0.03, -0.02, 0.05], np.float32)
    cloud = (obs_np[-1][fluid][:, L0.cart:L0.cart + 3] + shift + np.float32(0.004) * gc.weights((len(fluid), 3), 8)).astype(np.float32)
    return fluid, cloud


# ------------------------------------------------------------------------------------------ the planner's objective
def objective_reference(s, x, obs_np, init, fluid, cloud, eis, dtype, forward=None, end_grad=None):
    """The objective assembled from the checked pieces, differentiated w.r.t. x (float64 leaf): torch interpolation and float64
    rigid transform -> the restatement rollout in `dtype` on the device's edge lists -> sinkhorn_grad_ref at its end cloud -> the
    float64 penalties.  forward / end_grad: flip_allowance's model and the first-order stand-in of the loss behind the end state.
    Returns (value, gradient), or the scalar whose gradient the allowance needs."""
    from gnn_manip_amd.planner import interpolate_trajectory_torch
    xt = x if isinstance(x, torch.Tensor) else gc.t64(x, True)
    rot, ty = interpolate_trajectory_torch(xt, s.sample_traj.shape[0], float(s.rx_init), s.scale_rot, s.scale_ty, float(s.max_rot), s.max_ty)
    tr = poses(rot[:4], ty[:4], s.ty_init, gc.t64(init)).to(dtype)
    p = p_of(dtype)
    rows = torch.tensor(gc.rigid_rows(obs_np, L0))
    cur = gc.t64(obs_np, dtype=dtype)
    for t, ei in enumerate(eis):
        kw = {} if forward is None else dict(forward=forward)
        cur, _ = gc.step(p, cur, L0, rows, tr[t], torch.tensor(ei), gc.STEP_DIMS[4], gc.STEP_DIMS[5], **kw)
    c = slice(L0.cart, L0.cart + 3)
    if end_grad is not None:
        return (cur[-1][fluid][:, c] * gc.t64(end_grad)).sum()
    end = cur[-1][fluid][:, c]
    w, dx, _ = sinkhorn_grad_ref(end.detach().numpy(), cloud)
    v, a = velocity_acceleration_terms(torch.stack((rot[:4], ty[:4]), dim=1), float(s.max_rot), s.max_ty)
    smooth = s.beta * (end.double() * gc.t64(dx)).sum() + s.alpha * v + s.gamma * a        # first order in the end cloud: its gradient is the loss's
    smooth.backward()
    return s.beta * w + s.alpha * float(v.detach()) + s.gamma * float(a.detach()), xt.grad.numpy().copy(), s.beta * dx
