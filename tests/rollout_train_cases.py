"""Cases and float64 references of training through a rollout: a loss with a term on the final state AND on every step's record,
differentiated with respect to the initial window, the trajectory and every parameter of the model
(tests/test_rollout_train_cases.py checks them on the CPU, tests/test_gpu_rollout_train.py holds gm_rollout_step_backward_train,
gm_rollout_backward_train and RolloutEngine.differentiable_rollout(record=, params=) to them).

The scene, model and trajectory are tests/rollout_grad_cases.py's (step_a / step_b, 400 nodes, STEP_DIMS, T = 4); the rollout is
tests/grad_cases.step unrolled on given edge lists.  Record t is the last frame of window t after state_pre's control overwrite
(gm_rollout's record_last[t]).  The loss is (final * w).sum() + sum_t (record[t] * w_t).sum() with seeded float32 weights.

`reference` is plain autograd through the unrolled chain.  `reverse_sweep` restates the library's algorithm: the forward keeps each
step's pre-step window and no graph; the backward re-runs ONE step at a time, takes the gradient with respect to the window after
state_pre, adds the record's gradient to its last frame, and only then applies state_pre's transpose; a step's pose gets
state_post's share plus state_pre's; parameter gradients are accumulated from the last step to the first."""
import functools

import numpy as np
import torch

from oracle import torch_epd
import grad_cases as gc
import rollout_grad_cases as rc

L0 = rc.L0
T = rc.T
F64 = torch.float64
W_FINAL_SEED, W_RECORD_SEED = 6, 9
NUM_LAYERS, M_STEPS = gc.STEP_DIMS[4], gc.STEP_DIMS[5]


@functools.lru_cache(maxsize=None)
def final_weights():
    """[k, N, D] float32: rollout_grad_cases.weighted_sum's."""
    w = gc.weights(gc.step_state("step_a").shape, W_FINAL_SEED)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def record_weights(steps=T, seed=W_RECORD_SEED):
    """[steps, N, D] float32: w_t of the loss's term on record t."""
    w = gc.weights((steps,) + gc.step_state("step_a").shape[1:], seed)
    w.setflags(write=False)
    return w


def _after_pre(p, pre, rows, pose, ei, forward=torch_epd.epd_forward):
    """grad_cases.step from the window state_pre left: the next window."""
    ei = torch.as_tensor(ei)
    nodes = gc.node_features(pre, L0)
    ea = gc.edge_features(pre[-1][:, L0.cart:L0.cart + 3], ei[0], ei[1])
    pred = forward(p, nodes, ea, ei, NUM_LAYERS, M_STEPS)
    return gc.state_post(pre, L0, gc.integrate(pred, pre, L0), rows, pose)


def _step(p, cur, rows, pose, ei, forward=torch_epd.epd_forward):
    """grad_cases.step written out so that the window after state_pre is at hand: (pre, next window)."""
    pre = gc.state_pre(cur, L0, rows, pose)
    return pre, _after_pre(p, pre, rows, pose, ei, forward)


def unrolled(p, obs, targets, edge_lists, forward=torch_epd.epd_forward):
    """(final state [k, N, D], records [T, N, D]) of grad_cases.step applied len(edge_lists) times; targets: a list of
    [n_rigid, 3] tensors, or None."""
    rows = torch.tensor(gc.rigid_rows(obs.detach().numpy(), L0))
    cur, recs = obs, []
    for t, ei in enumerate(edge_lists):
        pre, cur = _step(p, cur, rows, None if targets is None else targets[t], ei, forward)
        recs.append(pre[-1])
    return cur, (torch.stack(recs) if recs else torch.zeros((0,) + tuple(obs.shape[1:]), dtype=obs.dtype))


def loss_of(final, records, w_final, w_records):
    loss = (final * torch.tensor(np.asarray(w_final), dtype=final.dtype)).sum()
    if w_records is not None:
        loss = loss + (records * torch.tensor(np.asarray(w_records), dtype=final.dtype)).sum()
    return loss


def reference(params_np, obs_np, traj_np, edge_lists, dtype, w_final, w_records):
    """Plain autograd through the unrolled chain: (final, records, d obs, d trajectory [T, n_rigid, 3] or None, {name: d parameter})
    as numpy.  w_records None: the loss has no term on the records."""
    p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in params_np.items()}
    obs = gc.t64(obs_np, True, dtype)
    tg = None if traj_np is None else [gc.t64(t, True, dtype) for t in traj_np[:len(edge_lists)]]
    final, records = unrolled(p, obs, tg, edge_lists)
    loss_of(final, records, w_final, w_records).backward()
    return (final.detach().numpy(), records.detach().numpy(), obs.grad.numpy(), None if tg is None else np.stack([t.grad.numpy() for t in tg]),
            {k: v.grad.numpy() for k, v in p.items()})


def reverse_sweep(params_np, obs_np, traj_np, edge_lists, w_final, w_records, dtype=F64, with_params=True):
    """The library's algorithm (gm_rollout_backward_train under RolloutEngine.differentiable_rollout): (final, records, d obs,
    d trajectory or None, {name: d parameter} or None).  The forward takes record t as frame k-2 of the window after step t."""
    p = {k: torch.tensor(v, dtype=dtype) for k, v in params_np.items()}
    rows = torch.tensor(gc.rigid_rows(obs_np, L0))
    steps = len(edge_lists)
    cur = gc.t64(obs_np, dtype=dtype)
    windows, recs = [], []
    with torch.no_grad():
        for t, ei in enumerate(edge_lists):
            windows.append(cur)
            _, cur = _step(p, cur, rows, None if traj_np is None else gc.t64(traj_np[t], dtype=dtype), ei)
            recs.append(cur[-2])
    final = cur.numpy()
    records = torch.stack(recs).numpy() if recs else np.zeros((0,) + obs_np.shape[1:])
    d_window = torch.tensor(np.asarray(w_final), dtype=dtype)
    d_traj = None if traj_np is None else np.zeros(np.shape(traj_np[:steps]))
    d_params = {k: torch.zeros_like(v) for k, v in p.items()} if with_params else None
    for t in range(steps - 1, -1, -1):
        w = windows[t].clone().requires_grad_(True)
        pose = None if traj_np is None else gc.t64(traj_np[t], True, dtype)
        leaves = {k: v.clone().requires_grad_(True) for k, v in p.items()} if with_params else p
        pre0 = gc.state_pre(w, L0, rows, pose)
        pre = pre0.detach().requires_grad_(True)     # the two halves of the step apart: what lies behind state_pre first
        nxt = _after_pre(leaves, pre, rows, pose, edge_lists[t])
        # the gradient w.r.t. the window state_pre left, state_post's share of the pose, the parameters
        wanted = [pre] + ([pose] if pose is not None else []) + (list(leaves.values()) if with_params else [])
        got = list(torch.autograd.grad(nxt, wanted, grad_outputs=d_window))
        g_pre = got.pop(0)
        post_share = got.pop(0) if pose is not None else None
        if w_records is not None:       # the record IS pre's last frame: its gradient joins before state_pre's transpose
            g_pre = torch.cat((g_pre[:-1], (g_pre[-1] + torch.tensor(np.asarray(w_records[t]), dtype=dtype))[None]))
        back = torch.autograd.grad(pre0, [w] + ([pose] if pose is not None else []), grad_outputs=g_pre, allow_unused=True)
        d_window = back[0]
        if pose is not None:
            pre_share = back[1] if back[1] is not None else torch.zeros_like(pose)
            d_traj[t] = (post_share + pre_share).numpy()
        if with_params:                 # step T-1 adds first, step 0 last
            for k, g in zip(d_params, got):
                d_params[k] = d_params[k] + g
    return final, records, d_window.numpy(), d_traj, None if d_params is None else {k: v.numpy() for k, v in d_params.items()}
