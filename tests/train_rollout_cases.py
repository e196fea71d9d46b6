"""Cases and the numpy restatement of training on a rollout in the library (csrc/train_step.hip: gm_rollout_l1_loss,
gm_train_rollout_step; the contract is in include/gnn_manip_hip.h) -- a plain helper module (no test) of
tests/test_train_rollout_cases.py (CPU: the restatement against torch autograd, the identity with the one-step training loss, the
table's own regime), tests/test_abi_train_rollout.py and tests/test_gpu_train_rollout.py (the kernels against the restatement).

The loss.  Step t is scored on the last frame of the window the step left -- windows[t + 1], or the final state for the last step
-- against frames[t], over the rows that are not rigid and, with a material column, whose flag in the last frame of windows[0] is
below 0.5:  loss = sum_c (float64 sum of the float32 |pred - frame| on axis c) / scale_c / (steps * count);  an element of the
gradient is sign(pred - frame) * (float)(1.0 / ((scale_c * steps) * count)), on record t + 1 (the final state's last frame for the
last step).

The step scene is tests/rollout_grad_cases.py's (400 nodes, STEP_DIMS, T = 4, its trajectory): the recorded frames are the float64
oracle rollout's positions plus a seeded drift on the free rows and the scripted poses on the rigid rows."""
import functools

import numpy as np
import torch

from conftest import STATS
import grad_cases as gc
import rollout_grad_cases as rc
from train_step_cases import LOSS_GRID_MAX, LOSS_ROWS, LOSS_WG, loss_regime  # noqa: F401  (the loss kernels share their geometry)

L0 = rc.L0
T = rc.T
ACC_STD = tuple(STATS["acceleration_std"])

# ---------------------------------------------------------------------------------------------- the loss kernel's table
LOSS_STEPS = (1, 2, 3)
LOSS_K = (2, 6)
LOSS_D, LOSS_CART, LOSS_MAT = 8, 2, 1            # the default scene's columns: id, material, xyz, three control columns
LOSS_FRAME_DIMS = (LOSS_D, LOSS_D - 3)
# name -> (rigid rows given, material column in force, position scale)
LOSS_MASKS = {"none": (False, False, None), "rigid": (True, False, (0.5, 2.0, 3.0)), "rigid_material": (True, True, ACC_STD),
              "empty": (True, True, None)}


def loss_cases(n):
    """Every (steps, k, frame_dim, mask) of the table at n rows."""
    return [(s, k, fd, m) for s in LOSS_STEPS for k in LOSS_K for fd in LOSS_FRAME_DIMS for m in LOSS_MASKS]


def loss_case(n, steps, k, frame_dim, mask, seed=0):
    """dict(windows [steps,k,n,D], final [k,n,D], frames [steps,n,frame_dim], rank int32 [n] or None, material_col, pos_scale) of
    a synthetic case: normal values, ONE exactly equal element on a counted row (sign 0) in the last step.  With rigid rows: a
    seeded third of the rows, ranked in ascending order.  With a material column: a 0 / 1 flag in the last frame of windows[0]
    (at least one row of each kind where n allows), its complement in the other label columns of that frame and in the material
    column of every other frame and window -- reading the wrong column or the wrong frame counts the wrong rows.  "empty": every
    flag is 1, nothing counts."""
    with_rigid, with_material, scale = LOSS_MASKS[mask]
    rng = np.random.default_rng([seed, n, steps, k, frame_dim, sorted(LOSS_MASKS).index(mask)])
    windows = rng.standard_normal((steps, k, n, LOSS_D)).astype(np.float32)
    final = rng.standard_normal((k, n, LOSS_D)).astype(np.float32)
    frames = rng.standard_normal((steps, n, frame_dim)).astype(np.float32)
    row = n // 2                                   # the counted row that holds the equal element
    rank = None
    if with_rigid:
        rigid = rng.random(n) < 0.33
        rigid[row] = False
        if n > 2:
            rigid[(row + 2) % n] = True
        rank = np.where(rigid, np.cumsum(rigid) - 1, -1).astype(np.int32)
    col = -1
    if with_material:
        col = LOSS_MAT
        flag = (rng.random(n) < 0.4).astype(np.float32)
        flag[row] = 0.0
        if n > 1:
            flag[(row + 1) % n] = 1.0
        if mask == "empty":
            flag[:] = 1.0
        windows[:, :, :, col] = 1.0 - flag
        final[:, :, col] = 1.0 - flag
        windows[0, k - 1, :, 0] = 1.0 - flag
        windows[0, k - 1, :, LOSS_CART + 3:] = (1.0 - flag)[:, None]
        windows[0, k - 1, :, col] = flag
    frames[steps - 1, row, LOSS_CART + 2] = final[k - 1, row, LOSS_CART + 2]
    return dict(windows=windows, final=final, frames=frames, rank=rank, material_col=col, pos_scale=scale)


def predicted(windows, final, t):
    """The frame step t is scored on."""
    return windows[t + 1][-1] if t + 1 < len(windows) else final[-1]


def counted_rows(windows, rank, material_col):
    n = windows.shape[2]
    counted = np.ones(n, bool) if rank is None else np.asarray(rank) < 0
    if material_col >= 0:
        counted &= np.asarray(windows[0][-1][:, material_col], np.float32) < np.float32(0.5)
    return counted


def rollout_l1_restated(windows, final, frames, cart, rank=None, material_col=-1, pos_scale=None, dtype=np.float32):
    """(loss float64, rows counted, d_records float32 [steps,n,D], d_final float32 [k,n,D]) as gm_rollout_l1_loss defines them.
    dtype: the arithmetic of pred - frame (float32 is the library's; float64 serves the identity with the one-step loss)."""
    windows, final, frames = (np.asarray(a, dtype) for a in (windows, final, frames))
    steps, k, n, D = windows.shape
    assert final.shape == (k, n, D) and frames.shape[:2] == (steps, n)
    scale = (1.0, 1.0, 1.0) if pos_scale is None else tuple(float(s) for s in pos_scale)
    counted = counted_rows(windows, rank, material_col)
    count = int(counted.sum())
    d_records, d_final = np.zeros((steps, n, D), np.float32), np.zeros((k, n, D), np.float32)
    if count == 0:
        return float("nan"), 0, d_records, d_final
    g = [np.float32(1.0 / ((scale[c] * steps) * count)) for c in range(3)]
    sums = np.zeros(3)
    for t in range(steps):
        d = predicted(windows, final, t)[:, cart:cart + 3] - frames[t][:, cart:cart + 3]        # in `dtype`
        assert d.dtype == dtype
        sums += np.abs(d)[counted].astype(np.float64).sum(axis=0)
        out = d_records[t + 1] if t + 1 < steps else d_final[k - 1]
        for c in range(3):
            out[counted, cart + c] = np.sign(d[counted, c]).astype(np.float32) * g[c]
    loss = float(((sums[0] / scale[0] + sums[1] / scale[1]) + sums[2] / scale[2]) / (float(steps) * float(count)))
    return loss, count, d_records, d_final


# ---------------------------------------------------------------------------------------------- the step scene
DRIFT_SEED, DRIFT = 12, 2e-5      # the free rows' recorded positions differ from the rollout's by about a tenth of a step's motion


@functools.lru_cache(maxsize=None)
def oracle_rollout(name="step_a", steps=T):
    """[steps, N, D] float64: the last frame after every step of the float64 restated rollout (rollout_grad_cases) of
    step_state(name) under its trajectory, on the oracle's edge lists."""
    p = rc.p_of(torch.float64)
    obs = gc.t64(gc.step_state(name))
    rows = torch.tensor(gc.rigid_rows(obs.numpy(), L0))
    tr = rc.trajectory(name, steps=steps)
    out = []
    with torch.no_grad():
        for t, ei in enumerate(rc.oracle_edge_lists(name, True, steps)):
            obs, _ = gc.step(p, obs, L0, rows, gc.t64(tr[t]), torch.tensor(ei), gc.STEP_DIMS[4], gc.STEP_DIMS[5])
            out.append(obs[-1].numpy())
    out = np.stack(out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def step_frames(name="step_a", steps=T, frame_dim=None):
    """[steps, N, frame_dim] float32 recorded frames for step_state(name): the oracle rollout's last frames with a seeded drift on
    the xyz of the free rows and the scripted poses (rollout_grad_cases.trajectory) on the rigid rows."""
    obs = gc.step_state(name)
    frames = oracle_rollout(name, steps).astype(np.float32)
    rigid = gc.rigid_rows(obs, L0)
    free = np.setdiff1d(np.arange(obs.shape[1]), rigid)
    c = slice(L0.cart, L0.cart + 3)
    drift = (DRIFT * np.random.default_rng(DRIFT_SEED).standard_normal((steps, len(free), 3))).astype(np.float32)
    for t in range(steps):
        frames[t][free, c] = frames[t][free, c] + drift[t]
        frames[t][rigid, c] = rc.trajectory(name, steps=steps)[t]
    frames = np.ascontiguousarray(frames[:, :, :frame_dim or L0.D])
    frames.setflags(write=False)
    return frames


def rigid_rank(obs):
    """int32 [N]: gm_rigid_rank's output for a window -- the rank of a rigid row among the rigid rows, -1 elsewhere."""
    rigid = np.asarray(obs)[-1][:, L0.mat] == 1
    return np.where(rigid, np.cumsum(rigid) - 1, -1).astype(np.int32)


def compute_target64(obs, next_pos):
    """oracle/epd_oracle.compute_target in float64: the one-step training target, the normalised acceleration."""
    pos = np.asarray(obs, np.float64)[:, :, L0.cart:L0.cart + 3]
    acc = np.asarray(next_pos, np.float64) - 2.0 * pos[-1] + pos[-2]
    return (acc - np.asarray(STATS["acceleration_mean"])) / np.asarray(STATS["acceleration_std"])


def non_overlapping_starts(frames_per_sim, k, steps):
    """Trainer.fit_rollout_epoch's default: per recording every `steps`-th sample whose `steps` frames are all recorded."""
    starts, first = [], 0
    for n_frames in frames_per_sim:
        starts += [first + t for t in range(0, n_frames - k - steps + 1, steps)]
        first += n_frames - k
    return starts
