"""CPU: the numpy restatement of the rollout's L1 loss (tests/train_rollout_cases.py) against torch autograd, the identity that ties
training on a rollout to training one step ahead, and the case table's own regime -- what tests/test_gpu_train_rollout.py holds
the kernels to is checked here first.

Bounds.  The gradient: bit equality with what autograd back-propagates through ``L1Loss(reduction='sum')`` on the same slices
(INTEGRATION.md 2e's loss; counts below 2^24).  The loss: 1e-12 relative against float64 torch on the same float32 differences (two
float64 summation orders of at most 450 000 terms).  The identity: 1e-9 relative, in float64 -- in float32 the positions cancel
(a position is ~0.5, a step's acceleration ~1e-4 of it), so it is a statement about the formulas, not about the device."""
import numpy as np
import pytest
import torch

from conftest import STATS
from oracle import epd_oracle as orc
from oracle import torch_epd
import grad_cases as gc
import rollout_grad_cases as rc
import train_rollout_cases as trc
import yardstick

L0 = trc.L0


def test_table_sits_on_the_loss_kernels_edges():
    wg, cap = trc.LOSS_WG, trc.LOSS_GRID_MAX
    assert {1, wg - 1, wg, wg + 1} <= set(trc.LOSS_ROWS)
    big = max(trc.LOSS_ROWS)
    assert big > wg * cap and trc.loss_regime(big) == (cap, 2) and big % wg != 0            # a second, ragged pass of the capped grid
    assert set(trc.LOSS_STEPS) == {1, 2, 3} and set(trc.LOSS_K) == {2, 6}                   # no record / one record / more; the shortest window
    assert set(trc.LOSS_FRAME_DIMS) == {trc.LOSS_D, trc.LOSS_D - 3} and trc.LOSS_CART + 3 <= trc.LOSS_D - 3
    assert len(trc.loss_cases(1)) == 3 * 2 * 2 * 4
    scales = [m[2] for m in trc.LOSS_MASKS.values() if m[2] is not None]
    assert any(m[2] is None for m in trc.LOSS_MASKS.values()) and all(len(set(s)) == 3 for s in scales)


@pytest.mark.parametrize("n", trc.LOSS_ROWS)
def test_loss_cases_hold_what_they_are_for(n):
    c0 = trc.LOSS_CART
    for steps, k, fd, mask in trc.loss_cases(n):
        case = trc.loss_case(n, steps, k, fd, mask)
        w, f, fr = case["windows"], case["final"], case["frames"]
        assert w.shape == (steps, k, n, trc.LOSS_D) and fr.shape == (steps, n, fd)
        loss, count, d_rec, d_fin = trc.rollout_l1_restated(w, f, fr, c0, case["rank"], case["material_col"], case["pos_scale"])
        what = (n, steps, k, fd, mask)
        if mask == "empty":
            assert count == 0 and np.isnan(loss) and not d_rec.any() and not d_fin.any(), what
            continue
        assert count >= 1 and np.isfinite(loss), what
        row = n // 2
        equal = sum(int((trc.predicted(w, f, t)[:, c0:c0 + 3] == fr[t][:, c0:c0 + 3]).sum()) for t in range(steps))
        assert equal >= 1 and d_fin[k - 1, row, c0 + 2] == 0 and np.abs(d_fin[k - 1, row]).sum() > 0, what      # on a counted row
        # zeros everywhere but the xyz of the scored frames
        assert not d_rec[0].any() and not d_fin[:k - 1].any(), what
        other = [c for c in range(trc.LOSS_D) if not c0 <= c < c0 + 3]
        assert not d_rec[:, :, other].any() and not d_fin[:, :, other].any(), what
        assert all(d_rec[t].any() for t in range(1, steps)), what
        counted = trc.counted_rows(w, case["rank"], case["material_col"])
        assert not d_fin[k - 1][~counted].any() and (np.abs(d_fin[k - 1][counted][:, c0:c0 + 2]) > 0).all(), what
        if mask == "none":
            assert count == n
        elif n > 2:
            assert 0 < count < n, what
            assert (case["rank"] >= 0).any() and sorted(case["rank"][case["rank"] >= 0]) == list(range(int((case["rank"] >= 0).sum())))
        if case["material_col"] >= 0 and n > 1:
            # the wrong column, or the right column of the wrong frame or window, counts other rows
            for wrong in (0, trc.LOSS_D - 1):
                assert not np.array_equal(trc.counted_rows(w, case["rank"], wrong), counted), (what, wrong)
            shifted = np.concatenate((w[:1, :1], w[:1, :-1]), axis=1) if k > 1 else w
            assert not np.array_equal(trc.counted_rows(shifted, case["rank"], case["material_col"]), counted), what
        if case["pos_scale"] is not None:
            g = np.abs(d_fin[k - 1][counted][:, c0:c0 + 3]).max(axis=0)
            assert len(set(g)) == 3, what                                                    # a scale per axis


def _torch_loss(case, dtype):
    """INTEGRATION.md 2e's loss by autograd, on the float32 differences: (loss, d loss / d (pred - frame) [steps, n, 3])."""
    w, f, fr, c0 = case["windows"], case["final"], case["frames"], trc.LOSS_CART
    steps = len(w)
    counted = torch.tensor(trc.counted_rows(w, case["rank"], case["material_col"]))
    count = int(counted.sum())
    d32 = np.stack([trc.predicted(w, f, t)[:, c0:c0 + 3] - fr[t][:, c0:c0 + 3] for t in range(steps)])
    d = torch.tensor(d32, dtype=dtype, requires_grad=True)
    crit = torch.nn.L1Loss(reduction="sum")
    scale = case["pos_scale"] or (1.0, 1.0, 1.0)
    picked = d[:, counted]
    loss = sum(crit(picked[:, :, c], torch.zeros_like(picked[:, :, c])) / ((scale[c] * steps) * count) for c in range(3))
    loss.backward()
    return float(loss.detach()), d.grad.numpy()


@pytest.mark.parametrize("n", [257, 5000])
@pytest.mark.parametrize("mask", ["none", "rigid", "rigid_material"])
def test_loss_restatement_is_torchs_gradient_bit_for_bit(n, mask):
    c0 = trc.LOSS_CART
    for steps, k in ((1, 2), (3, 6)):
        case = trc.loss_case(n, steps, k, trc.LOSS_D - 3, mask)
        loss, count, d_rec, d_fin = trc.rollout_l1_restated(case["windows"], case["final"], case["frames"], c0, case["rank"],
                                                            case["material_col"], case["pos_scale"])
        got = np.stack([(d_rec[t + 1] if t + 1 < steps else d_fin[k - 1])[:, c0:c0 + 3] for t in range(steps)])
        l64, g64 = _torch_loss(case, torch.float64)
        assert abs(loss - l64) <= 1e-12 * abs(l64), (n, mask, steps, loss, l64)
        assert yardstick.same_bits(got, g64.astype(np.float32)), (n, mask, steps)
        assert (got == 0).sum() == 1 + 3 * steps * (n - count)                               # sign(0) = 0 once, the rows that do not count
        if case["pos_scale"] is None:                                                        # float32 autograd itself: 2e's loop
            l32, g32 = _torch_loss(case, torch.float32)
            assert yardstick.same_bits(got, g32), (n, mask, steps)
            assert abs(loss - l32) <= 1e-5 * abs(l64)


def test_one_step_with_acc_std_is_the_one_step_training_loss():
    """steps = 1, pos_scale = acc_std:  |p + (p - p') + (a std + mean) - next| / std = |a - ((next - 2p + p') - mean) / std|, the
    L1 training loss of train_dyn.py:58-65 on compute_target -- over the rows that are not rigid."""
    obs = gc.step_state("step_a")
    rows = gc.rigid_rows(obs, L0)
    free = np.setdiff1d(np.arange(obs.shape[1]), rows)
    frame = trc.step_frames("step_a").astype(np.float64)[:1]                                   # the recorded frame behind the window
    pose = gc.t64(frame[0][rows][:, L0.cart:L0.cart + 3])
    ei = torch.tensor(rc.oracle_edge_lists("step_a")[0])
    p = rc.p_of(torch.float64)
    o64 = gc.t64(obs)
    with torch.no_grad():
        pre = gc.state_pre(o64, L0, torch.tensor(rows), pose)
        nodes = gc.node_features(pre, L0)
        ea = gc.edge_features(pre[-1][:, L0.cart:L0.cart + 3], ei[0], ei[1])
        pred = torch_epd.epd_forward(p, nodes, ea, ei, gc.STEP_DIMS[4], gc.STEP_DIMS[5])
        final, _ = gc.step(p, o64, L0, torch.tensor(rows), pose, ei, gc.STEP_DIMS[4], gc.STEP_DIMS[5])
    target = trc.compute_target64(obs, frame[0][:, L0.cart:L0.cart + 3])
    want32 = orc.compute_target(obs, frame[0][:, L0.cart:L0.cart + 3].astype(np.float32), STATS, [2, 3, 4])
    assert np.abs(target - want32).max() <= 1e-2 * np.abs(target).max()                       # the float32 oracle's, up to its cancellation
    one_step = np.abs(pred.numpy() - target)[free].sum() / len(free)
    loss, count, _, _ = trc.rollout_l1_restated(o64.numpy()[None], final.numpy(), frame, L0.cart, trc.rigid_rank(obs), -1, trc.ACC_STD,
                                                dtype=np.float64)
    print(f"\n[train rollout] one-step loss {one_step:.12e}, rollout loss at steps = 1 {loss:.12e}")
    assert count == len(free) and abs(loss - one_step) <= 1e-9 * one_step
    # with the material column in force the rows of material 2 drop out of both
    sand = np.nonzero(obs[-1][:, L0.mat] < 0.5)[0]
    loss_m, count_m, _, _ = trc.rollout_l1_restated(o64.numpy()[None], final.numpy(), frame, L0.cart, trc.rigid_rank(obs), L0.mat,
                                                    trc.ACC_STD, dtype=np.float64)
    assert count_m == len(sand) < count and abs(loss_m - np.abs(pred.numpy() - target)[sand].sum() / len(sand)) <= 1e-9 * loss_m


def test_step_scene_is_in_its_regime():
    obs = gc.step_state("step_a")
    rigid = gc.rigid_rows(obs, L0)
    free = np.setdiff1d(np.arange(obs.shape[1]), rigid)
    frames, clean = trc.step_frames("step_a"), trc.oracle_rollout("step_a")
    c = slice(L0.cart, L0.cart + 3)
    assert frames.shape == (trc.T, gc.STEP_N, L0.D) and trc.step_frames("step_a", frame_dim=L0.D - 3).shape[2] == L0.D - 3
    assert np.array_equal(frames[:, rigid][:, :, c], rc.trajectory("step_a"))                 # the rigid rows follow the recording
    drift = np.abs(frames[:, free][:, :, c] - clean[:, free][:, :, c])
    assert 0.2 * trc.DRIFT < drift.mean() < 2 * trc.DRIFT and (drift > 0).mean() > 0.99       # a loss of the drift's size, both signs
    rank = trc.rigid_rank(obs)
    assert np.array_equal(np.nonzero(rank >= 0)[0], rigid) and list(rank[rigid]) == list(range(len(rigid)))
    assert 0 < (obs[-1][free][:, L0.mat] > 0.5).sum() < len(free)                             # the material column changes the count
    assert trc.non_overlapping_starts([20, 20], 6, 4) == [0, 4, 8, 14, 18, 22]
    assert trc.non_overlapping_starts([12], 6, 8) == []
