"""Training on a rollout in the library, on the MI355X (csrc/train_step.hip: gm_rollout_l1_loss, gm_train_rollout_step;
gnn_manip_amd/train.py: Trainer.step_rollout / evaluate_rollout / fit_rollout_epoch; CoffeeDataset.rollout_sample).

Bounds.  The loss's count and gradients, the forward's windows, the parameter gradients, weights and moments: bit equality -- with
the numpy restatements (tests/train_rollout_cases.py, tests/train_step_cases.py) and with the existing entry points the call is
composed of (RolloutEngine.step / run, gm_rollout_backward_train).  A loss: 1e-12 relative against the float64 numpy sum of the same
float32 differences.  The parameter gradients against the float64 restated sweep (tests/rollout_train_cases.py) on the device's
edge lists: the rule of tests/yardstick.py with the ReLU flip allowance.  Every figure is printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc
import grad_cases as gc
import rollout_grad_cases as rc
import rollout_train_cases as tc
import train_rollout_cases as trc
import train_step_cases as sc
from gpu_support import K_NB, dev, edges_of, forward_windows, load_model, poison_allocator, step_engine, to_dev
from grad_cases import L0, flip_allowance
from yardstick import lazy, same_bits, within

pytestmark = pytest.mark.gpu

LR = 1e-3
T = trc.T
NAN = float("nan")


# ------------------------------------------------------------------------------------------ the calls
def _loss_call(windows, final, frames, fd, rank, col, scale, dev, grads=True):
    """gm_rollout_l1_loss through ctypes in a NaN-filled workspace, outputs pre-filled: (loss [1] float64 numpy, count, d_records,
    d_final)."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    steps, k, n, D = windows.shape
    need = L.gm_rollout_l1_loss_workspace_bytes(n, steps)
    assert need > 0
    ws = torch.full((need // 4 + 1,), NAN, device=dev).view(torch.uint8)
    loss = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    rows = torch.full((1,), -1, dtype=torch.int64, device=dev)
    d_rec = torch.full((steps, n, D), NAN, device=dev) if grads else None
    d_fin = torch.full((k, n, D), NAN, device=dev) if grads else None
    arr = None if scale is None else (C.c_double * 3)(*scale)
    check(L.gm_rollout_l1_loss(ptr(windows), ptr(final), ptr(frames), int(frames.shape[2]), steps, n, C.byref(fd), ptr(rank), col, arr,
                               ptr(loss), ptr(rows), ptr(d_rec), ptr(d_fin), ptr(ws), need, current_stream(dev)))
    return loss.cpu().numpy(), int(rows), d_rec, d_fin


def _close(got, want):
    return abs(got - want) <= 1e-12 * abs(want)


def _state(t):
    from gnn_manip_amd import train
    return [t.export(w) for w in (train.PARAMS, train.EXP_AVG, train.EXP_AVG_SQ)]


def _same_state(a, b, what):
    for kind, ta, tb in zip(("weights", "exp_avg", "exp_avg_sq"), a, b):
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert same_bits(u, v), (what, kind, i)


def _params(hidden):
    return rc.params() if hidden == 128 else orc.init_params(25, 4, 3, hidden, 2, 2, 845 + hidden)


def _setup(dev, hidden=128, sand_only=False, frame_dim=None, name="step_a"):
    """(trainer, module, engine after set_scene, obs0, frames on the device, the numpy window and frames)."""
    from gnn_manip_amd import Trainer
    dims = (25, 4, 3, hidden, 2, 2)
    m = load_model(_params(hidden), dims, dev)
    eng = step_engine(m, dev)
    obs_np, frames_np = gc.step_state(name), trc.step_frames(name, frame_dim=frame_dim)
    obs, frames = to_dev(obs_np, dev), to_dev(frames_np, dev)
    assert eng.set_scene(obs) == len(gc.rigid_rows(obs_np, L0)) > 0
    t = Trainer(m, lr=LR, sand_only=sand_only, material_col=sc.MATERIAL_COL if sand_only else None)
    return t, m, eng, obs, frames, obs_np, frames_np


def _chain(eng, obs_np, frames, col, scale, dev):
    """One training step's gradients from the existing entry points, with the MODULE's weights: the engine's forward keeping its
    windows under the poses gathered by torch indexing, the standalone loss, gm_rollout_backward_train into zeroed buffers:
    (windows, final, trajectory, loss, count, d_records, d_final, grads)."""
    steps = int(frames.shape[0])
    rigid = eng.rigid_rank >= 0
    traj = frames[:, rigid, L0.cart:L0.cart + 3].contiguous()
    windows, final = forward_windows(eng, obs_np, traj.cpu().numpy(), steps, dev)
    loss, count, d_rec, d_fin = _loss_call(windows, final, frames, eng.fdesc, eng.rigid_rank, col, scale, dev)
    grads = [torch.zeros_like(p) for p in eng._training_model()[1]]
    eng._sweep_backward(windows, traj, steps, d_fin, (eng.rigid_rank, eng.n_rigid), False, d_records=d_rec, grads=grads)
    return windows, final, traj, loss, count, d_rec, d_fin, grads


# ------------------------------------------------------------------------------------------ 1. gm_rollout_l1_loss alone
@pytest.mark.parametrize("n", trc.LOSS_ROWS)
def test_rollout_l1_loss_is_the_restatement(dev, n):
    from gnn_manip_amd.graph import make_feature_desc
    c0 = trc.LOSS_CART
    for steps, k, frame_dim, mask in trc.loss_cases(n):
        case = trc.loss_case(n, steps, k, frame_dim, mask)
        want_loss, want_count, want_rec, want_fin = trc.rollout_l1_restated(case["windows"], case["final"], case["frames"], c0, case["rank"],
                                                                             case["material_col"], case["pos_scale"])
        fd = make_feature_desc(0.015, STATS, BOUNDS, CART, MAT, CTRL, k, trc.LOSS_D)
        w, f, fr = (to_dev(case[key], dev) for key in ("windows", "final", "frames"))
        rank = None if case["rank"] is None else to_dev(case["rank"], dev)
        runs = [_loss_call(w, f, fr, fd, rank, case["material_col"], case["pos_scale"], dev) for _ in range(2)]
        (l0, r0, rec0, fin0), (l1, r1, rec1, fin1) = runs
        what = (n, steps, k, frame_dim, mask)
        assert l0.view(np.uint64) == l1.view(np.uint64) and r0 == r1 and same_bits(rec0, rec1) and same_bits(fin0, fin1), what
        assert r0 == want_count, (what, r0, want_count)
        assert same_bits(rec0, want_rec) and same_bits(fin0, want_fin), what       # fully written: no NaN of the pre-fill is left
        if want_count == 0:
            assert mask == "empty" and np.isnan(l0[0]) and not rec0.any() and not fin0.any(), what
        else:
            assert _close(l0[0], want_loss), (what, l0[0], want_loss)
        alone = _loss_call(w, f, fr, fd, rank, case["material_col"], case["pos_scale"], dev, grads=False)   # the loss alone
        assert alone[0].view(np.uint64) == l0.view(np.uint64) and alone[1] == r0, what
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ 2. the forward
@pytest.mark.parametrize("frame_dim", [None, L0.D - 3], ids=["frames_D", "frames_D-3"])
def test_forward_keeps_the_engines_windows(dev, frame_dim):
    t, m, eng, obs, frames, obs_np, frames_np = _setup(dev, frame_dim=frame_dim)
    before = _state(t)
    obs_bits = obs.clone()
    t.evaluate_rollout(eng, obs, frames)
    kept = t.kept_windows().clone()
    assert kept.shape == (T + 1, L0.k, gc.STEP_N, L0.D) and same_bits(obs, obs_bits)      # obs0 is not written
    rigid = eng.rigid_rank >= 0
    traj = frames[:, rigid, L0.cart:L0.cart + 3].contiguous()
    assert same_bits(traj, rc.trajectory("step_a"))
    windows, final = forward_windows(eng, obs_np, traj.cpu().numpy(), T, dev)
    assert same_bits(kept[:T], windows) and same_bits(kept[T], final)
    ran = obs.clone()
    eng.set_scene(ran)
    eng.run(ran, traj, T)                                                                  # gm_rollout
    assert same_bits(kept[T], ran)
    want = trc.rollout_l1_restated(windows.cpu().numpy(), final.cpu().numpy(), frames_np, L0.cart, trc.rigid_rank(obs_np))[0]
    print(f"\n[train rollout] evaluate_rollout: loss {float(t.last_loss):.9e}, restated {want:.9e}")
    assert _close(float(t.last_loss), want)
    # fewer steps than frames: the first ones
    t.evaluate_rollout(eng, obs, frames, steps=2)
    assert same_bits(t.kept_windows()[:3], kept[:3])
    _same_state(_state(t), before, "evaluate_rollout")
    assert t.record() == dict(steps_applied=0, steps_skipped=0, beta1_pow=1.0, beta2_pow=1.0)


# ------------------------------------------------------------------------------------------ 3. the gradients and the update
@pytest.mark.parametrize("sand_only", [False, True], ids=["all_free_rows", "sand_only"])
@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_one_step_has_the_sweeps_gradients_and_the_restated_update(dev, hidden, sand_only):
    from gnn_manip_amd import train
    t, m, eng, obs, frames, obs_np, frames_np = _setup(dev, hidden, sand_only)
    col = L0.mat if sand_only else -1
    scale = trc.ACC_STD if sand_only else None
    w0 = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    windows, final, traj, loss, count, d_rec, d_fin, want = _chain(eng, obs_np, frames, col, scale, dev)
    free = int((eng.rigid_rank < 0).sum())
    assert count == (int((obs_np[-1][:, L0.mat] < 0.5).sum()) if sand_only else free) and 0 < count <= free
    t.step_rollout(eng, obs, frames, pos_scale=scale)
    got = t.export(train.GRADS)
    for i, (g, ref) in enumerate(zip(got, want)):
        assert same_bits(g, ref), (hidden, "gradient", i, float((g - ref).abs().max()))
    assert all(torch.isfinite(g).all() for g in got) and any(float(g.abs().max()) > 0 for g in got)
    assert float(t.last_loss) == float(loss[0])
    state = sc.adam_state(w0)
    w1 = sc.adam_restated(w0, [g.cpu().numpy() for g in want], state, LR)
    _same_state(_state(t), (w1, state["m"], state["v"]), hidden)
    assert t.record()["steps_applied"] == 1 and t.record()["steps_skipped"] == 0


# ------------------------------------------------------------------------------------------ 4. against float64
def test_gradients_against_the_float64_restated_sweep(dev):
    from gnn_manip_amd import train
    t, m, eng, obs, frames, obs_np, frames_np = _setup(dev)
    t.step_rollout(eng, obs, frames, pos_scale=trc.ACC_STD)
    got = t.export(train.GRADS)
    kept = t.kept_windows()
    windows, final = kept[:T].clone(), kept[T].clone()
    eis = [edges_of(windows[i], eng) for i in range(T)]
    _, count, w_rec, w_fin = trc.rollout_l1_restated(windows.cpu().numpy(), final.cpu().numpy(), frames_np, L0.cart, trc.rigid_rank(obs_np),
                                                     -1, trc.ACC_STD)
    assert count > 0
    traj_np = rc.trajectory("step_a")
    params = rc.params()
    r64 = tc.reverse_sweep(params, obs_np, traj_np, eis, w_fin, w_rec)
    r32 = tc.reverse_sweep(params, obs_np, traj_np, eis, w_fin, w_rec, dtype=torch.float32)

    def compute():
        p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
        o = gc.t64(obs_np, True)
        tg = [gc.t64(x, True) for x in traj_np]

        def run(fwd):
            fin, recs = tc.unrolled(p, o, tg, eis, forward=fwd)
            return tc.loss_of(fin, recs, w_fin, w_rec)
        bounds, units = flip_allowance(run, [o] + tg + list(p.values()))
        return dict(zip(p, bounds[1 + len(tg):])), units
    allow = lazy(compute)
    assert len(got) == len(params)
    for name, g in zip(params, got):
        within(f"step_rollout {name}", g.cpu().numpy(), r64[4][name], r32[4][name], lambda name=name: (allow()[0][name], allow()[1]),
               tag="[train rollout]")


# ------------------------------------------------------------------------------------------ 5. three steps
def test_three_steps_are_the_chain_bit_for_bit(dev):
    from gnn_manip_amd import train
    t, m, eng, obs, frames, obs_np, frames_np = _setup(dev, sand_only=True)
    rank_np = trc.rigid_rank(obs_np)

    def restated_loss():
        """Of the module's weights as they stand."""
        rigid = eng.rigid_rank >= 0
        windows, final = forward_windows(eng, obs_np, frames[:, rigid, L0.cart:L0.cart + 3].cpu().numpy(), T, dev)
        return trc.rollout_l1_restated(windows.cpu().numpy(), final.cpu().numpy(), frames_np, L0.cart, rank_np, L0.mat)[0]

    t.evaluate_rollout(eng, obs, frames)
    first = float(t.last_loss)
    assert _close(first, restated_loss())
    w = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    state = sc.adam_state(w)
    slots = torch.zeros(3, dtype=torch.float64, device=dev)
    for i in range(3):
        t.sync_module()                                            # the module (the chain's model) takes the trainer's weights
        for p, want in zip(m.parameters(), w):
            assert same_bits(p, want), i
        *_, loss, count, d_rec, d_fin, grads = _chain(eng, obs_np, frames, L0.mat, None, dev)
        t.step_rollout(eng, obs, frames, loss_out=slots[i:i + 1])
        for j, (g, ref) in enumerate(zip(t.export(train.GRADS), grads)):
            assert same_bits(g, ref), (i, j)
        w = sc.adam_restated(w, [g.cpu().numpy() for g in grads], state, LR)
        _same_state(_state(t), (w, state["m"], state["v"]), i)
        assert float(slots[i]) == float(loss[0])
    t.sync_module()
    t.evaluate_rollout(eng, obs, frames)
    last = float(t.last_loss)
    assert _close(last, restated_loss())
    print(f"\n[train rollout] loss before three steps {first:.6e}, per step {slots.cpu().numpy()}, after {last:.6e}")
    _same_state(_state(t), (w, state["m"], state["v"]), "evaluate_rollout changes nothing")
    rec = t.record()
    assert (rec["steps_applied"], rec["steps_skipped"]) == (3, 0) and rec["beta1_pow"] == state["b1p"] and rec["beta2_pow"] == state["b2p"]


# ------------------------------------------------------------------------------------------ 6. skips and errors
def test_a_nan_frame_is_skipped_and_a_poisoned_allocator_changes_no_bit(dev):
    t, m, eng, obs, frames, obs_np, frames_np = _setup(dev, hidden=64)
    twin, _, eng2, _, _, _, _ = _setup(dev, hidden=64)
    t.step_rollout(eng, obs, frames)
    poison_allocator(dev, NAN)
    twin.step_rollout(eng2, obs, frames)                              # its workspace comes out of the poisoned blocks
    _same_state(_state(t), _state(twin), "poisoned allocator")
    assert float(t.last_loss) == float(twin.last_loss)
    before, rec0 = _state(t), t.record()
    bad = frames.clone()
    row = int(torch.nonzero(eng.rigid_rank < 0)[5])                   # a counted row
    bad[2, row, L0.cart + 1] = NAN
    slot = torch.zeros(1, dtype=torch.float64, device=dev)
    t.step_rollout(eng, obs, bad, loss_out=slot)
    assert np.isnan(float(slot))
    _same_state(_state(t), before, "skipped step")
    assert t.record() == dict(rec0, steps_skipped=rec0["steps_skipped"] + 1) and t.record()["steps_skipped"] == 1
    t.evaluate_rollout(eng, obs, bad, loss_out=slot)                  # update = 0: nothing moves, the record included
    assert np.isnan(float(slot)) and t.record()["steps_skipped"] == 1
    _same_state(_state(t), before, "evaluate_rollout")
    t.step_rollout(eng, obs, frames)                                  # the next good step is the twin's
    twin.step_rollout(eng2, obs, frames)
    _same_state(_state(t), _state(twin), "the next good step")
    assert t.record()["steps_applied"] == 2 and twin.record() == dict(t.record(), steps_skipped=0)


def test_refusals(dev):
    from gnn_manip_amd import EncProcDecGNN, Trainer
    from gnn_manip_amd._lib import current_stream, lib, ptr
    t, m, eng, obs, frames, obs_np, frames_np = _setup(dev, hidden=64)
    before = _state(t)
    for bad, match in ((dict(steps=0), "steps=0"), (dict(steps=T + 1), "steps=5"), (dict(pos_scale=(1.0, 0.0, 1.0)), "pos_scale"),
                       (dict(loss_out=torch.zeros(1, device=dev)), "loss_out")):
        with pytest.raises(ValueError, match=match):
            t.step_rollout(eng, obs, frames, **bad)
    with pytest.raises(ValueError, match="columns"):
        t.step_rollout(eng, obs, frames[:, :, :6].contiguous())
    with pytest.raises(ValueError, match="obs0"):
        t.step_rollout(eng, obs[:-1].contiguous(), frames)
    with pytest.raises(ValueError, match="frames"):
        t.step_rollout(eng, obs, frames[:, :-1].contiguous())
    with pytest.raises(ValueError, match="frames"):
        t.step_rollout(eng, obs, frames.double())
    with pytest.raises(ValueError, match="set_scene"):
        t.step_rollout(step_engine(m, dev), obs, frames)
    with pytest.raises(ValueError, match="64, 128 and 256"):
        Trainer(EncProcDecGNN(25, 4, 3, 100, 2, 2))
    # the C entry point itself
    L = lib()
    err = lambda: L.gm_last_error().decode()
    n, nr, s = eng.n, eng.n_rigid, current_stream(dev)
    need = L.gm_train_rollout_step_workspace_bytes(C.byref(t.desc), C.byref(eng.fdesc), n, nr, K_NB, T)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    args = dict(obs=obs, frames=frames, rank=eng.rigid_rank, frame_dim=L0.D, steps=T, col=-1, ws=ws, ws_bytes=need, lr=LR)

    def call(**kw):
        a = dict(args, **kw)
        return L.gm_train_rollout_step(t._h, ptr(a["obs"]), n, C.byref(eng.fdesc), K_NB, ptr(a["rank"]), nr, ptr(a["frames"]), a["frame_dim"],
                                       a["steps"], a["col"], None, a["lr"], 1, None, ptr(a["ws"]), a["ws_bytes"], s)
    for kw in (dict(obs=None), dict(frames=None), dict(rank=None), dict(ws=None)):
        assert call(**kw) == -1 and err() == "gm_train_rollout_step: null pointer", kw
    for steps in (0, -3):
        assert call(steps=steps) == -1 and err().startswith("gm_train_rollout_step: steps=%d outside" % steps)
    for frame_dim in (4, 6, 9):
        assert call(frame_dim=frame_dim) == -1 and err().startswith("gm_train_rollout_step: frame_dim=%d is neither" % frame_dim)
    assert call(col=L0.D) == -1 and err() == "gm_train_rollout_step: material_col=%d outside the %d state columns" % (L0.D, L0.D)
    assert call(lr=NAN) == -1 and err() == "gm_train_rollout_step: lr is NaN"
    assert call(ws_bytes=need - 1) == -4 and err() == "gm_train_rollout_step: workspace %d < %d" % (need - 1, need)
    _same_state(_state(t), before, "refusals")                        # nothing above reached the device
    assert t.record() == dict(steps_applied=0, steps_skipped=0, beta1_pow=1.0, beta2_pow=1.0)


# ------------------------------------------------------------------------------------------ 7. and 8. the dataset
@pytest.fixture(scope="module")
def g9_root(golden, tmp_path_factory):
    """The synthetic recordings of tests/golden/g9_dataset.npz as a dataset directory."""
    g = golden("g9_dataset.npz")
    root = str(tmp_path_factory.mktemp("g9_train_rollout")) + "/"
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")
    return root


def test_rollout_sample_is_the_datasets_window_and_the_recordings_frames(dev, g9_root):
    from gnn_manip_amd import CoffeeDataset
    from gnn_manip_amd.graph import _node_features
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", device=dev, use_control=True)
    assert len(ds) == 6 and ds.sims[0].shape == (9, 60, 5)
    for idx, steps in ((0, 3), (1, 2), (2, 1), (3, 3), (5, 1)):
        window, frames = ds.rollout_sample(idx, steps)
        s, f = ds.index[idx]
        assert same_bits(window, ds.sample(idx)[0]), idx
        assert frames.shape == (steps, 60, 5) and frames.data_ptr() == ds.sims[s][f + 6].data_ptr() and frames.is_contiguous()
        assert same_bits(frames, ds.sims[s][f + 6:f + 6 + steps])
    for idx, steps in ((1, 3), (2, 2), (5, 2), (0, 0), (6, 1), (-1, 1)):
        with pytest.raises(IndexError):
            ds.rollout_sample(idx, steps)
    plain = CoffeeDataset(g9_root, 6, 0.015, split="train", device=dev)               # no control columns: the recording's own
    window, frames = plain.rollout_sample(3, 2)
    assert window.shape == (6, 60, 5) and same_bits(window, plain.sample(3)[0]) and frames.shape == (2, 60, 5)
    # with noise: the draw of batch([idx], seed, stream)
    noisy = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    for idx, seed, stream in ((0, 0, 0), (4, 7, 3)):
        window, frames = noisy.rollout_sample(idx, 1, seed=seed, stream=stream)
        batch = noisy.batch([idx], seed, stream)
        assert same_bits(_node_features(window, noisy._window_desc()), batch.x), (idx, seed, stream)
        clean = noisy.sample(idx)[0]
        assert not same_bits(window[:, :, 2:5], clean[:, :, 2:5]) and same_bits(window[0], clean[0])      # the walk starts at zero
        assert same_bits(window[:, :, 5:], clean[:, :, 5:]) and same_bits(window[:, :, :2], clean[:, :, :2])   # control: the clean positions'
        again, _ = noisy.rollout_sample(idx, 1, seed=seed, stream=stream)
        other, _ = noisy.rollout_sample(idx, 1, seed=seed, stream=stream + 1)
        assert same_bits(again, window) and not same_bits(other, window)


def test_fit_rollout_epoch_is_step_by_step(dev, g9_root):
    from gnn_manip_amd import CoffeeDataset, RolloutEngine, Trainer
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    dims = (25, 4, 3, 64, 2, 2)
    params = orc.init_params(*dims, 309)
    scale = [float(v) for v in ds.stats["acceleration_std"]]

    def fresh():
        m = load_model(params, dims, dev)
        return Trainer(m, lr=LR, sand_only=True, material_col=sc.MATERIAL_COL), RolloutEngine(m, ds.graph_attr, 60, k_steps=6, data_dim=8, device=dev)

    for steps, starts in ((1, None), (2, None), (2, [0, 1, 4])):
        want_starts = trc.non_overlapping_starts([9, 9], 6, steps) if starts is None else starts
        by_step, eng = fresh()
        slots = torch.zeros(len(want_starts), dtype=torch.float64, device=dev)
        for i, start in enumerate(want_starts):
            window, frames = ds.rollout_sample(start, steps, seed=5, stream=start)
            eng.set_scene(window)
            by_step.step_rollout(eng, window, frames, steps, pos_scale=scale, loss_out=slots[i:i + 1])
        want = slots.cpu().numpy()
        assert len(want) == {1: 6, 2: 2}[steps] if starts is None else 3
        t, eng = fresh()
        got = t.fit_rollout_epoch(ds, eng, steps, starts=starts, seed=5, pos_scale=scale)
        print(f"\n[train rollout] fit_rollout_epoch steps={steps} starts={want_starts}: {got}")
        assert got.dtype == np.float64 and np.isfinite(got).all() and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
        _same_state(_state(t), _state(by_step), ("fit_rollout_epoch", steps, starts))
        assert t.record()["steps_applied"] == len(want_starts)
