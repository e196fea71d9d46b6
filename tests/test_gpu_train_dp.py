"""Data-parallel training on the MI355X (csrc/train_step.hip: gm_rank_sum, gm_trainer_contribution, gm_trainer_reduce;
gnn_manip_amd/train.py: Trainer.contribution / reduce / distribute / replicas_in_step, apply(samples_total=), the sharded epochs;
gnn_manip_amd/dataset.py: GraphLoader(shard=)).

Bounds.  No new tolerance.  gm_rank_sum, the merged gradients, the merged record and the updates: bit equality with the numpy
restatements of tests/train_dp_cases.py and tests/train_accum_cases.py, and between ranks (a NaN the restatement holds must be a
NaN: IEEE 754 does not fix its payload, see train_dp_cases).  The one accuracy claim, the merged gradient against the float64
oracle's summed gradient, is the rule of tests/yardstick.py with the ReLU flip allowance: the bar of the single-process mini-batch.

Several ranks run in ONE process as several trainers built from the same weights ("virtual ranks"): each accumulates its block,
the contributions are stacked in rank order, every trainer reduces the same stack.  Two tests start real rank processes
(tests/_train_dp_worker.py): two gloo ranks on this GPU, and one rank on RCCL with the payload on the device.  More than one rank on
RCCL needs more than one GPU and is not tested here."""
import json
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
import grad_cases as gc
import train_accum_cases as ac
import train_dp_cases as dp
import train_rollout_cases as trc
import train_step_cases as sc
from gpu_support import dev, load_model, rank_sum as _rank_sum, step_engine, to_dev
from grad_cases import L0
from yardstick import compare, same_bits

pytestmark = pytest.mark.gpu

LR = ac.LR
NAN = float("nan")
T = 3


# ------------------------------------------------------------------------------------------ helpers
def _trainer(dev, max_grad_norm=None):
    from gnn_manip_amd import Trainer
    m = load_model(ac.params(), ac.DIMS, dev)
    t = Trainer(m, lr=LR)
    t.max_grad_norm = max_grad_norm
    return t, m


def _batch(i, dev):
    return tuple(to_dev(a, dev) for a in ac.sample(i))


def _state(t):
    from gnn_manip_amd import train
    return [t.export(w) for w in (train.PARAMS, train.EXP_AVG, train.EXP_AVG_SQ)]


def _same_state(a, b, what):
    for kind, ta, tb in zip(("weights", "exp_avg", "exp_avg_sq"), a, b):
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert same_bits(u, v), (what, kind, i)


def _grads(t):
    from gnn_manip_amd import train
    return [g.cpu().numpy() for g in t.export(train.GRADS)]


def _bits64(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, np.float64)
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _record_bits(rec):
    return {k: (v if isinstance(v, int) else int(_bits64(np.float64(v).reshape(1))[0])) for k, v in rec.items()}


def _exchange(trainers, samples_total, poisoned=()):
    """The virtual ranks' exchange: every trainer's contribution, stacked in rank order, reduced by every trainer.  Returns the
    stack as numpy bytes."""
    gathered = torch.stack([t.contribution(poisoned=r in poisoned) for r, t in enumerate(trainers)])
    for t in trainers:
        t.reduce(gathered, samples_total)
    return gathered.cpu().numpy()


def _rollout_setup(dev, max_grad_norm=None):
    from gnn_manip_amd import Trainer
    dims = (25, 4, 3, 64, 2, 2)
    m = load_model(orc.init_params(*dims, 845 + 64), dims, dev)
    eng = step_engine(m, dev)
    obs_np = gc.step_state("step_a")
    obs, frames = to_dev(obs_np, dev), to_dev(trc.step_frames("step_a")[:T], dev)
    assert eng.set_scene(obs) == len(gc.rigid_rows(obs_np, L0)) > 0
    t = Trainer(m, lr=LR)
    t.max_grad_norm = max_grad_norm
    return t, eng, obs, frames


# ------------------------------------------------------------------------------------------ 1. gm_rank_sum
@pytest.mark.parametrize("count", dp.RANK_SUM_COUNTS)
def test_rank_sum_is_the_restated_sum(dev, count):
    for world in dp.RANK_SUM_WORLDS:
        for stride in ((count + 3) // 4 * 4, (count + 3) // 4 * 4 + 12):       # the tightest stride, and one past the count
            rows = dp.rank_sum_case(world, count, stride)
            want = dp.rank_sum_restated(rows[:, :count])
            got, again = _rank_sum(rows, count, dev), _rank_sum(rows, count, dev, fill=1e30)
            assert np.isfinite(want).all() and np.abs(want).max() < 1e30         # the sentinel columns past `count` stayed out
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (count, world, stride, int((got != want).sum()))
            assert np.array_equal(again.view(np.uint32), want.view(np.uint32)), "the destination's old contents showed"
            if world == 1:
                assert np.array_equal(got.view(np.uint32), rows[0, :count].view(np.uint32))
        if count >= 255:                                                        # the order shows: the reversed ranks give other bits
            rows = dp.rank_sum_case(3, count, (count + 3) // 4 * 4)
            assert not np.array_equal(dp.rank_sum_restated(rows[::-1, :count]).view(np.uint32), dp.rank_sum_restated(rows[:, :count]).view(np.uint32))


def test_rank_sum_adds_in_rank_order_and_passes_non_finite_values_on(dev):
    for count in (1, 5, 1029):                                                # the tail alone; a group and a tail; many workgroups' worth
        for values, want in dp.TRIPLE_ORDERS:
            rows = np.repeat(np.array(values, np.float32).reshape(3, 1), (count + 3) // 4 * 4, axis=1)
            got = _rank_sum(rows, count, dev)
            assert np.array_equal(got, np.full(count, want, np.float32)), (count, values, got[:4])
            assert np.array_equal(got.view(np.uint32), dp.rank_sum_restated(rows[:, :count]).view(np.uint32))
    count = 1029                                                              # 257 groups of four and a tail of one
    for world in (2, 3, 8):
        base = dp.rank_sum_case(world, count, 1032, seed=3)
        for where in (0, 515, 1027, 1028):
            for bad in (NAN, float("inf"), -float("inf")):
                for rank in (0, world - 1):
                    rows = base.copy()
                    rows[rank, where] = bad
                    want = dp.rank_sum_restated(rows[:, :count])
                    got = _rank_sum(rows, count, dev)
                    assert dp.same_bits_or_nan(got, want) and not np.isfinite(got[where]), (world, where, bad, rank)
                    assert int((~np.isfinite(got)).sum()) == 1
        rows = base.copy()
        rows[0, 7], rows[world - 1, 7] = float("inf"), -float("inf")            # inf - inf: a NaN is born
        got = _rank_sum(rows, count, dev)
        assert math.isnan(got[7]) and dp.same_bits_or_nan(got, dp.rank_sum_restated(rows[:, :count]))
    # one rank copies the bits: a NaN's payload, a negative zero, a denormal
    odd = np.array([0x7fc12345, 0x80000000, 0x00000001, 0xff800000, 0xffc00001], np.uint32).view(np.float32).reshape(1, 5)
    rows = np.zeros((1, 8), np.float32)
    rows[:, :5] = odd
    assert np.array_equal(_rank_sum(rows, 5, dev).view(np.uint32), odd.view(np.uint32)[0])


# ------------------------------------------------------------------------------------------ 2. one rank
def _same_record(t, twin, what):
    assert t.record() == twin.record(), what
    assert _record_bits(t.accum_record()) == _record_bits(twin.accum_record()), (what, t.accum_record(), twin.accum_record())


@pytest.mark.parametrize("clip", [None, ac.CLIP_ACTIVE])
def test_one_rank_is_the_plain_mini_batch(dev, clip):
    t, _ = _trainer(dev, clip)
    twin, _ = _trainer(dev, clip)
    got, want = torch.full((3,), 7.0, dtype=torch.float64, device=dev), torch.full((3,), 7.0, dtype=torch.float64, device=dev)
    for u, group in enumerate(([0], [1, 2], [2, 0, 1])):                    # one sample, then mini-batches of two and three
        batches = [_batch(i, dev) for i in group]
        for tr in (t, twin):
            tr.zero_grad()
            for b in batches:
                tr.accumulate(*b)
        before = _grads(t)
        own = t.contribution()
        assert own.dtype == torch.uint8 and own.numel() == t.contribution_bytes() and own.numel() % 16 == 0
        grad, tail = dp.split_contribution(own.cpu().numpy())
        rec = t.accum_record()
        assert tail == (len(group), 0, rec["loss_sum"], u) and rec["samples"] == len(group)
        t.reduce(own.view(1, -1), len(group))
        for a, b in zip(before, _grads(t)):
            assert same_bits(a, b), "one rank's reduce keeps the gradient's bits"
        _same_record(t, twin, ("before apply", u))
        t.apply(loss_out=got[u:u + 1])
        twin.apply(loss_out=want[u:u + 1])
        _same_state(_state(t), _state(twin), ("update", u, clip))
        _same_record(t, twin, ("after apply", u))
        assert float(t.last_grad_norm) == float(twin.last_grad_norm) or clip is None
    assert np.array_equal(_bits64(got), _bits64(want)) and np.isfinite(want.cpu().numpy()).all()
    assert t.record()["steps_applied"] == 3
    # the flat part of a contribution is the exported tensors, each on a 16-byte boundary with zeros between
    flat, off = grad, 0
    for g in before:
        assert np.array_equal(flat[off:off + g.size].view(np.uint32), g.reshape(-1).view(np.uint32))
        pad = (-g.size) % 4
        assert not flat[off + g.size:off + g.size + pad].any()
        off += g.size + pad
    assert off == flat.size
    t.status()


@pytest.mark.parametrize("clip", [None, 1e-3])
def test_one_rank_is_the_plain_rollout_mini_batch(dev, clip):
    t, eng, obs, frames = _rollout_setup(dev, clip)
    twin, eng2, _, _ = _rollout_setup(dev, clip)
    got, want = torch.full((2,), 7.0, dtype=torch.float64, device=dev), torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    for u in range(2):
        for tr, e in ((t, eng), (twin, eng2)):
            tr.zero_grad()
            tr.accumulate_rollout(e, obs, frames, pos_scale=trc.ACC_STD)
        t.reduce(t.contribution().view(1, -1), 1)
        _same_record(t, twin, ("rollout, before apply", u))
        t.apply(loss_out=got[u:u + 1])
        twin.apply(loss_out=want[u:u + 1])
        _same_state(_state(t), _state(twin), ("rollout update", u, clip))
        _same_record(t, twin, ("rollout, after apply", u))
    assert np.array_equal(_bits64(got), _bits64(want)) and np.isfinite(want.cpu().numpy()).all() and t.record()["steps_applied"] == 2


# ------------------------------------------------------------------------------------------ 3. virtual ranks
@pytest.mark.parametrize("world,clip", [(2, ac.CLIP_ACTIVE), (3, None)])
def test_virtual_ranks_sum_in_rank_order_and_update_alike(dev, world, clip):
    from gnn_manip_amd.planner import shard_range
    made = [_trainer(dev, clip) for _ in range(world)]
    trainers, m = [t for t, _ in made], made[0][1]
    names = [k for k, _ in m.named_parameters()]
    batches = [_batch(i, dev) for i in range(3)]
    blocks = [range(*shard_range(3, world, r)) for r in range(world)]
    assert sorted(i for b in blocks for i in b) == [0, 1, 2]
    w = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    state = sc.adam_state(w)
    for u in range(3):
        own = torch.full((3,), 7.0, dtype=torch.float64, device=dev)
        for t, block in zip(trainers, blocks):
            t.zero_grad()
            for i in block:
                t.accumulate(*batches[i], loss_out=own[i:i + 1])
        parts = [_grads(t) for t in trainers]
        _exchange(trainers, 3)
        merged = _grads(trainers[0])
        for k in range(len(merged)):
            want = dp.rank_sum_restated(np.stack([parts[r][k].reshape(-1) for r in range(world)])).reshape(merged[k].shape)
            assert np.array_equal(merged[k].view(np.uint32), want.view(np.uint32)), ("merged gradient", u, names[k])
        for t in trainers[1:]:
            for a, b in zip(merged, _grads(t)):
                assert same_bits(a, b)
        if u == 0:                                                              # the weights are the oracle's: its summed gradient
            ref_losses, r64 = ac.oracle_gradients()
            _, r32 = ac.oracle_gradients("float32")
            worst, worst2 = compare(dict(zip(names, merged)), r64, r32, ac.oracle_flip_allowance, what="merged gradients")
            print(f"\n[train dp] world {world}: worst tensor {worst[0]} err {worst[2]:.3e} tol {worst[3]:.3e}; with allowance {worst2}")
            np.testing.assert_allclose(own.cpu().numpy(), ref_losses, rtol=1e-5)
        slots = torch.full((world, 2), 7.0, dtype=torch.float64, device=dev)
        for r, t in enumerate(trainers):
            t.apply(loss_out=slots[r, 0:1], norm_out=slots[r, 1:2])
        losses = own.cpu().numpy()
        assert np.array_equal(_bits64(slots[:, 0]), np.repeat(_bits64(np.float64(ac.mean_loss(losses)).reshape(1)), world)), (u, slots, losses)
        recs = [t.accum_record() for t in trainers]
        assert all(_record_bits(r) == _record_bits(recs[0]) for r in recs) and (recs[0]["samples"], recs[0]["bad"]) == (3, 0)
        norm = ac.norm_of(merged, 3)
        assert abs(recs[0]["grad_norm"] - norm) <= 1e-12 * norm and np.array_equal(_bits64(slots[:, 1]), np.repeat(_bits64(np.float64(recs[0]["grad_norm"]).reshape(1)), world))
        assert recs[0]["scale"] == float(ac.scale_of(recs[0]["grad_norm"], 3, clip))
        w = ac.scaled_adam_restated(w, merged, state, LR, np.float32(recs[0]["scale"]))
        for t in trainers:
            _same_state(_state(t), (w, state["m"], state["v"]), ("restated update", u, world))
    for t in trainers:
        assert t.record() == trainers[0].record() and t.record()["steps_applied"] == 3 and t.record()["steps_skipped"] == 0
        t.status()


# ------------------------------------------------------------------------------------------ 4. skips and empty contributions
def test_a_rank_without_samples_contributes_zeros(dev):
    a, _ = _trainer(dev)
    b, _ = _trainer(dev)
    batch = _batch(0, dev)
    own = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
    a.zero_grad()
    a.accumulate(*batch, loss_out=own)
    b.zero_grad()                                                             # rank 1 owns nothing of this mini-batch
    part = _grads(a)
    raw = _exchange([a, b], 1)
    grad_b, tail_b = dp.split_contribution(raw[1])
    assert tail_b == (0, 0, 0.0, 0) and not grad_b.any()
    for k, (g, p) in enumerate(zip(_grads(b), part)):
        want = dp.rank_sum_restated(np.stack([p.reshape(-1), np.zeros(p.size, np.float32)])).reshape(p.shape)
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), k
    slots = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    a.apply(loss_out=slots[0:1])
    b.apply(loss_out=slots[1:2])
    _same_state(_state(a), _state(b), "a rank without samples")
    assert np.array_equal(_bits64(slots), np.repeat(_bits64(own), 2)) and math.isfinite(float(own))
    assert a.record() == b.record() == dict(steps_applied=1, steps_skipped=0, beta1_pow=0.9, beta2_pow=0.999)
    assert (b.accum_record()["samples"], b.accum_record()["bad"]) == (1, 0)


def _pair_after_one_update(dev, clip=ac.CLIP_ACTIVE):
    """Two virtual ranks after one shared mini-batch of samples 0 and 1."""
    pair = [_trainer(dev, clip)[0] for _ in range(2)]
    for r, t in enumerate(pair):
        t.zero_grad()
        t.accumulate(*_batch(r, dev))
    _exchange(pair, 2)
    for t in pair:
        t.apply()
    return pair


def test_a_poisoned_rank_skips_the_update_everywhere_and_leaves_no_trace(dev):
    pair, twins = _pair_after_one_update(dev), _pair_after_one_update(dev)
    before, rec0 = [_state(t) for t in pair], pair[0].record()
    assert rec0["steps_applied"] == 1
    pair[0].zero_grad()
    pair[0].accumulate(*_batch(2, dev))
    pair[1].zero_grad()                                                       # what Trainer.accumulate leaves behind a failed sample
    raw = _exchange(pair, 2, poisoned={1})
    grad, tail = dp.split_contribution(raw[1])
    assert tail == (0, 1, 0.0, 1) and not grad.any()
    slots = torch.full((2,), 7.0, dtype=torch.float64, device=dev)
    for r, t in enumerate(pair):
        t.apply(loss_out=slots[r:r + 1])
        _same_state(_state(t), before[r], ("poisoned", r))
        assert t.record() == dict(rec0, steps_skipped=1)
        rec = t.accum_record()
        assert (rec["samples"], rec["bad"]) == (1, 2)                         # the poisoned sample, and one sample short of the two
    assert np.isnan(slots.cpu().numpy()).all()
    for group in (pair, twins):                                               # the next mini-batch is the twins', who never saw it
        for r, t in enumerate(group):
            t.zero_grad()
            t.accumulate(*_batch(2 - r, dev))
        _exchange(group, 2)
        for t in group:
            t.apply()
    for t, twin in zip(pair, twins):
        _same_state(_state(t), _state(twin), "the next mini-batch")
        assert float(t.last_loss) == float(twin.last_loss) and float(t.last_grad_norm) == float(twin.last_grad_norm)
        assert twin.record() == dict(t.record(), steps_skipped=0) and t.record()["steps_applied"] == 2
        t.status()


def test_replicas_out_of_step_and_a_wrong_sample_count_skip_the_update(dev):
    pair = _pair_after_one_update(dev)
    pair[1].zero_grad()                                                       # rank 1 goes one update ahead on its own
    pair[1].accumulate(*_batch(2, dev))
    pair[1].apply()
    assert [t.record()["steps_applied"] for t in pair] == [1, 2]
    before = [_state(t) for t in pair]
    for r, t in enumerate(pair):
        t.zero_grad()
        t.accumulate(*_batch(r, dev))
    raw = _exchange(pair, 2)
    assert [dp.split_contribution(raw[r])[1][3] for r in range(2)] == [1, 2]
    for r, t in enumerate(pair):
        t.apply()
        rec = t.accum_record()
        assert (rec["samples"], rec["bad"]) == (2, 1) and math.isnan(float(t.last_loss))
        _same_state(_state(t), before[r], ("out of step", r))
        assert t.record()["steps_skipped"] == 1 and t.record()["steps_applied"] == 1 + r
    # a sample count that is not the sum of the ranks'
    pair = _pair_after_one_update(dev)
    before = [_state(t) for t in pair]
    for r, t in enumerate(pair):
        t.zero_grad()
        t.accumulate(*_batch(r, dev))
    raw = _exchange(pair, 3)
    tails = [dp.split_contribution(raw[r])[1] for r in range(2)]
    for r, t in enumerate(pair):
        rec = t.accum_record()
        want = dp.merge_restated(tails, 3)
        assert (rec["samples"], rec["bad"], rec["loss_sum"]) == (want["samples"], want["bad"], want["loss_sum"]) and want["bad"] == 1
        t.apply()
        _same_state(_state(t), before[r], ("wrong samples_total", r))
        assert t.record() == dict(steps_applied=1, steps_skipped=1, beta1_pow=0.9, beta2_pow=0.999)


def test_contribution_and_reduce_refusals(dev):
    from gnn_manip_amd._lib import GMError, current_stream, lib, ptr
    t, _ = _trainer(dev)
    L, s = lib(), current_stream(dev)
    err = lambda: L.gm_last_error().decode()
    need = t.contribution_bytes()
    buf = torch.full((2 * need + 16,), 0x5A, dtype=torch.uint8, device=dev)
    before = _state(t)
    no_batch = "no mini-batch begun (gm_trainer_begin)"
    assert L.gm_trainer_contribution(t._h, ptr(buf), need, 0, s) == -1 and err() == "gm_trainer_contribution: " + no_batch
    assert L.gm_trainer_reduce(t._h, ptr(buf), 1, need, 1, s) == -1 and err() == "gm_trainer_reduce: " + no_batch
    poisoned = t.contribution(poisoned=True)                                  # allowed without a mini-batch
    grad, tail = dp.split_contribution(poisoned.cpu().numpy())
    assert tail == (0, 1, 0.0, 0) and not grad.any()
    t.zero_grad()
    assert L.gm_trainer_contribution(t._h, None, need, 0, s) == -1 and err() == "gm_trainer_contribution: null pointer"
    assert L.gm_trainer_contribution(t._h, ptr(buf), need - 1, 1, s) == -1 and err() == "gm_trainer_contribution: out_bytes %d < %d" % (need - 1, need)
    assert L.gm_trainer_contribution(t._h, ptr(buf[4:]), need, 0, s) == -1 and err() == "gm_trainer_contribution: out_dev must lie on 16 bytes"
    assert L.gm_trainer_reduce(t._h, None, 1, need, 1, s) == -1 and err() == "gm_trainer_reduce: null pointer"
    for world in (0, 65):
        assert L.gm_trainer_reduce(t._h, ptr(buf), world, need, 1, s) == -1 and err() == "gm_trainer_reduce: world=%d outside 1..64" % world
    for stride in (need - 16, need + 8):
        assert L.gm_trainer_reduce(t._h, ptr(buf), 2, stride, 1, s) == -1
        assert err() == "gm_trainer_reduce: stride_bytes=%d below %d or no multiple of 16" % (stride, need)
    assert L.gm_trainer_reduce(t._h, ptr(buf[8:]), 2, need, 1, s) == -1 and err() == "gm_trainer_reduce: contributions_dev must lie on 16 bytes"
    assert L.gm_trainer_reduce(t._h, ptr(buf), 2, need, 0, s) == -1 and err() == "gm_trainer_reduce: samples_total_host=0 below 1"
    assert bool((buf == 0x5A).all())                                          # nothing above reached the device
    with pytest.raises(ValueError, match="samples_total"):
        t.apply(samples_total=2)                                              # not a distributed trainer
    with pytest.raises(ValueError, match="not distributed"):
        t.replicas_in_step()
    with pytest.raises(ValueError, match="uint8"):
        t.reduce(buf[:2 * need].view(2, need).float(), 1)
    with pytest.raises(GMError, match="no sample accumulated"):               # an empty mini-batch is still no update on its own
        t.apply()
    _same_state(_state(t), before, "refusals")
    assert t.record() == dict(steps_applied=0, steps_skipped=0, beta1_pow=1.0, beta2_pow=1.0)


# ------------------------------------------------------------------------------------------ 5. rank processes
@pytest.fixture(scope="module")
def g9_root(golden, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("g9_train_dp")) + "/"
    dp.write_g9_root(golden("g9_dataset.npz"), root)
    return root


def _run_ranks(mode, world, root, out_dir):
    """`world` fresh rank processes of tests/_train_dp_worker.py; their logs."""
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_train_dp_worker.py")
    procs = []
    for rank in range(world):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0")
        procs.append(subprocess.Popen([sys.executable, worker, mode, root, str(out_dir)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=300)
        except subprocess.TimeoutExpired:
            p.kill()
            o, _ = p.communicate()
        logs.append(o.decode(errors="replace"))
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)


def _virtual_epochs(root, dev, world):
    """The worker's two epochs on `world` virtual ranks in this process: (the trainers, rollout losses, loader losses)."""
    from gnn_manip_amd import GraphLoader
    from gnn_manip_amd.planner import shard_range
    ds, two = dp.epoch_datasets(root, dev)
    made = [dp.epoch_trainer(two, dev) for _ in range(world)]
    trainers = [t for t, _ in made]
    scale = [float(v) for v in two.stats["acceleration_std"]]

    def update(losses, norms):
        slots = torch.full((world, 2), 7.0, dtype=torch.float64, device=dev)
        for r, t in enumerate(trainers):
            t.apply(loss_out=slots[r, 0:1], norm_out=slots[r, 1:2])
        got = slots.cpu().numpy()
        assert all(np.array_equal(_bits64(got[r]), _bits64(got[0])) for r in range(world))
        losses.append(got[0, 0])
        norms.append(got[0, 1])

    rollout, loader = ([], []), ([], [])
    scenes = [None] * world
    starts = list(dp.ROLLOUT_STARTS)
    for first in range(0, len(starts), dp.ROLLOUT_BATCH):
        group = starts[first:first + dp.ROLLOUT_BATCH]
        for r, (t, engines) in enumerate(made):
            t.zero_grad()
            for start in group[slice(*shard_range(len(group), world, r))]:
                window, frames = two.rollout_sample(start, 1, seed=dp.ROLLOUT_SEED, stream=start)
                eng = engines[int(window.shape[1])]
                if scenes[r] != two.index[start][0]:
                    eng.set_scene(window)
                    scenes[r] = two.index[start][0]
                t.accumulate_rollout(eng, window, frames, 1, pos_scale=scale)
        _exchange(trainers, len(group))
        update(*rollout)
    batches = list(GraphLoader(ds, batch_size=dp.LOADER_BATCH, seed=dp.LOADER_SEED, fused=True, prefetch=0))
    assert len(batches) == 3
    for first in range(0, len(batches), dp.LOADER_ACCUMULATE):
        group = batches[first:first + dp.LOADER_ACCUMULATE]
        for r, t in enumerate(trainers):
            t.zero_grad()
            for batch in group[slice(*shard_range(len(group), world, r))]:
                t.accumulate(batch)
        _exchange(trainers, len(group))
        update(*loader)
    return trainers, [np.array(a) for a in rollout], [np.array(a) for a in loader]


def test_two_gloo_ranks_on_one_gpu_are_the_virtual_ranks(dev, g9_root, tmp_path):
    trainers, rollout, loader = _virtual_epochs(g9_root, dev, 2)
    want = dp.state_arrays(trainers[0])
    assert want["counters"].tolist() == [4, 0] and np.isfinite(rollout[0]).all() and np.isfinite(loader[0]).all()
    _run_ranks("gloo2", 2, g9_root, tmp_path)
    for rank in range(2):
        got = np.load(tmp_path / f"rank{rank}.npz")
        for k, v in want.items():
            assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), (rank, k)
        for name, (losses, norms) in (("rollout", rollout), ("loader", loader)):
            assert np.array_equal(_bits64(got[name + "_losses"]), _bits64(losses)), (rank, name, got[name + "_losses"], losses)
            assert np.array_equal(_bits64(got[name + "_norms"]), _bits64(norms)) and (norms > 0).all()
        assert bool(got["in_step"][0])
        # the mini-batch whose sample failed on rank 1: skipped on both ranks, raised on rank 1 alone, behind the exchange
        assert got["after_counters"].tolist() == [4, 1] and bool(got["untouched"][0])
        raised = str(got["raised"][0])
        assert ("mask_col" in raised and "gm_train_step_accumulate" in raised) if rank == 1 else raised == "", (rank, raised)


def test_one_rccl_rank_is_the_plain_epoch_with_one_synchronisation(dev, g9_root, tmp_path):
    _run_ranks("rccl1", 1, g9_root, tmp_path)
    got = json.load(open(tmp_path / "rccl1.json"))
    assert got["backend"] == "nccl" and got["calls"] == ["Stream.synchronize"], got["calls"]
    assert got["same_state"] and got["in_step"] and got["counters"] == [2, 0]
    assert got["losses"] == got["want"] and got["norms"] == got["want_norms"] and len(got["losses"]) == 2
