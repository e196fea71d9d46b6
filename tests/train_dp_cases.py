"""Cases and numpy restatements of data-parallel training in the library (csrc/train_step.hip: gm_rank_sum,
gm_trainer_contribution, gm_trainer_reduce; gnn_manip_amd/train.py: Trainer.contribution / reduce / distribute, exchange_bytes;
gnn_manip_amd/dataset.py: owned_positions, GraphLoader(shard=); the contract is in include/gnn_manip_hip.h) -- a plain helper
module (no test) of tests/test_train_dp_cases.py (CPU), tests/test_abi_train_dp.py and tests/test_gpu_train_dp.py (the kernels
against the restatements, bit for bit).

gm_rank_sum:  dst = ((row 0 + row 1) + row 2) + ..., float32 adds rounded one by one, in rank order.  gm_trainer_reduce merges the
ranks' 32-byte tails {samples, bad, loss_sum, steps_applied} into the mini-batch record: integer sums, loss_sum in float64 in rank
order from rank 0's value, bad + 1 for unequal steps_applied, bad + 1 for a sample count other than the caller's.

NaN: IEEE 754 leaves the sign and payload of a NaN that an add produces or passes on to the implementation, and numpy on the host
and the MI355X differ there (inf - inf).  The restatement is therefore compared bit for bit wherever it is not NaN, and as NaN
where it is (same_bits_or_nan)."""
import numpy as np

import train_accum_cases as ac

RANK_SUM_COUNTS = ac.SUMSQ_COUNTS         # around one workgroup and its 16-byte groups, tails of 1..3, past 128 x 256 x 4 elements
RANK_SUM_WORLDS = (1, 2, 3, 8)            # a copy, one add, and rank loops of an odd and an even length
TAIL_BYTES = 32

# 1e30f - 1e30f + 1f: the three rank orders and what a float32 sum IN THAT ORDER gives.  Another order gives another value.
TRIPLE_ORDERS = (((1e30, -1e30, 1.0), 1.0), ((1e30, 1.0, -1e30), 0.0), ((1.0, 1e30, -1e30), 0.0))


def rank_sum_restated(rows):
    """[world, count] float32 -> [count] float32: the rows added one after the other, each add rounded to float32."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2
    total = rows[0].copy()
    with np.errstate(all="ignore"):
        for r in range(1, rows.shape[0]):
            total = total + rows[r]
            assert total.dtype == np.float32
    return total


def same_bits_or_nan(got, want):
    """got equals the restatement `want` bit for bit where want is a number, and is NaN where want is NaN."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]) and bool(np.isnan(got[nan]).all())


def rank_sum_case(world, count, stride, seed=0):
    """[world, stride] float32: magnitudes over twelve decades and both signs, so that the order of the adds shows in the bits;
    the columns past `count` hold a sentinel that must never reach the result."""
    rng = np.random.default_rng([seed, world, count])
    rows = (rng.standard_normal((world, stride)) * 10.0 ** rng.integers(-6, 7, (world, stride))).astype(np.float32)
    rows[:, count:] = 7e37
    return rows


def merge_restated(tails, samples_total):
    """The mini-batch record gm_trainer_reduce leaves, from the ranks' tails [(samples, bad, loss_sum, steps_applied), ...]:
    {'samples', 'bad', 'loss_sum'} -- sumsq, grad_norm and scale are gm_trainer_begin's 0.0, NaN, NaN."""
    samples = sum(int(t[0]) for t in tails)
    bad = sum(int(t[1]) for t in tails)
    loss_sum = float(tails[0][2])
    for t in tails[1:]:
        loss_sum = loss_sum + float(t[2])
    if len({int(t[3]) for t in tails}) != 1:
        bad += 1
    if samples != int(samples_total):
        bad += 1
    return {"samples": samples, "bad": bad, "loss_sum": loss_sum}


def split_contribution(raw):
    """A contribution's bytes (a uint8 array) as (its float32 gradient part, (samples, bad, loss_sum, steps_applied))."""
    raw = np.ascontiguousarray(raw, np.uint8)
    assert raw.size % 16 == 0 and raw.size > TAIL_BYTES
    tail = raw[-TAIL_BYTES:]
    ints, loss = tail.view(np.int64), tail.view(np.float64)
    return raw[:-TAIL_BYTES].view(np.float32), (int(ints[0]), int(ints[1]), float(loss[2]), int(ints[3]))


def pack_contribution(grad, tail):
    """The other direction: a float32 gradient part (a multiple of four elements) and a tail as a contribution's bytes."""
    grad = np.ascontiguousarray(grad, np.float32)
    assert grad.size % 4 == 0
    t = np.zeros(4, np.int64)
    t[0], t[1], t[3] = tail[0], tail[1], tail[3]
    t[2:3].view(np.float64)[0] = tail[2]
    return np.concatenate((grad.view(np.uint8), t.view(np.uint8)))


# ---------------------------------------------------------------------------------------------- the epochs of the spawned ranks
# tests/_train_dp_worker.py (two processes) and tests/test_gpu_train_dp.py (two virtual ranks in one process) run the same thing:
EPOCH_DIMS, EPOCH_PARAM_SEED, EPOCH_LR = (25, 4, 3, 64, 2, 2), 309, 1e-3
ROLLOUT_STARTS, ROLLOUT_BATCH, ROLLOUT_SEED = (0, 1, 2, 3, 4), 3, 5      # three windows of 60 nodes, two of 48: mini-batches of 3 and 2
LOADER_BATCH, LOADER_SEED, LOADER_ACCUMULATE = 2, 2, 2                   # three batches: mini-batches of 2 and 1 (rank 1 owns none of it)
EPOCH_CLIP = 0.05


def write_g9_root(g, root):
    """The synthetic recordings of tests/golden/g9_dataset.npz (`g`) as a dataset directory `root` (ends with a slash)."""
    import os
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")


def epoch_datasets(root, dev):
    """(the two recordings as they are: for GraphLoader; the second without its first twelve rows, 60 and 48 nodes: for rollouts)."""
    from gnn_manip_amd import CoffeeDataset
    ds = CoffeeDataset(root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    sims = [ds.sims[0], ds.sims[1][:, 12:].contiguous()]
    two = CoffeeDataset.from_recordings(sims, 6, 0.015, ds.stats, ds.bounds, ds.cartesian_idx, ds.material_id, ds.control_idx, noise=3e-4,
                                        use_control=True)
    return ds, two


def epoch_trainer(two, dev):
    """(a trainer on EPOCH_DIMS with the clip EPOCH_CLIP, {node count: its RolloutEngine})."""
    import train_step_cases as sc
    from gpu_support import load_model
    from gnn_manip_amd import RolloutEngine, Trainer
    from oracle import epd_oracle as orc
    m = load_model(orc.init_params(*EPOCH_DIMS, EPOCH_PARAM_SEED), EPOCH_DIMS, dev)
    engines = {n: RolloutEngine(m, two.graph_attr, n, k_steps=6, data_dim=8, device=dev) for n in (60, 48)}
    t = Trainer(m, lr=EPOCH_LR, sand_only=True, material_col=sc.MATERIAL_COL)
    t.max_grad_norm = EPOCH_CLIP
    return t, engines


def state_arrays(t):
    """{name: numpy array} of a trainer's weights and moments, and its record's two counters."""
    from gnn_manip_amd import train
    out = {}
    for kind, what in (("w", train.PARAMS), ("m", train.EXP_AVG), ("v", train.EXP_AVG_SQ)):
        for i, a in enumerate(t.export(what)):
            out[f"{kind}{i}"] = a.cpu().numpy()
    rec = t.record()
    out["counters"] = np.array([rec["steps_applied"], rec["steps_skipped"]], np.int64)
    return out


# ---------------------------------------------------------------------------------------------- sharding
SHARD_CASES = tuple((n, world, group) for n in (0, 1, 5, 6, 7, 13) for world in (1, 2, 3, 8) for group in (1, 2, 3, 5))


def owned_restated(n_items, rank, world, group):
    """Position p belongs to group p // group, at place p % group of its len_g places; place q belongs to the rank r with
    r * base + min(r, rem) <= q < ..., base, rem = divmod(len_g, world): planner.shard_range's blocks, written out per item."""
    owned = []
    for p in range(n_items):
        first = (p // group) * group
        length = min(group, n_items - first)
        base, rem = divmod(length, world)
        q, owner, lo = p - first, None, 0
        for r in range(world):
            hi = lo + base + (1 if r < rem else 0)
            if lo <= q < hi:
                owner = r
            lo = hi
        if owner == rank:
            owned.append(p)
    return owned
