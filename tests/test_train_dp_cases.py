"""CPU: the restatements and the host side of data-parallel training (tests/train_dp_cases.py): the rank-ordered float32 sum and
the record merge, the sharding of mini-batches over ranks (dataset.owned_positions, GraphLoader(shard=)) and the byte exchange
(train.exchange_bytes) over two gloo ranks."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import train_dp_cases as dp


# ------------------------------------------------------------------------------------------ the restatements
def test_rank_sum_restated_adds_in_rank_order_in_float32():
    for values, want in dp.TRIPLE_ORDERS:
        rows = np.array(values, np.float32).reshape(3, 1)
        got = dp.rank_sum_restated(rows)
        assert got.dtype == np.float32 and got.shape == (1,) and float(got[0]) == want, (values, got)
    assert sorted(w for _, w in dp.TRIPLE_ORDERS) == [0.0, 0.0, 1.0]           # the order decides
    # one rank: the bits, a NaN's payload and the sign of a zero included
    odd = np.array([0x7fc12345, 0x80000000, 0x00000001, 0xff800000], np.uint32).view(np.float32).reshape(1, 4)
    assert np.array_equal(dp.rank_sum_restated(odd).view(np.uint32), odd.view(np.uint32)[0])
    # float32 rounding after every add: 2^24 + 1 + 1 stays 2^24 in float32, while float64 reaches 2^24 + 2
    rows = np.array([[2.0 ** 24], [1.0], [1.0]], np.float32)
    assert float(dp.rank_sum_restated(rows)[0]) == 2.0 ** 24 and float(rows.astype(np.float64).sum()) == 2.0 ** 24 + 2
    # against a scalar loop
    rows = dp.rank_sum_case(8, 37, 40)
    want = []
    for i in range(37):
        total = rows[0, i]
        for r in range(1, 8):
            total = np.float32(total + rows[r, i])
        want.append(total)
    assert np.array_equal(dp.rank_sum_restated(rows[:, :37]).view(np.uint32), np.array(want, np.float32).view(np.uint32))
    assert dp.same_bits_or_nan(np.array([np.nan, 1.0], np.float32), np.array([-np.nan, 1.0], np.float32))
    assert not dp.same_bits_or_nan(np.array([0.0, 1.0], np.float32), np.array([-0.0, 1.0], np.float32))
    assert not dp.same_bits_or_nan(np.array([2.0, 1.0], np.float32), np.array([np.nan, 1.0], np.float32))


def test_merge_restated_sums_in_rank_order_and_counts_disagreements():
    tails = [(2, 0, 1e16, 5), (1, 0, -1e16, 5), (0, 0, 1.0, 5)]
    assert dp.merge_restated(tails, 3) == {"samples": 3, "bad": 0, "loss_sum": 1.0}
    assert dp.merge_restated(tails[::-1], 3)["loss_sum"] == 0.0                 # (1 - 1e16) + 1e16 in float64: the order decides
    assert dp.merge_restated(tails, 4)["bad"] == 1                              # not the caller's sample count
    assert dp.merge_restated([(2, 0, 0.5, 5), (1, 0, 0.5, 6)], 3)["bad"] == 1   # replicas out of step
    assert dp.merge_restated([(2, 0, 0.5, 5), (1, 0, 0.5, 6)], 2)["bad"] == 2   # both
    assert dp.merge_restated([(2, 1, 0.5, 5), (0, 1, 0.0, 5)], 2) == {"samples": 2, "bad": 2, "loss_sum": 0.5}   # a poisoned peer
    assert dp.merge_restated([(3, 0, 0.25, 0)], 3) == {"samples": 3, "bad": 0, "loss_sum": 0.25}
    grad = np.arange(8, dtype=np.float32)
    raw = dp.pack_contribution(grad, (3, 1, 0.125, 9))
    assert raw.dtype == np.uint8 and raw.size == 32 + dp.TAIL_BYTES
    g, tail = dp.split_contribution(raw)
    assert np.array_equal(g, grad) and tail == (3, 1, 0.125, 9)


# ------------------------------------------------------------------------------------------ sharding
@pytest.mark.parametrize("n,world,group", dp.SHARD_CASES)
def test_every_item_is_owned_exactly_once(n, world, group):
    from gnn_manip_amd.dataset import owned_positions
    from gnn_manip_amd.planner import shard_range
    blocks = [owned_positions(n, (rank, world, group)) for rank in range(world)]
    assert sorted(p for b in blocks for p in b) == list(range(n))
    for rank, block in enumerate(blocks):
        assert block == sorted(block) == dp.owned_restated(n, rank, world, group)
        for first in range(0, n, group):                                        # contiguous inside every group: shard_range's block
            lo, hi = shard_range(min(group, n - first), world, rank)
            assert [p for p in block if first <= p < first + group] == list(range(first + lo, first + hi))
    assert owned_positions(n, None) == list(range(n))


def test_a_short_last_group_leaves_ranks_empty():
    from gnn_manip_amd.dataset import owned_positions
    # 7 items in groups of 3 over 3 ranks: the last group is one item, rank 0's
    assert [owned_positions(7, (r, 3, 3)) for r in range(3)] == [[0, 3, 6], [1, 4], [2, 5]]
    # 5 items in groups of 4 over 8 ranks: ranks 4..7 never own anything, ranks 1..3 nothing of the last group
    assert [owned_positions(5, (r, 8, 4)) for r in range(8)] == [[0, 4], [1], [2], [3], [], [], [], []]


class _Samples:
    device = torch.device("cpu")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


@pytest.mark.parametrize("shuffle", [False, True])
def test_graph_loader_shard_yields_the_unsharded_loaders_owned_batches(monkeypatch, shuffle):
    """The fused path with its build replaced by a recorder: the sample indices and the first noise stream of every batch."""
    from gnn_manip_amd import dataset as dsm

    class Recorded:
        def __init__(self, dataset, indices, seed, first_stream, workspaces, pinned):
            self.what = (tuple(indices), seed, first_stream)

        def finish(self):
            return self.what

    monkeypatch.setattr(dsm, "_QueuedBatch", Recorded)
    monkeypatch.setattr(dsm, "_pinned_records", lambda rows: torch.zeros((max(int(rows), 1), 4), dtype=torch.int32))
    n, bs, group = 23, 3, 3                                                     # 8 batches, the last of two samples; groups of 3, 3, 2
    make = lambda **kw: dsm.GraphLoader(_Samples(n), batch_size=bs, shuffle=shuffle, seed=4, fused=True, **kw)
    for prefetch in (0, 1):
        full = make(prefetch=prefetch)
        assert full.shard is None and len(full) == full.batches_in_all == 8 and full.owned_batches() == list(range(8))
        epochs = [list(full), list(full)]                                       # the second epoch goes on in the streams
        assert [b[2] for b in epochs[0]] == [3 * j for j in range(8)] and [b[2] for b in epochs[1]] == [23 + 3 * j for j in range(8)]
        assert sorted(i for b in epochs[0] for i in b[0]) == list(range(n))
        for world in (1, 2, 3):
            seen = []
            for rank in range(world):
                part = make(prefetch=prefetch, shard=(rank, world, group))
                owned = dsm.owned_positions(8, (rank, world, group))
                assert part.owned_batches() == owned and len(part) == len(owned) and part.batches_in_all == 8
                for epoch in epochs:
                    assert list(part) == [epoch[j] for j in owned], (world, rank)
                seen += owned
            assert sorted(seen) == list(range(8))
    with pytest.raises(ValueError, match="shard"):
        make(shard=(2, 2, 3))
    # without the fused build: the same owned batches, sample by sample
    monkeypatch.setattr(dsm, "collate_graphs", lambda samples: tuple(samples))
    plain = list(dsm.GraphLoader(_Samples(n), batch_size=bs))
    part = dsm.GraphLoader(_Samples(n), batch_size=bs, shard=(1, 2, group))
    assert list(part) == [plain[j] for j in part.owned_batches()] and part.owned_batches() == [2, 5, 7]


# ------------------------------------------------------------------------------------------ the exchange
def _payload(rank, nbytes):
    return torch.from_numpy(np.random.default_rng([9, rank]).integers(0, 256, nbytes, dtype=np.uint8))


def _exchange_worker(rank, world, port, q):
    import torch.distributed as dist
    from gnn_manip_amd.train import exchange_bytes
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = []
    for nbytes in (16, 48, 4112):
        local = _payload(rank, nbytes)
        gathered = torch.full((world, nbytes), 0xAB, dtype=torch.uint8)
        assert exchange_bytes(local, gathered) is gathered                    # host tensors: gloo's all_gather
        staged = torch.full((world, nbytes), 0xCD, dtype=torch.uint8)
        staging = (torch.empty(nbytes, dtype=torch.uint8), torch.empty((world, nbytes), dtype=torch.uint8))
        exchange_bytes(local, staged, staging=staging)                        # the staged path, with plain host buffers
        out.append((gathered.numpy().copy(), staged.numpy().copy(), local.numpy().copy()))
    q.put((rank, out))
    dist.barrier()
    dist.destroy_process_group()


def test_exchange_bytes_over_two_gloo_ranks():
    world = 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_exchange_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for k, nbytes in enumerate((16, 48, 4112)):
        want = np.stack([_payload(r, nbytes).numpy() for r in range(world)])
        for rank in range(world):
            gathered, staged, local = got[rank][k]
            assert np.array_equal(gathered, want) and np.array_equal(staged, want), (rank, nbytes)   # rank order, on every rank
            assert np.array_equal(local, want[rank])                                                  # the payload is not written
