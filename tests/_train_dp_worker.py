"""Rank program of the two spawned tests of tests/test_gpu_train_dp.py: ``_train_dp_worker.py MODE DATASET_ROOT OUT_DIR`` under
torch.distributed's environment rendezvous, every rank on cuda:0.

MODE gloo2: two ranks on gloo (RCCL refuses two ranks per device; the sharding, the contribution and the reduce are the same), the
payload staged through the host.  fit_rollout_epoch(batch_size=3) and fit_epoch(accumulate=2) over recordings of two sizes, then a
mini-batch in which rank 1's sample fails on the host.  Every rank writes its state to OUT_DIR/rank<r>.npz.

MODE rccl1: one rank on RCCL, the payload on the device: fit_epoch(accumulate=2) of a distributed trainer against the same epoch of
a trainer that is not, with the synchronisations of the distributed epoch counted."""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import train_dp_cases as dp   # noqa: E402


def gloo2(root, out_dir, dev):
    from gnn_manip_amd import GraphLoader
    from gnn_manip_amd._lib import GMError
    rank, world = dist.get_rank(), dist.get_world_size()
    ds, two = dp.epoch_datasets(root, dev)
    t, engines = dp.epoch_trainer(two, dev)
    assert t.distribute(collective_device="cpu") is t
    scale = [float(v) for v in two.stats["acceleration_std"]]
    out = {}
    out["rollout_losses"] = t.fit_rollout_epoch(two, engines, 1, starts=list(dp.ROLLOUT_STARTS), seed=dp.ROLLOUT_SEED, pos_scale=scale,
                                                batch_size=dp.ROLLOUT_BATCH)
    out["rollout_norms"] = t.last_epoch_grad_norms
    loader = GraphLoader(ds, batch_size=dp.LOADER_BATCH, seed=dp.LOADER_SEED, fused=True, prefetch=1, shard=(rank, world, dp.LOADER_ACCUMULATE))
    out["loader_losses"] = t.fit_epoch(loader, accumulate=dp.LOADER_ACCUMULATE)
    out["loader_norms"] = t.last_epoch_grad_norms
    out["in_step"] = np.array([t.replicas_in_step()])
    out.update(dp.state_arrays(t))
    # a mini-batch of two samples, one per rank; rank 1's is refused by the library on the host
    batch = next(iter(GraphLoader(ds, batch_size=dp.LOADER_BATCH, seed=dp.LOADER_SEED, fused=True, prefetch=0)))
    t.zero_grad()
    mask_col = t.mask_col
    if rank == 1:
        t.mask_col = 10 ** 6                              # no such node column: gm_train_step_accumulate refuses the sample
    t.accumulate(batch)                                   # rank 1: the error is kept, nothing is raised yet
    t.mask_col = mask_col
    raised = ""
    try:
        t.apply(samples_total=2)                          # every rank exchanges; rank 1 raises behind the exchange
    except GMError as error:
        raised = str(error)
    out["raised"] = np.array([raised])
    after = dp.state_arrays(t)
    out["after_counters"] = after["counters"]
    out["untouched"] = np.array([all(np.array_equal(after[k].view(np.uint32), out[k].view(np.uint32)) for k in after if k != "counters")])
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **out)


def rccl1(root, out_dir, dev):
    from gnn_manip_amd import GraphLoader
    ds, two = dp.epoch_datasets(root, dev)
    make = lambda shard: GraphLoader(ds, batch_size=dp.LOADER_BATCH, seed=dp.LOADER_SEED, fused=True, prefetch=1, shard=shard)
    plain, _ = dp.epoch_trainer(two, dev)
    want = plain.fit_epoch(make(None), accumulate=dp.LOADER_ACCUMULATE)
    want_norms = plain.last_epoch_grad_norms
    t, _ = dp.epoch_trainer(two, dev)
    t.distribute()
    loader = make((0, 1, dp.LOADER_ACCUMULATE))
    calls = []

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped

    saved = torch.cuda.synchronize, torch.cuda.Stream.synchronize
    torch.cuda.synchronize = spy("torch.cuda.synchronize", saved[0])
    torch.cuda.Stream.synchronize = spy("Stream.synchronize", saved[1])
    try:
        got = t.fit_epoch(loader, accumulate=dp.LOADER_ACCUMULATE)
    finally:
        torch.cuda.synchronize, torch.cuda.Stream.synchronize = saved
    a, b = dp.state_arrays(t), dp.state_arrays(plain)
    same = all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a) and sorted(a) == sorted(b)
    bits = lambda x: np.asarray(x, np.float64).view(np.uint64).tolist()
    with open(os.path.join(out_dir, "rccl1.json"), "w") as fp:
        json.dump({"calls": calls, "same_state": bool(same), "losses": bits(got), "want": bits(want), "norms": bits(t.last_epoch_grad_norms),
                   "want_norms": bits(want_norms), "in_step": bool(t.replicas_in_step()), "counters": a["counters"].tolist(),
                   "backend": dist.get_backend()}, fp)


def main():
    mode, root, out_dir = sys.argv[1:4]
    dist.init_process_group({"gloo2": "gloo", "rccl1": "nccl"}[mode])
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    {"gloo2": gloo2, "rccl1": rccl1}[mode](root, out_dir, dev)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
