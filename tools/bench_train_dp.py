"""What data-parallel training adds to an update ON ONE GPU: Trainer.contribution + Trainer.reduce
(gm_trainer_contribution, gm_trainer_reduce: gm_rank_sum in rank order) for world = 1, 2 and 8, with the gathered buffer filled
locally -- rank 0's row is the trainer's own contribution, the other rows are zeros -- beside one whole update (Trainer.step on
tools/bench_train.py's batch).  The all-gather itself is NOT here: it needs more than one GPU.  Prints one JSON line.

    python tools/bench_train_dp.py [--hidden 128] [--worlds 1,2,8] [--calls 200] [--rounds 7] [--n 5000] [--batch 2]

Per world: ms per contribution + reduce, median [min, max] of --rounds blocks of --calls calls that end in a synchronise, and the
bytes they move: the copy reads and writes the gradient buffer once, the sum reads it `world` times and writes it once.  The
gradient buffer is a few megabytes and stays in the last-level cache, so a last section times gm_rank_sum alone, by device events,
over --sum-floats floats per rank (128 MB: every row comes from HBM) and reports its rate.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--worlds", type=str, default="1,2,8")
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20, help="updates per block of the whole-update figure")
    ap.add_argument("--sum-floats", type=int, default=1 << 25, help="floats per rank of the stand-alone gm_rank_sum figure (128 MB)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_dp: no HIP device (there is no CPU fallback)")
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, Trainer, scene
    dev = torch.device("cuda:0")
    side = 0.152 * (args.n / 5000.0) ** (1.0 / 3.0) * 0.8              # tools/bench_train.py's batch
    ga = GraphBoundedMultimaterialControl(0.015, scene.STATS, scene.CART, scene.MAT, scene.CTRL, scene.BOUNDS)
    batch = []
    for b in range(args.batch):
        obs = torch.from_numpy(scene.make_scene(args.n, seed=100 + b, side=side)).to(dev)
        batch.append((obs, obs[-1][:, 2:5] + 1e-4))
    with torch.no_grad():
        nodes, edge_attr, edge_index, tgt = ga.process_collate(batch)
    torch.manual_seed(0)
    model = EncProcDecGNN(25, 4, 3, args.hidden, 2, 10).to(dev)
    trainer = Trainer(model, lr=1e-4)

    def block(fn, count):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(count):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / count * 1e3

    stats = lambda v: {"median_ms": float(np.median(v)), "min_ms": min(v), "max_ms": max(v)}
    update = lambda: trainer.step(nodes, edge_attr, edge_index, tgt)
    block(update, 3)
    out = {"metric": "ms per contribution + reduce of a data-parallel update on one GPU (no all-gather), beside one whole update",
           "unit": "ms", "update": stats([block(update, args.steps) for _ in range(args.rounds)]),
           "config": {"workload": f"hidden={args.hidden}, 10 MP steps; the update: batch of {args.batch} scenes x N={args.n}",
                      "nodes": int(nodes.shape[0]), "edges": int(edge_attr.shape[0]), "calls_per_block": args.calls, "rounds": args.rounds}}
    nbytes = trainer.contribution_bytes()
    grad_bytes = nbytes - 32
    out["contribution_bytes"] = nbytes
    worlds = [int(w) for w in args.worlds.split(",")]
    trainer.zero_grad()
    trainer.accumulate(nodes, edge_attr, edge_index, tgt)              # real gradients in the buffer
    buffers, fns, times = {}, {}, {w: [] for w in worlds}
    for w in worlds:
        gathered = torch.zeros((w, nbytes), dtype=torch.uint8, device=dev)
        buffers[w] = gathered

        def exchange(gathered=gathered):
            trainer.contribution(out=gathered[0])                      # rank 0's row; the others stay zeros: the sum keeps its value
            trainer.reduce(gathered, 1)
        fns[w] = exchange
        block(exchange, args.warmup)
    for _ in range(args.rounds):                                       # alternating: drift reaches every world alike
        for w in worlds:
            times[w].append(block(fns[w], args.calls))
    out["worlds"] = {}
    for w in worlds:
        moved = (w + 1) * grad_bytes + 2 * grad_bytes
        s = stats(times[w])
        s.update(bytes_moved=moved, gb_per_s=moved / (s["median_ms"] * 1e-3) / 1e9, share_of_update=s["median_ms"] / out["update"]["median_ms"])
        out["worlds"][str(w)] = s
    out["value"] = out["worlds"][str(worlds[-1])]["median_ms"]
    # gm_rank_sum on its own over rows far larger than the 256 MB last-level cache: its rate from HBM, by device events
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    count = args.sum_floats
    del buffers, fns
    src = torch.randn((max(worlds), count), dtype=torch.float32, device=dev)
    dst = torch.empty(count, dtype=torch.float32, device=dev)
    out["rank_sum_from_hbm"] = {"floats_per_rank": count}
    for w in worlds:
        call = lambda: check(lib().gm_rank_sum(ptr(src), count, w, count, ptr(dst), current_stream(dev)))
        call()
        ms = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(10):
                call()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / 10)
        moved = (w + 1) * 4 * count
        s = stats(ms)
        s.update(bytes_moved=moved, gb_per_s=moved / (s["median_ms"] * 1e-3) / 1e9)
        out["rank_sum_from_hbm"][str(w)] = s
    trainer.status()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
