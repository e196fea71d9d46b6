"""Training steps/s with the data loader INSIDE the timed loop: what an epoch of examples/train_dyn.py
runs at, for four ways of getting its batches --

  fixed      one batch built once outside the loop: tools/bench_train.py's measurement, the ceiling
  unfused    GraphLoader(fused=False): every sample through torch calls and the stand-alone entry points
  fused_p0   GraphLoader(fused=True, prefetch=0): the library's two phases, waiting for its own edge count
  fused_p1   GraphLoader(fused=True, prefetch=1): the next batch's first phase queued ahead of the step

on synthetic resident recordings (scene.make_scene plus a seeded drift), the reference's training configuration (batch of 2,
hidden 128, 10 message-passing steps, L1 loss, Adam).  Every variant is warmed, then the variants alternate in one process for
--rounds rounds; a window is --steps steps and ends in a synchronise.  Prints one JSON line with every round.

    python tools/bench_loader.py [--n 5000] [--sims 2] [--frames 206] [--steps 200] [--rounds 3]

--n-list 5000,4000 gives the recordings those sizes in turn (recording s has n_list[s % len] rows, each at its own size's density):
a shuffled loader then meets batches that mix sizes, which the fused variants build in one ragged library call.
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def recording(n, frames, seed, side):
    """[frames, n, 5] float32: a dense scene whose rows wander a fraction of the radius around their places while the whole scene
    drifts, so that velocities, controls and targets are non-zero and the graph keeps its density over the recording."""
    from gnn_manip_amd import scene
    base = scene.make_scene(n, seed=seed, k=1, side=side)[0, :, :5]
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    amp = 1e-3 * rng.random((n, 3))
    phase = 2 * np.pi * rng.random((n, 3))
    t = np.arange(frames, dtype=np.float64)[:, None, None]
    drift = 2e-3 * np.stack((np.sin(t[:, 0, 0] / 40), np.cos(t[:, 0, 0] / 55) - 1, np.sin(t[:, 0, 0] / 70)), axis=-1)[:, None, :]
    rec = np.repeat(base[None], frames, axis=0)
    rec[:, :, 2:5] = (base[None, :, 2:5].astype(np.float64) + amp * np.sin(t / 9 + phase) + drift).astype(np.float32)
    return np.ascontiguousarray(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--n-list", type=str, default=None, help="comma-separated recording sizes, taken in turn (overrides --n)")
    ap.add_argument("--sims", type=int, default=2)
    ap.add_argument("--frames", type=int, default=206, help="frames per recording: an epoch is sims * (frames - k) / batch batches")
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--noise", type=float, default=3e-4)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed window (at least 200 for a figure of record)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader: no HIP device (there is no CPU fallback)")
    from gnn_manip_amd import CoffeeDataset, EncProcDecGNN, GraphLoader, scene
    dev = torch.device("cuda:0")
    n_list = [int(v) for v in args.n_list.split(",")] if args.n_list else [args.n]
    sizes = [n_list[s % len(n_list)] for s in range(args.sims)]
    side = lambda n: 0.152 * (n / 5000.0) ** (1.0 / 3.0) * 0.8        # tools/bench_train.py's density
    sims = [torch.from_numpy(recording(n, args.frames, 300 + s, side(n))).to(dev) for s, n in enumerate(sizes)]
    ds = CoffeeDataset.from_recordings(sims, args.k, 0.015, scene.STATS, scene.BOUNDS, scene.CART, scene.MAT[0], scene.CTRL, noise=args.noise,
                                       use_control=True)
    H, M = args.hidden, 10
    torch.manual_seed(0)
    model = EncProcDecGNN(3 * (args.k - 1) + 10, 4, 3, H, 2, M).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    crit = torch.nn.L1Loss(reduction="sum")

    def step(b):
        pred = model.forward(b.x, b.edge_attr, b.edge_index)
        loss = crit(pred, b.y) / pred.shape[0]
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    def endless(loader):
        while True:
            yield from loader

    def fixed_batches():
        b = next(iter(GraphLoader(ds, batch_size=args.batch, shuffle=True, seed=0)))
        while True:
            yield b

    variants = {
        "fixed": fixed_batches(),
        "unfused": endless(GraphLoader(ds, batch_size=args.batch, shuffle=True, seed=0)),
        "fused_p0": endless(GraphLoader(ds, batch_size=args.batch, shuffle=True, seed=0, fused=True, prefetch=0)),
        "fused_p1": endless(GraphLoader(ds, batch_size=args.batch, shuffle=True, seed=0, fused=True, prefetch=1)),
    }

    def window(it, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        edges = 0
        for _ in range(steps):
            b = next(it)
            edges += int(b.edge_attr.shape[0])
            loss = step(b)
        torch.cuda.synchronize()
        return steps / (time.perf_counter() - t0), edges / steps, float(loss.detach())

    for it in variants.values():
        window(it, args.warmup)
    rounds = {name: [] for name in variants}
    edges = {}
    for _ in range(args.rounds):
        for name, it in variants.items():
            rate, e, loss = window(it, args.steps)
            rounds[name].append(round(rate, 2))
            edges[name] = round(e)
            assert np.isfinite(loss), (name, loss)
    out = {"metric": "training steps/sec with the loader inside the loop (forward + backward + Adam)", "unit": "steps/s",
           "value": float(np.median(rounds["fused_p1"])),
           "variants": {name: {"rounds": r, "median": float(np.median(r)), "min": min(r), "max": max(r), "mean_edges": edges[name]}
                        for name, r in rounds.items()},
           "config": {"workload": f"batch of {args.batch} x N={'/'.join(str(n) for n in sorted(set(sizes)))}, k={args.k}, noise {args.noise}, hidden={H}, 10 MP steps, L1, Adam",
                      "recordings": args.sims, "frames": args.frames, "batches_per_epoch": len(ds) // args.batch,
                      "steps_per_window": args.steps, "rounds": args.rounds, "warmup_steps": args.warmup},
           "dtype": "f32", "data": "synthetic"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
