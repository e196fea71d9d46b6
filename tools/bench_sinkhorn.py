"""Sinkhorn loss forward alone against forward + backward (SamplesLoss under autograd), timed with HIP events.  Prints one JSON
line per shape.

    python tools/bench_sinkhorn.py [--reps 20] [--warmup 3]

Shapes: the planner's (64 candidates against the shared desired cloud, the 4500 non-rigid particles of the C5 scene at N = 5k)
and one 2500 x 2500 pair; and the weighted call at the planner's shape: `planner_weighted`, the same clouds with explicit random
weights on the desired cloud (uniform candidates, the planner's weighted case), and `planner_density`, the desired cloud as
`planner.density_target` at a cell of three particle spacings (216 cells of up to 27 particles).
Per shape, interleaved call by call: `fwd` = the planner's call (torch.no_grad(), shared workspace),
`fwd_grad` = the same call with x requiring grad (own workspace), `fwd_bwd` = that call plus backward() with respect to x (and
to y for the single pair).  Each time is one call between two events on the current stream, host round trip of the default
`diameter` path included; median and range over --reps calls.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def bench(name, X, y, need_y, reps, warmup, b=None):
    from gnn_manip_amd.losses import SamplesLoss
    loss = SamplesLoss(loss="sinkhorn", p=2, blur=0.05)

    def fwd():
        with torch.no_grad():
            loss.batched(X, y, b=b)

    def fwd_grad():
        loss.batched(X.detach().requires_grad_(), y, b=b)

    def fwd_bwd():
        x = X.detach().requires_grad_()
        yy = y.detach().requires_grad_(need_y)
        loss.batched(x, yy, b=b).sum().backward()

    runs = dict(fwd=fwd, fwd_grad=fwd_grad, fwd_bwd=fwd_bwd)
    for _ in range(warmup):
        for fn in runs.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            t[k].append(_time(fn))
    med = {k: float(np.median(v)) for k, v in t.items()}
    rec = dict(shape=name, batch=int(X.shape[0]), n=int(X.shape[1]), m=int(y.shape[-2]), y_shared=y.dim() == 2, weighted=b is not None, dy=need_y,
               reps=reps)
    for k, v in t.items():
        rec[k + "_ms"] = round(med[k], 4)
        rec[k + "_range_ms"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    rec["bwd_ms"] = round(med["fwd_bwd"] - med["fwd_grad"], 4)
    rec["bwd_over_fwd"] = round((med["fwd_bwd"] - med["fwd_grad"]) / med["fwd"], 4)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from gnn_manip_amd import scene
    assert torch.cuda.is_available(), "bench_sinkhorn.py measures on the GPU"
    dev = torch.device("cuda:0")
    obs = scene.make_scene(5000, seed=1000, vel_scale=1e-6)          # bench.py's C5 scene
    cloud = obs[-1][obs[-1][:, 1] != 1][:, 2:5].astype(np.float32)     # its non-rigid rows: the planner's clouds
    rng = np.random.default_rng(0)
    X = np.stack([cloud + 1e-3 * rng.standard_normal(cloud.shape).astype(np.float32) for _ in range(64)])
    Xd, target = torch.from_numpy(X).to(dev), torch.from_numpy(cloud + 0.01).to(dev)
    bench("planner", Xd, target, False, args.reps, args.warmup)
    w = torch.from_numpy(rng.dirichlet(np.ones(len(cloud))).astype(np.float32)).to(dev)
    bench("planner_weighted", Xd, target, False, args.reps, args.warmup, b=w)
    from gnn_manip_amd.planner import density_target
    centres, weights = density_target(target, 0.025)     # the particles sit about 0.0083 apart
    bench("planner_density", Xd, centres, False, args.reps, args.warmup, b=weights)
    x = (0.5 + 0.05 * rng.standard_normal((1, 2500, 3))).astype(np.float32)
    y = (0.53 + 0.07 * rng.standard_normal((2500, 3))).astype(np.float32)
    bench("pair_2500", torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), True, args.reps, args.warmup)


if __name__ == "__main__":
    main()
