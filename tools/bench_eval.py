"""Time compute_rollout's ground-truth mode (cma_traj=None) on a synthetic recorded simulation: N particles, `steps` rollout
steps, the flagship model shape.  One JSON line.

    python tools/bench_eval.py [--n 5000] [--steps 100] [--repeats 3] [--root DIR]
    python tools/bench_eval.py --ragged [--sizes 5000,4000,5000,4000] [--steps 20] [--repeats 3]

--ragged: evaluate_rollout over recordings of the sizes --sizes (no Sinkhorn), the default grouping -- a group per node count --
and ragged=True -- one ragged group -- alternating in one process; seconds per call of each.

--root: the tree whose gnn_manip_amd is measured (default: this repository) -- an export of another commit with its library
built, for an A/B of the same call.  The dataset is a CoffeeTestDataset filled in memory; every run includes what the call
includes (the frames it reads from the dataset, the rollout, the copy of the records to the host)."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np


def ragged_main(args):
    import torch
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, evaluate_rollout, scene
    dev = torch.device("cuda:0")
    k = 6
    sizes = [int(v) for v in args.sizes.split(",")]
    steps = min(args.steps, 20) if args.steps == 100 else args.steps
    sims = [torch.from_numpy(np.ascontiguousarray(scene.make_scene(n, seed=5 + i, k=steps + k)[:, :, :5])).to(dev) for i, n in enumerate(sizes)]
    ga = GraphBoundedMultimaterialControl(scene.CONN_R, scene.STATS, scene.CART, scene.MAT, scene.CTRL, scene.BOUNDS)
    torch.manual_seed(0)
    model = EncProcDecGNN(25, 4, 3, 128, 2, 10).to(dev)
    with torch.no_grad():
        list(model.parameters())[-2].mul_(1e-2)
    forms = {"default": False, "ragged": True}
    outs = {name: evaluate_rollout(sims, model, ga, k_steps=k, sinkhorn=False, ragged=flag) for name, flag in forms.items()}     # warm-up
    assert all(torch.equal(a["prediction"], b["prediction"]) for a, b in zip(outs["default"], outs["ragged"]))
    times = {name: [] for name in forms}
    for _ in range(args.repeats):
        for name, flag in forms.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            evaluate_rollout(sims, model, ga, k_steps=k, sinkhorn=False, ragged=flag)
            torch.cuda.synchronize(dev)
            times[name].append(round(time.perf_counter() - t0, 4))
    print(json.dumps({"tool": "bench_eval --ragged", "sizes": sizes, "steps": steps,
                      "seconds": {name: {"rounds": t, "median": float(np.median(t)), "min": min(t), "max": max(t)} for name, t in times.items()}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--ragged", action="store_true", help="evaluate_rollout(ragged=True) against its default grouping")
    ap.add_argument("--sizes", type=str, default="5000,4000,5000,4000", help="--ragged: the recordings' node counts")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    import gnn_manip_amd
    if args.ragged:
        return ragged_main(args)
    from gnn_manip_amd import CoffeeTestDataset, EncProcDecGNN, scene
    from gnn_manip_amd.rollout import compute_rollout

    dev = torch.device("cuda:0")
    k = 6
    T = args.steps + k
    sim = scene.make_scene(args.n, seed=5, k=T)[:, :, :5]
    ds = object.__new__(CoffeeTestDataset)
    ds.k, ds.conn_r, ds.max_neighbours, ds.device, ds.noise, ds.use_control = k, scene.CONN_R, 20, dev, None, True
    ds.data_dim, ds.time_steps, ds.cartesian_idx, ds.control_idx, ds.material_id = 5, T, scene.CART, scene.CTRL, scene.MAT[0]
    ds.stats = {key: torch.tensor(v) for key, v in scene.STATS.items()}
    ds.bounds = {key: torch.tensor(v) for key, v in scene.BOUNDS.items()}
    ds.sims = [torch.from_numpy(np.ascontiguousarray(sim)).to(dev)]
    ds.index = [(0, t) for t in range(T - k)]
    ds.graph_attr = ds._get_graph_attr()

    torch.manual_seed(0)
    model = EncProcDecGNN(25, 4, 3, 128, 2, 10).to(dev)
    with torch.no_grad():
        last = list(model.parameters())[-2]
        last.mul_(1e-2)                       # a damped decoder: the random model's rollout stays a scene
    call = types.SimpleNamespace(cma_traj=None, k_steps=k, device=dev, plot=False)
    out = compute_rollout(ds, model, call)    # warm-up: the library's images, the allocator
    assert out.shape == (args.steps, args.n, 8) and np.isfinite(out).all()
    times = []
    for _ in range(args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        again = compute_rollout(ds, model, call)
        torch.cuda.synchronize(dev)
        times.append(time.perf_counter() - t0)
    assert np.array_equal(again, out)
    print(json.dumps({"tool": "bench_eval", "package": os.path.dirname(gnn_manip_amd.__file__), "n": args.n, "steps": args.steps,
                      "seconds": [round(t, 4) for t in times], "median_s": round(float(np.median(times)), 4),
                      "checksum": float(np.abs(out).sum())}))


if __name__ == "__main__":
    main()
