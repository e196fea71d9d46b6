"""What the fp16 single-product mode (``model.set_precision("f16")``) buys and costs, measured on one box:

    python tools/bench_precision.py [--configs target,c2,c5,c4] [--alternations 3] [--no-accuracy]

Per configuration of bench.py (target: N = 100k hidden 128; c2: N = 5k; c5: a block-diagonal batch of 8 x 5k; c4: N = 100k hidden
256) ONE model and ONE engine are built, and the two modes are ALTERNATED on them -- f32, f16, f32, f16, ... -- so that both see
the same clocks, the same scene and the same allocator state.  Every pass is a warm-up plus a timed ``engine.run`` of the
configuration's step count, from the same initial state; reported are the passes' steps/s (mean, min, max: the spread of that
mode inside this call) and the ratio of the means.  After the alternations one instrumented pass per mode (gm_model_profile) gives the
kernel time per step and kind.  One JSON line per configuration.

Accuracy: one C5 candidate (N = 5k) rolled out 200 steps in both modes from the same state -- the Sinkhorn loss of the end cloud
against the benchmark's target cloud under each mode, the largest position difference between the two end clouds, and, for scale, the
largest displacement of a particle over the rollout.  With the benchmark's stationary model (decoder output scaled by 1e-5, so that
the pile stays dense) and with a livelier one (--lively-scale, default 1e-3).

The default precision is restored on exit; nothing here changes what bench.py measures."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (the workloads and their engines are bench.py's)

CANDIDATES = {"target": 1, "c2": 1, "c5": 8, "c4": 1}
KINDS = {"edge_kernel": 0, "node_kernel": 1, "graph_build": 2, "encoder_kernels": 3, "csr_and_features": 4}
MODES = ("f32", "f16")


def time_config(key, dev, alternations, steps=None):
    wl = bench.WORKLOADS[key]
    steps = steps or min(wl["steps"], 100)
    warmup = max(wl["warmup"], 2)
    cand = CANDIDATES[key]
    model, eng, obs0, traj, *_ = bench.build_engine(wl, dev, 0, cand, "auto", steps + warmup)
    w_traj, t_traj = traj[:warmup].contiguous(), traj[warmup:].contiguous()
    rates = {m: [] for m in MODES}
    with torch.no_grad():
        for _ in range(alternations):
            for mode in MODES:
                model.set_precision(mode)
                obs = obs0.clone()
                eng.run(obs, w_traj, warmup)
                eng.status()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(obs, t_traj, steps)
                torch.cuda.synchronize()
                rates[mode].append(cand * steps / (time.perf_counter() - t0))
                eng.status()
        kernels = {}
        psteps = min(steps, 64)   # a kind records at most 4096 scopes (bench.py: measure)
        for mode in MODES:
            model.set_precision(mode)
            obs = obs0.clone()
            eng.run(obs, w_traj, warmup)
            model.profile(31)
            eng.run(obs, t_traj[:psteps].contiguous(), psteps)
            torch.cuda.synchronize()
            model.profile(0)
            kernels[mode] = {}
            for name, kind in KINDS.items():
                n_k, ms_k = model.profile_query(kind)
                kernels[mode][name + "_ms_per_step"] = None if n_k < 0 else round(ms_k / psteps, 4)
        edges = eng.status()
    model.set_precision("f32")
    rec = {"config": key, "n_particles": wl["n"], "hidden": wl["hidden"], "candidates": cand, "steps": steps, "alternations": alternations,
           "edges_last_step": edges}
    for mode in MODES:
        r = rates[mode]
        rec[mode] = {"steps_per_s_mean": round(float(np.mean(r)), 2), "min": round(min(r), 2), "max": round(max(r), 2),
                     "spread_percent": round(100 * (max(r) - min(r)) / float(np.mean(r)), 2), "passes": [round(x, 2) for x in r],
                     "kernels": kernels[mode]}
    rec["f16_over_f32"] = round(rec["f16"]["steps_per_s_mean"] / rec["f32"]["steps_per_s_mean"], 4)
    return rec


def accuracy(dev, decoder_scale, horizon=200):
    from gnn_manip_amd.losses import SamplesLoss
    wl = bench.WORKLOADS["c5"]
    model, eng, obs0, traj, *_ = bench.build_engine(wl, dev, 0, 1, "auto", horizon)
    if decoder_scale != 1e-5:   # build_engine scaled the decoder's output layer by 1e-5
        with torch.no_grad():
            model.decoder[-1].weight.mul_(decoder_scale / 1e-5)
            model.decoder[-1].bias.mul_(decoder_scale / 1e-5)
    free = torch.nonzero(obs0[-1, :, 1] != 1).reshape(-1)
    target = (obs0[-1].index_select(0, free)[:, 2:5] + 0.01).contiguous()
    loss_fn = SamplesLoss("sinkhorn", p=2, blur=0.05)
    ends, losses, edges = {}, {}, {}
    with torch.no_grad():
        for mode in MODES:
            model.set_precision(mode)
            end = eng.rollout(obs0, traj, horizon=horizon)
            edges[mode] = eng.status()
            ends[mode] = end[-1].index_select(0, free)[:, 2:5].contiguous()
            losses[mode] = float(loss_fn.batched(ends[mode].unsqueeze(0).contiguous(), target).double().cpu()[0])
    model.set_precision("f32")
    start = obs0[-1].index_select(0, free)[:, 2:5]
    return {"accuracy": "one C5 candidate", "n_particles": wl["n"], "horizon": horizon, "decoder_output_scale": decoder_scale,
            "sinkhorn_loss_f32": losses["f32"], "sinkhorn_loss_f16": losses["f16"],
            "loss_difference_relative": abs(losses["f16"] - losses["f32"]) / max(abs(losses["f32"]), 1e-30),
            "max_position_difference": float((ends["f16"] - ends["f32"]).abs().max()),
            "max_displacement_over_rollout_f32": float((ends["f32"] - start).abs().max()),
            "finite": bool(torch.isfinite(ends["f16"]).all() and torch.isfinite(ends["f32"]).all()),
            "edges_last_step": edges}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--configs", default="target,c2,c5,c4")
    ap.add_argument("--alternations", type=int, default=3)
    ap.add_argument("--steps", type=int, default=0, help="timed steps per pass (0: the configuration's own, at most 100)")
    ap.add_argument("--no-accuracy", action="store_true")
    ap.add_argument("--lively-scale", type=float, default=1e-3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_precision.py needs a GPU"
    assert args.alternations >= 1
    dev = torch.device("cuda:0")
    for key in [k for k in args.configs.split(",") if k]:
        print(json.dumps(time_config(key, dev, args.alternations, args.steps)), flush=True)
    if not args.no_accuracy:
        for scale in (1e-5, args.lively_scale):
            print(json.dumps(accuracy(dev, scale)), flush=True)


if __name__ == "__main__":
    main()
