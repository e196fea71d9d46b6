"""Milliseconds per rollout step of one TRAINING step on a T-step rollout, for
its two forms on the same windows --

  python     2e's loop: differentiable_rollout(sweep="library", record=True, params=True) under autograd, the recorded poses by
             boolean indexing, torch's L1 loss, torch.optim.Adam over the module's parameters
  library    Trainer.step_rollout: gm_train_rollout_step, one call per sample; with --accumulate B > 1 or --max-grad-norm X the
             mini-batch form instead: zero_grad, B x accumulate_rollout, apply (one update per B samples, the norm of the mean
             gradient clipped to X)

on two synthetic 5000-node recordings rolled side by side as one block-diagonal scene (tools/bench_loader.py's recordings), hidden
128, 10 message-passing steps.  Both forms run the same reverse sweep (gm_rollout_backward_train) and read one edge count per step
back; what differs is the host side.  Every variant is warmed, then the variants alternate in one process for --rounds rounds; a
window is --samples training steps and ends in a synchronise.  Prints one JSON line with every round.

    python tools/bench_train_rollout.py [--n 5000] [--horizons 4,8] [--samples 10] [--rounds 5] [--accumulate B] [--max-grad-norm X]
                                        [--variants python,library]

--batched: another measurement -- what a mini-batch of rollout windows buys as ONE ragged rollout.  The recordings have the sizes
--sizes (a mini-batch of --batch-size windows cycles through them); the two forms of an update alternate in one process:

  sequential  zero_grad, one accumulate_rollout per window on the engine of its size, apply
  batched     zero_grad, one torch.cat of the windows, set_scene on the ragged engine, accumulate_rollout_batch, apply

and the figure is milliseconds per rollout step PER SAMPLE: the update's time / (batch size x T), median [min, max] over the rounds.

    python tools/bench_train_rollout.py --batched [--sizes 5000,4000] [--batch-size 2] [--horizons 4] [--samples 4] [--rounds 3]
"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bench_loader import recording


def batched_main(args):
    """--batched: a mini-batch as one ragged rollout against the same mini-batch sample by sample."""
    from gnn_manip_amd import CoffeeDataset, EncProcDecGNN, RolloutEngine, Trainer, scene
    dev = torch.device("cuda:0")
    sizes = [int(v) for v in args.sizes.split(",")]
    B, T = args.batch_size, int(args.horizons.split(",")[0])
    batch_sizes = [sizes[j % len(sizes)] for j in range(B)]
    frames_needed = args.k + T * (args.samples + 1)
    sets = []
    for j, n in enumerate(batch_sizes):
        side = 0.152 * (n / 5000.0) ** (1.0 / 3.0) * 0.8
        sets.append(CoffeeDataset.from_recordings([torch.from_numpy(recording(n, frames_needed, 300 + j, side)).to(dev)], args.k, 0.015,
                                                  scene.STATS, scene.BOUNDS, scene.CART, scene.MAT[0], scene.CTRL, use_control=True))
    data = [[ds.rollout_sample(i * T, T) for ds in sets] for i in range(args.samples)]      # [update][sample] (window, frames)
    torch.manual_seed(0)
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        m = EncProcDecGNN(3 * (args.k - 1) + 10, 4, 3, args.hidden, 2, 10).to(dev)
        with torch.no_grad():
            list(m.parameters())[-2].mul_(1e-3)
        models.append(m)
    trainers = [Trainer(m, lr=args.lr) for m in models]
    singles = [RolloutEngine(models[0], sets[0].graph_attr, n, k_steps=args.k, data_dim=8, device=dev) for n in batch_sizes]
    ragged = RolloutEngine(models[1], sets[0].graph_attr, k_steps=args.k, data_dim=8, device=dev, sizes=batch_sizes)
    slot = torch.zeros(1, dtype=torch.float64, device=dev)

    def sequential(update):
        t = trainers[0]
        t.zero_grad()
        for eng, (window, frames) in zip(singles, update):
            eng.set_scene(window)
            t.accumulate_rollout(eng, window, frames, T)
        t.apply(loss_out=slot)

    def batched(update):
        t = trainers[1]
        t.zero_grad()
        obs0 = torch.cat([w for w, _ in update], dim=1).contiguous()
        ragged.set_scene(obs0)
        t.accumulate_rollout_batch(ragged, obs0, [f for _, f in update], T)
        t.apply(loss_out=slot)

    variants = {"sequential": sequential, "batched": batched}

    def window(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for update in data:
            fn(update)
        torch.cuda.synchronize()
        assert np.isfinite(float(slot)), float(slot)
        return 1e3 * (time.perf_counter() - t0) / (len(data) * B * T)
    for fn in variants.values():
        fn(data[0])
        fn(data[1 % len(data)])
    rounds = {name: [] for name in variants}
    for _ in range(args.rounds):
        for name, fn in variants.items():
            rounds[name].append(round(window(fn), 3))
    res = {name: {"rounds": r, "median": float(np.median(r)), "min": min(r), "max": max(r)} for name, r in rounds.items()}
    print(json.dumps({"metric": "ms per rollout step per sample of one update on a mini-batch of T-step rollouts", "unit": "ms",
                      "value": res["batched"]["median"], "variants": res,
                      "config": {"sizes": batch_sizes, "batch_size": B, "T": T, "hidden": args.hidden, "updates_per_window": args.samples,
                                 "rounds": args.rounds}, "dtype": "f32", "data": "synthetic"}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batched", action="store_true", help="measure a mini-batch as one ragged rollout against sample by sample")
    ap.add_argument("--sizes", type=str, default="5000,4000", help="--batched: the recordings' node counts")
    ap.add_argument("--batch-size", type=int, default=2, help="--batched: windows per update")
    ap.add_argument("--n", type=int, default=5000)
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=128)
    ap.add_argument("--horizons", type=str, default="4,8")
    ap.add_argument("--samples", type=int, default=10, help="training steps per timed window")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lr", type=float, default=1e-5)
    ap.add_argument("--accumulate", type=int, default=1, help="samples per update of the library form")
    ap.add_argument("--max-grad-norm", type=float, default=None, help="the library form's clip (default: none)")
    ap.add_argument("--variants", type=str, default="python,library")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_train_rollout: no HIP device (there is no CPU fallback)")
    if args.batched:
        return batched_main(args)
    from gnn_manip_amd import CoffeeDataset, EncProcDecGNN, RolloutEngine, Trainer, scene
    dev = torch.device("cuda:0")
    horizons = [int(v) for v in args.horizons.split(",")]
    B = args.accumulate
    if B < 1 or args.samples % B or args.warmup % B:
        raise SystemExit("bench_train_rollout: --samples and --warmup must be multiples of --accumulate")
    mini_batches = B > 1 or args.max_grad_norm is not None
    frames_needed = args.k + max(horizons) * (args.samples + 1)
    side = 0.152 * (args.n / 5000.0) ** (1.0 / 3.0) * 0.8             # tools/bench_train.py's density
    sets = [CoffeeDataset.from_recordings([torch.from_numpy(recording(args.n, frames_needed, 300 + s, side)).to(dev)], args.k, 0.015,
                                          scene.STATS, scene.BOUNDS, scene.CART, scene.MAT[0], scene.CTRL, use_control=True)
            for s in range(args.scenes)]

    def samples(T):
        """(window [k, scenes * n, 8], frames [T, scenes * n, 5]) of every non-overlapping start: the scenes side by side."""
        out = []
        for i in range(args.samples):
            parts = [ds.rollout_sample(i * T, T) for ds in sets]
            out.append((torch.cat([w for w, _ in parts], dim=1).contiguous(), torch.cat([f for _, f in parts], dim=1).contiguous()))
        return out

    def module():
        torch.manual_seed(0)
        m = EncProcDecGNN(3 * (args.k - 1) + 10, 4, 3, args.hidden, 2, 10).to(dev)
        with torch.no_grad():
            list(m.parameters())[-2].mul_(1e-3)                        # a random decoder damped: the rollout stays in the box
        return m

    results = {}
    for T in horizons:
        data = samples(T)
        m_py, m_lib = module(), module()
        eng_py = RolloutEngine(m_py, sets[0].graph_attr, args.n, k_steps=args.k, data_dim=8, device=dev, candidates=args.scenes)
        eng_lib = RolloutEngine(m_lib, sets[0].graph_attr, args.n, k_steps=args.k, data_dim=8, device=dev, candidates=args.scenes)
        eng_py.set_scene(data[0][0])
        eng_lib.set_scene(data[0][0])
        rigid = data[0][0][-1][:, 1] == 1
        free = int((~rigid).sum())
        opt = torch.optim.Adam(m_py.parameters(), lr=args.lr)
        l1 = torch.nn.L1Loss(reduction="sum")
        trainer = Trainer(m_lib, lr=args.lr)
        slot = torch.zeros(1, dtype=torch.float64, device=dev)
        pending = [0]

        def python_step(window, frames):
            poses = frames[:, rigid, 2:5].contiguous()
            final, records = eng_py.differentiable_rollout(window, poses, horizon=T, sweep="library", record=True, params=True)
            pred = torch.cat((records[1:], final[-1:]))
            loss = l1(pred[:, ~rigid, 2:5], frames[:, ~rigid, 2:5]) / (T * free)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss

        def library_step(window, frames):
            trainer.step_rollout(eng_lib, window, frames, T, loss_out=slot)
            return slot

        def library_mini_batch_step(window, frames):
            if pending[0] == 0:
                trainer.zero_grad()
            trainer.accumulate_rollout(eng_lib, window, frames, T)
            pending[0] += 1
            if pending[0] == B:
                trainer.max_grad_norm = args.max_grad_norm
                trainer.apply(loss_out=slot)
                pending[0] = 0
            return slot

        variants = {"python": python_step, "library": library_mini_batch_step if mini_batches else library_step}
        variants = {name: variants[name] for name in args.variants.split(",")}

        def window(fn, count):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(count):
                loss = fn(*data[i % len(data)])
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / (count * T), float(loss.detach())

        for fn in variants.values():
            window(fn, args.warmup)
        rounds = {name: [] for name in variants}
        for _ in range(args.rounds):
            for name, fn in variants.items():
                ms, loss = window(fn, args.samples)
                assert np.isfinite(loss), (name, T, loss)
                rounds[name].append(round(ms, 3))
        results[f"T={T}"] = {name: {"rounds": r, "median": float(np.median(r)), "min": min(r), "max": max(r)} for name, r in rounds.items()}
        if "python" in variants:
            results[f"T={T}"]["edges_last_step"] = eng_py.status()   # the python form's last forward step (the engine's own workspace)
    first = results[f"T={horizons[0]}"]
    out = {"metric": "ms per rollout step of a training step on a T-step rollout (forward + loss + reverse sweep + Adam)", "unit": "ms",
           "value": first["library" if "library" in first else "python"]["median"], "horizons": results,
           "config": {"workload": f"{args.scenes} x N={args.n} side by side, k={args.k}, hidden={args.hidden}, 10 MP steps, L1 on the free rows, Adam",
                      "samples_per_window": args.samples, "rounds": args.rounds, "warmup_samples": args.warmup, "lr": args.lr,
                      "accumulate": B, "max_grad_norm": args.max_grad_norm},
           "dtype": "f32", "data": "synthetic"}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
