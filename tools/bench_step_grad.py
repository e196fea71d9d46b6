"""Input gradients of a rollout step, timed with HIP events.  Prints one JSON line per shape.

    python tools/bench_step_grad.py [--reps 10] [--warmup 2] [--shapes train,100k] [--horizon 4] [--parent-lib PATH]

Shapes: `train` = the training benchmark's graph (two collated 5000-node scenes, hidden 128, 10 message-passing steps) and
`100k` = one scene of N = 100k.  Per shape, interleaved call by call:
  * `bwd` = gm_epd_backward and `bwd_inputs` = gm_epd_backward_inputs with both outputs, on the SAME tape of one training forward
    (the backward reads the tape and writes its own workspace): what d_nodes / d_edge_attr cost on top of the parameter gradients;
    `bwd_inputs_only` = gm_epd_backward_inputs_only on that tape: what leaving the weight-gradient work out saves.  With
    --parent-lib (a build of another commit's library, e.g. `python -m gnn_manip_amd.build --tag=parent` in a checkout of it),
    `bwd_inputs_parent` = THAT library's gm_epd_backward_inputs, on a model handle and a tape of its own making, in the same
    interleaving;
  * `step_fwd_bwd` = RolloutEngine.differentiable_step on the shape's state plus backward() of a seeded linear loss with respect to
    obs and rigid_target (the forward's one host read of the edge count included); `step_fwd` = the same forward under no_grad;
  * `tape_bytes` = gm_train_tape_bytes of the step's graph;
  * `rollout_bwd_per_step` = the backward sweep of RolloutEngine.differentiable_rollout over --horizon steps (one re-run step and
    its inputs-only backward per step), divided by the horizon; `rollout_fwd_per_step` its forward (the inference rollout plus one
    window copy per step).  `rollout_peak_bytes` / `unrolled_peak_bytes`: torch.cuda.max_memory_allocated above the level before
    the call, over forward + backward of that rollout and of the same horizon unrolled through differentiable_step (every
    step's tape alive until backward()).
  * the reverse sweep inside the library, against the autograd one, in the same run: `lib_step_bwd` = one
    RolloutEngine.step_backward (gm_rollout_step_backward: the step's forward with a tape and every transpose, one library call)
    and `autograd_step_bwd` = one step of the autograd sweep, the body of the loop in _RolloutFunction.backward (differentiable_step
    with inputs_only on the window under enable_grad, then torch.autograd.grad), both on the same window, pose and upstream
    gradient, interleaved call by call; `rollout_lib_bwd_per_step` / `rollout_lib_fwd_per_step` / `rollout_lib_peak_bytes` = the
    rollout figures above with differentiable_rollout(sweep="library").  `sweep_ws_bytes` = gm_rollout_backward_workspace_bytes
    (sized for N x max_neighbours edges whatever the graph holds; the engine keeps it once allocated, so the peak of a later call
    does not count it: it is reported next to the peaks).
  * training through the rollout: `sweep_lib_bwd_per_step` / `sweep_train_bwd_per_step` = ONE reverse sweep of --horizon steps
    (RolloutEngine._sweep_backward: gm_rollout_backward_train) on the windows of one forward, without and with `grads` (zeroed
    outside the timed window) and a gradient on every record, interleaved call by call, divided by the horizon: what the
    weight-gradient launches add to a step of the sweep, to be read against `bwd_inputs` - `bwd_inputs_only` of the same run.
Each time is one call between two events on the current stream; median and range over --reps calls.
"""
import argparse
import ctypes as C
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


def _load_parent(path):
    """Another build of the library: only what the comparison calls, with this tree's prototypes (the ABI version is the same)."""
    from gnn_manip_amd._lib import PROTOTYPES
    P = C.CDLL(path)
    for name in ("gm_model_create", "gm_model_destroy", "gm_train_tape_bytes", "gm_epd_forward_train",
                 "gm_train_backward_inputs_workspace_bytes", "gm_epd_backward_inputs", "gm_last_error"):
        fn = getattr(P, name)
        fn.restype, fn.argtypes = PROTOTYPES[name]
    return P


def _peak(fn, dev):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated(dev) - base)


def bench(name, scenes, reps, warmup, hidden=128, m_steps=10, horizon=4, parent_lib=None):
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, scene
    from gnn_manip_amd._lib import ModelDesc, check, current_stream, lib, ptr
    from gnn_manip_amd.epd_gnn import _grad_arrays, _ws
    dev = torch.device("cuda:0")
    L = lib()
    ga = GraphBoundedMultimaterialControl(0.015, scene.STATS, scene.CART, scene.MAT, scene.CTRL, scene.BOUNDS)
    torch.manual_seed(0)
    model = EncProcDecGNN(25, 4, 3, hidden, 2, m_steps).to(dev)
    obs = torch.from_numpy(np.concatenate(scenes, axis=1)).to(dev).contiguous()
    n_per = scenes[0].shape[1]
    eng = RolloutEngine(model, ga, n_per, k_steps=obs.shape[0], data_dim=obs.shape[2], device=dev, candidates=len(scenes))
    n_rigid = eng.set_scene(obs)
    target = obs[-1][eng.rigid_rows][:, 2:5].contiguous() + 2e-4

    # ---- the two backward entry points on one tape
    with torch.no_grad():
        _, _, ei = eng.differentiable_step(obs, target)
        nodes = ga.compute_nodes(obs)
        edge_attr = ga.compute_edges(obs, ei[0], ei[1]).contiguous()
    n, e = int(nodes.shape[0]), int(edge_attr.shape[0])
    d = ModelDesc(*model.model_desc())
    h = model.device_handle(dev)
    tape = _ws(L.gm_train_tape_bytes(C.byref(d), n, e), dev)
    out = torch.empty((n, 3), device=dev)
    check(L.gm_epd_forward_train(h, ptr(nodes), n, ptr(edge_attr), ptr(ei.contiguous()), e, ptr(out), ptr(tape), tape.numel(), current_stream()))
    grad_out = torch.randn_like(out)
    tensors, views, t_arr, g_arr = _grad_arrays(list(model.parameters()), dev)
    ws = _ws(L.gm_train_backward_inputs_workspace_bytes(C.byref(d), n, e), dev)
    d_nodes, d_edge_attr = torch.empty_like(nodes), torch.empty_like(edge_attr)

    def bwd():
        check(L.gm_epd_backward(h, t_arr, len(tensors), ptr(nodes), ptr(edge_attr), n, e, ptr(grad_out), g_arr, ptr(tape), tape.numel(),
                                ptr(ws), ws.numel(), current_stream()))

    def bwd_inputs():
        check(L.gm_epd_backward_inputs(h, t_arr, len(tensors), ptr(nodes), ptr(edge_attr), n, e, ptr(grad_out), g_arr, ptr(d_nodes),
                                       ptr(d_edge_attr), ptr(tape), tape.numel(), ptr(ws), ws.numel(), current_stream()))

    def bwd_inputs_only():
        check(L.gm_epd_backward_inputs_only(h, t_arr, len(tensors), ptr(nodes), ptr(edge_attr), n, e, ptr(grad_out), ptr(d_nodes),
                                            ptr(d_edge_attr), ptr(tape), tape.numel(), ptr(ws), ws.numel(), current_stream()))

    model_calls = dict(bwd=bwd, bwd_inputs=bwd_inputs, bwd_inputs_only=bwd_inputs_only)
    if parent_lib:
        P = _load_parent(parent_lib)
        hp = C.c_void_p()
        assert P.gm_model_create(C.byref(d), t_arr, len(tensors), 1, current_stream(), C.byref(hp)) == 0, P.gm_last_error()
        tape_p, ws_p, out_p = torch.empty_like(tape), torch.empty_like(ws), torch.empty_like(out)
        assert P.gm_epd_forward_train(hp, ptr(nodes), n, ptr(edge_attr), ptr(ei.contiguous()), e, ptr(out_p), ptr(tape_p), tape_p.numel(),
                                      current_stream()) == 0, P.gm_last_error()
        dn_p, de_p = torch.empty_like(nodes), torch.empty_like(edge_attr)

        def bwd_inputs_parent():
            rc = P.gm_epd_backward_inputs(hp, t_arr, len(tensors), ptr(nodes), ptr(edge_attr), n, e, ptr(grad_out), g_arr, ptr(dn_p),
                                          ptr(de_p), ptr(tape_p), tape_p.numel(), ptr(ws_p), ws_p.numel(), current_stream())
            assert rc == 0, P.gm_last_error()
        model_calls["bwd_inputs_parent"] = bwd_inputs_parent

    w_o = torch.randn_like(obs)
    traj = torch.stack([target + 2e-4 * t for t in range(horizon)]).contiguous()
    sweep = {}

    def rollout_fwd_bwd(which="autograd", key="rollout"):
        o, tr = obs.detach().requires_grad_(), traj.detach().requires_grad_()
        a, b, c = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        a.record()
        final = eng.differentiable_rollout(o, tr, horizon=horizon, sweep=which)
        loss = (final * w_o).sum()
        b.record()
        loss.backward()
        c.record()
        c.synchronize()
        sweep.setdefault(key + "_fwd_per_step", []).append(a.elapsed_time(b) / horizon)
        sweep.setdefault(key + "_bwd_per_step", []).append(b.elapsed_time(c) / horizon)

    def rollout_lib_fwd_bwd():
        rollout_fwd_bwd("library", "rollout_lib")

    def lib_step_bwd():
        eng.step_backward(obs, target, w_o)

    def autograd_step_bwd():      # the body of the loop in _RolloutFunction.backward
        with torch.enable_grad():
            w = obs.detach().requires_grad_(True)
            pose = target.detach().clone().requires_grad_(True)
            nxt, _, _ = eng.differentiable_step(w, pose, inputs_only=True)
        torch.autograd.grad(nxt, [w, pose], grad_outputs=w_o)

    def unrolled_fwd_bwd():
        o, tr = obs.detach().requires_grad_(), traj.detach().requires_grad_()
        cur = o
        for t in range(horizon):
            cur, _, _ = eng.differentiable_step(cur, tr[t], inputs_only=True)
        (cur * w_o).sum().backward()

    def step_fwd():
        with torch.no_grad():
            eng.differentiable_step(obs, target)

    def step_fwd_bwd():
        o, t = obs.detach().requires_grad_(), target.detach().requires_grad_()
        nxt, _, _ = eng.differentiable_step(o, t)
        (nxt * w_o).sum().backward()

    t = {}
    for group in (model_calls, dict(step_fwd=step_fwd, step_fwd_bwd=step_fwd_bwd),
                  dict(lib_step_bwd=lib_step_bwd, autograd_step_bwd=autograd_step_bwd)):
        for _ in range(warmup):
            for fn in group.values():
                fn()
        torch.cuda.synchronize()
        for k in group:
            t[k] = []
        for _ in range(reps):
            for k, fn in group.items():
                t[k].append(_time(fn))
        if "bwd" in group:   # the tapes and workspaces of the first group are not needed by the second
            tape = ws = None
            if parent_lib:
                tape_p = ws_p = None
                P.gm_model_destroy(hp)
    rollout_fwd_bwd()                     # warm-up
    rollout_lib_fwd_bwd()
    sweep.clear()
    for _ in range(max(1, reps // 2)):    # the two sweeps interleaved
        rollout_fwd_bwd()
        rollout_lib_fwd_bwd()
    t.update(sweep)

    # ---- the library sweep without and with parameter gradients, on the windows of one forward
    windows = torch.empty((horizon,) + tuple(obs.shape), device=dev)
    cur = obs.clone()
    eng.set_scene(cur)
    for i in range(horizon):
        windows[i].copy_(cur)
        eng.step(cur, traj[i])
    eng.status()
    scene_key = (eng.rigid_rank, eng.n_rigid)
    _, tr_tensors, _, tr_desc = eng._training_model()
    p_grads = [torch.zeros_like(x) for x in tr_tensors]
    d_records = torch.randn((horizon,) + tuple(obs.shape[1:]), device=dev)

    def sweep_lib():
        eng._sweep_backward(windows, traj, horizon, w_o, scene_key, True)

    def sweep_train():
        eng._sweep_backward(windows, traj, horizon, w_o, scene_key, True, d_records=d_records, grads=p_grads)

    for _ in range(warmup):
        sweep_lib()
        sweep_train()
    torch.cuda.synchronize()
    t["sweep_lib_bwd_per_step"], t["sweep_train_bwd_per_step"] = [], []
    for _ in range(reps):
        t["sweep_lib_bwd_per_step"].append(_time(sweep_lib) / horizon)
        for x in p_grads:
            x.zero_()
        torch.cuda.synchronize()
        t["sweep_train_bwd_per_step"].append(_time(sweep_train) / horizon)
    windows = d_records = None
    peaks = dict(rollout_peak_bytes=_peak(rollout_fwd_bwd, dev), rollout_lib_peak_bytes=_peak(rollout_lib_fwd_bwd, dev),
                 unrolled_peak_bytes=_peak(unrolled_fwd_bwd, dev),
                 sweep_ws_bytes=int(L.gm_rollout_backward_workspace_bytes(C.byref(d), C.byref(eng.fdesc), eng.n, eng.max_neighbours)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    rec = dict(shape=name, nodes=n, edges=e, rigid=n_rigid, hidden=hidden, m_steps=m_steps, reps=reps,
               tape_bytes=int(L.gm_train_tape_bytes(C.byref(d), n, e)))
    for k, v in t.items():
        rec[k + "_ms"] = round(med[k], 4)
        rec[k + "_range_ms"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    rec["inputs_over_bwd"] = round(med["bwd_inputs"] / med["bwd"], 4)
    rec["inputs_only_over_inputs"] = round(med["bwd_inputs_only"] / med["bwd_inputs"], 4)
    if parent_lib:
        rec["inputs_only_over_parent_inputs"] = round(med["bwd_inputs_only"] / med["bwd_inputs_parent"], 4)
    rec["lib_over_autograd_step"] = round(med["lib_step_bwd"] / med["autograd_step_bwd"], 4)
    rec["train_minus_lib_sweep_per_step_ms"] = round(med["sweep_train_bwd_per_step"] - med["sweep_lib_bwd_per_step"], 4)
    rec["bwd_inputs_minus_inputs_only_ms"] = round(med["bwd_inputs"] - med["bwd_inputs_only"], 4)
    rec["lib_over_autograd_sweep"] = round(med["rollout_lib_bwd_per_step"] / med["rollout_bwd_per_step"], 4)
    rec.update(horizon=horizon, **peaks)
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="train,100k")
    ap.add_argument("--horizon", type=int, default=4)
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    from gnn_manip_amd import scene
    assert torch.cuda.is_available(), "bench_step_grad.py measures on the GPU"
    for shape in args.shapes.split(","):
        if shape == "train":      # bench.py extra_train's batch
            bench("train_2x5000", [scene.make_scene(5000, seed=100 + b, side=0.152 * 0.8) for b in range(2)], args.reps, args.warmup,
                  horizon=args.horizon, parent_lib=args.parent_lib)
        elif shape == "100k":
            bench("scene_100k", [scene.make_scene(100000, seed=1000)], args.reps, args.warmup, horizon=args.horizon,
                  parent_lib=args.parent_lib)
        else:
            raise SystemExit(f"unknown shape {shape!r}")


if __name__ == "__main__":
    main()
