"""Device-resident rollout: host-side mirror of the reference's rollout loop
(``compute_rollout`` gnn_manip/utils/rollout_utils.py:14-67 == ``cma_objective``'s loop
gnn_manip/utils/traj_utils.py:119-152) and of ``get_position_from_prediction``
(rollout_utils.py:145-158).

One step = state_pre -> node features -> radius graph -> destination sort -> edge features ->
encode/process/decode -> Euler integration -> state_post, all enqueued on the current HIP stream
by ``gm_rollout_step`` with no host synchronisation and no PCIe traffic.
"""
import ctypes as C
import os

import torch
from torch.autograd.function import once_differentiable

from ._lib import ModelDesc, check, current_stream, lib, ptr
from .epd_gnn import _device_arrays, _pointers, _zeroed_like
from .graph import _NodeFeaturesFunction, _need_cuda, _node_features, _ws, get_connectivity, get_edges_displacement, make_feature_desc


def get_position_from_prediction(stats, cartesian_idx, pred_acc, obs_seq, _desc=None):
    """Reference ``get_position_from_prediction`` (rollout_utils.py:145-158) on the device.  Differentiable in ``pred_acc`` and
    ``obs_seq``."""
    _need_cuda(pred_acc, "pred_acc")
    obs = obs_seq.contiguous().float()
    pred = pred_acc.contiguous().float()
    k, n, dd = obs.shape
    if _desc is None:
        one = [1.0, 1.0, 1.0]
        full = dict(velocity_mean=[0.0] * 3, velocity_std=one)
        full.update(stats)
        _desc = make_feature_desc(1.0, full, dict(lower_bounds=[0.0] * 3, upper_bounds=one), cartesian_idx,
                                  [0], None, k, dd)
    if torch.is_grad_enabled() and (pred.requires_grad or obs.requires_grad):
        return _IntegrateFunction.apply(pred, obs, _desc)
    return _integrate(pred, obs, _desc)


def _integrate(pred, obs, desc):
    n = int(obs.shape[1])
    out = torch.empty((n, 3), dtype=torch.float32, device=obs.device)
    check(lib().gm_integrate(ptr(pred), ptr(obs), n, C.byref(desc), ptr(out), current_stream()))
    return out


class _IntegrateFunction(torch.autograd.Function):
    """get_position_from_prediction under autograd (it is linear): gm_integrate_backward."""

    @staticmethod
    def forward(ctx, pred, obs, desc):
        ctx.desc, ctx.shape = desc, tuple(obs.shape)
        return _integrate(pred, obs, desc)

    @staticmethod
    def backward(ctx, d_next):
        d_next = d_next.contiguous().float()
        n = ctx.shape[1]
        d_pred = torch.empty((n, 3), dtype=torch.float32, device=d_next.device)
        d_obs = torch.empty(ctx.shape, dtype=torch.float32, device=d_next.device)
        check(lib().gm_integrate_backward(ptr(d_next), n, C.byref(ctx.desc), ptr(d_pred), ptr(d_obs), current_stream()))
        return (d_pred if ctx.needs_input_grad[0] else None), (d_obs if ctx.needs_input_grad[1] else None), None


def _roll_forward(engine, obs0, trajectory, steps, keep, records=None):
    """The forward of both rollout Functions: the inference rollout -- ``step`` in place on a detached clone of ``obs0``, no tape,
    one synchronisation at its end -- with ``keep(t, window)`` called on every pre-step window, all the backward needs of step t
    besides its pose; how the windows are held is the caller's business.  records: None or [steps, N, D] to fill.  Returns the
    final state and the trajectory as the steps read it (detached, contiguous float32)."""
    obs = obs0.detach().clone().contiguous()
    traj = None if trajectory is None else trajectory.detach().contiguous().float()
    engine.set_scene(obs)
    for t in range(steps):
        keep(t, obs)
        engine.step(obs, None if traj is None else traj[t])
        if records is not None:
            # the last frame after step t's control overwrite is frame k-2 of the window the step left (the shift moved it there)
            records[t].copy_(obs[-2])
    engine.status()
    return obs, traj


class _RolloutFunction(torch.autograd.Function):
    """RolloutEngine.differentiable_rollout: the inference rollout forward, a reverse sweep of re-run differentiable steps backward."""

    @staticmethod
    def forward(ctx, engine, obs0, trajectory, steps, edges):
        windows = []
        obs, traj = _roll_forward(engine, obs0, trajectory, steps, lambda t, window: windows.append(window.clone()))
        ctx.engine, ctx.windows, ctx.traj, ctx.edges = engine, windows, traj, edges
        ctx.scene = (engine.rigid_rank, engine.rigid_rows, engine.n_rigid)
        return obs

    @staticmethod
    @once_differentiable
    def backward(ctx, d_window):
        eng, traj = ctx.engine, ctx.traj
        eng.rigid_rank, eng.rigid_rows, eng.n_rigid = ctx.scene   # the engine may have been given another scene since
        need_traj = traj is not None and ctx.needs_input_grad[2]
        d_traj = torch.zeros_like(traj) if need_traj else None
        edges = [None] * len(ctx.windows)   # of the recomputed steps, for the caller's list (return_edges)
        d_window = d_window.contiguous().float()
        for t in range(len(ctx.windows) - 1, -1, -1):
            with torch.enable_grad():
                w = ctx.windows[t].requires_grad_(True)
                pose = None if traj is None else traj[t].clone().requires_grad_(need_traj)
                nxt, _, ei = eng.differentiable_step(w, pose, inputs_only=True)
            # step t's tape lives from here to the end of this call to autograd, which frees it: one tape at a time
            grads = torch.autograd.grad(nxt, [w, pose] if need_traj else [w], grad_outputs=d_window)
            d_window = grads[0]
            if need_traj:
                d_traj[t] = grads[1]
            ctx.windows[t] = None
            edges[t] = ei if ctx.edges is not None else None
            del nxt, w, pose, grads
        if ctx.edges is not None:
            ctx.edges[:] = edges
        return None, (d_window if ctx.needs_input_grad[1] else None), d_traj, None, None


class _RolloutTrainFunction(torch.autograd.Function):
    """RolloutEngine.differentiable_rollout(sweep="library"): _RolloutFunction's forward with the windows kept in one [T, k, N, D]
    array, and the whole reverse sweep as one gm_rollout_backward_train call.  `record`: the per-step records are a second
    output.  `model`: None (the parameters are constants, no tensors follow: the sweep is gm_rollout_backward's) or the (gm_model
    handle, descriptor) the tensors that follow belong to, as EncProcDecGNN._training_spec resolved them from the LIVE
    parameters -- the parameters themselves, or the padded tensors built from them under autograd, which then carries their
    gradients back into the checkpoint's shapes."""

    @staticmethod
    def forward(ctx, engine, obs0, trajectory, steps, record, model, *tensors):
        windows = torch.empty((steps,) + tuple(obs0.shape), dtype=torch.float32, device=obs0.device)
        records = torch.empty((steps,) + tuple(obs0.shape[1:]), dtype=torch.float32, device=obs0.device) if record else None
        obs, traj = _roll_forward(engine, obs0, trajectory, steps, lambda t, window: windows[t].copy_(window), records)
        ctx.engine, ctx.windows, ctx.traj, ctx.steps, ctx.model, ctx.record = engine, windows, traj, steps, model, record
        ctx.scene = (engine.rigid_rank, engine.n_rigid)
        ctx.save_for_backward(*tensors)
        ctx.set_materialize_grads(False)   # an output the loss does not touch: no gradient array is made up (or read) for it
        return (obs, records) if record else obs

    @staticmethod
    @once_differentiable
    def backward(ctx, d_final, d_records=None):
        eng = ctx.engine
        if d_final is None:
            d_final = torch.zeros((eng.k, eng.n, eng.data_dim), dtype=torch.float32, device=eng.device)
        need_traj = ctx.traj is not None and ctx.needs_input_grad[2]
        tensors = ctx.saved_tensors
        model = grads = None
        if ctx.model is not None:
            h, mdesc = ctx.model
            model = (h,) + _device_arrays(tensors, eng.device) + (mdesc,)
            if any(ctx.needs_input_grad[6:]):
                grads = _zeroed_like(model[1])   # ONE set, whatever T
        d_obs0, d_traj = eng._sweep_backward(ctx.windows, ctx.traj, ctx.steps, d_final.contiguous().float(), ctx.scene, need_traj,
                                             d_records=None if d_records is None else d_records.contiguous().float(), model=model,
                                             grads=grads)
        ctx.windows = None
        d_tensors = tuple(g if ctx.needs_input_grad[6 + i] else None for i, g in enumerate(grads)) if grads else (None,) * len(tensors)
        return (None, (d_obs0 if ctx.needs_input_grad[1] else None), d_traj, None, None, None) + d_tensors


class RolloutEngine:
    """Runs rollouts of an ``EncProcDecGNN`` for scenes of ``n_nodes`` particles.

    graph_attr: a ``GraphBoundedMultimaterial(Control)`` (gnn_manip_amd.graph) carrying conn_r,
    stats, bounds and the column indices, exactly like ``dataset.graph_attr`` in the reference.
    The engine follows the model's ``set_precision``: every step it runs is in the arithmetic the model has at that call.
    """

    # run() renumbers the particles of scenes at least this large in grid-cell order, again every RENUMBER_EVERY steps
    RENUMBER_MIN_NODES = 20000
    RENUMBER_EVERY = 64

    def __init__(self, model, graph_attr, n_nodes=None, k_steps=6, data_dim=None, max_neighbours=20, device="cuda:0",
                 candidates=1, renumber="auto", sizes=None):
        """candidates > 1: the engine steps that many equal-sized scenes at once, stored back to back along the
        node axis ([k, candidates*n_nodes, D]); the radius graph never links two scenes (block-diagonal batch,
        the offset rule of collate_utils.py:76), everything else is per node / per edge.

        renumber: True / False / "auto" (scenes of RENUMBER_MIN_NODES particles or more).  ``run`` then asks the library
        (gm_rollout, renumber_every = RENUMBER_EVERY) to work on a copy of the state whose rows are in grid-cell order (the
        radius graph's own grid, x fastest; particles of a cell in index order: the same every time), so that the per-edge
        gathers of neighbouring rows find each other in cache, re-ordered every RENUMBER_EVERY steps (particles move a
        fraction of a cell per step), and to write the result back in the caller's numbering.  A radius graph does not depend on the numbering
        (neighbours are ranked by distance; only an exact tie in distance falls back on the index) and every per-node /
        per-edge function is numbering-free, so what changes is the order in which a node's incoming messages are
        summed: float32 rounding, far inside the 1e-5 parity bound.

        sizes=[n0, n1, ...] (with n_nodes=None): a RAGGED engine, which steps scenes of these sizes at once, stored back to back
        along the node axis ([k, n0 + n1 + ..., D]; ``offsets``, ``rows(g)``), through the library's ``_ragged`` entry points:
        ``step``, ``run``, ``run_recorded``, ``rollout``, ``set_scene`` and ``status``.  The rows of scene g are bit for bit what
        an engine of n_g nodes computes for that scene alone (include/gnn_manip_hip.h states the one condition).  Rigid ranks are
        global: row j of a pose array belongs to the j-th rigid row of the assembled window, scene 0's first.  Up to 64 scenes;
        equal sizes are allowed.  ``step_backward`` and ``differentiable_rollout(sweep="library", record=, params=)`` run the
        library's ragged sweeps on it.  A ragged engine does not renumber (``renumber=True`` raises ValueError); ``differentiable_step``,
        ``sweep="autograd"`` and ``rollout_candidates`` raise ValueError on it."""
        self.model = model
        self.graph_attr = graph_attr
        self.candidates = int(candidates)
        self.offsets = self._offsets_host = None
        if sizes is not None:
            sizes = [int(v) for v in sizes]
            if n_nodes is not None or self.candidates != 1:
                raise ValueError("RolloutEngine: sizes= describes the whole batch; give neither n_nodes nor candidates with it")
            if not 1 <= len(sizes) <= 64 or min(sizes) < 1:
                raise ValueError(f"RolloutEngine: sizes must be 1..64 scenes of at least one node each, got {sizes}")
            if renumber is True:
                raise ValueError("RolloutEngine: a ragged engine (sizes=) does not renumber")
            renumber = False
            self.offsets = [0]
            for v in sizes:
                self.offsets.append(self.offsets[-1] + v)
            self._offsets_host = (C.c_int64 * len(self.offsets))(*self.offsets)   # read by the library during each call
            n_nodes = self.offsets[-1]
        elif n_nodes is None:
            raise ValueError("RolloutEngine needs n_nodes or sizes")
        self.sizes = sizes
        self.n_per = int(n_nodes)
        self.n = int(n_nodes) * self.candidates
        self.k = int(k_steps)
        self.device = torch.device(device)
        self.max_neighbours = int(max_neighbours)
        if data_dim is None:
            data_dim = (graph_attr.control_idx[-1] + 1) if graph_attr.control_idx is not None else graph_attr.cartesian_idx[-1] + 1
        self.data_dim = int(data_dim)
        self.fdesc = make_feature_desc(graph_attr.conn_r, graph_attr.stats, graph_attr.bounds, graph_attr.cartesian_idx,
                                       graph_attr.material_idx, graph_attr.control_idx, self.k, self.data_dim)
        self.fdesc.nodes_per_graph = self.n_per if self.candidates > 1 else 0
        self.mdesc = ModelDesc(*model.model_desc())
        L = lib()
        self.ws = _ws(L.gm_rollout_workspace_bytes(C.byref(self.mdesc), self.n, self.max_neighbours), self.device)
        self.rigid_rank = None
        self.rigid_rows = None   # int64 indices of the rigid rows, ascending (differentiable_step)
        self.n_rigid = 0
        if renumber == "auto" and os.environ.get("GM_RENUMBER") in ("0", "1"):   # A/B runs of the benchmark
            renumber = os.environ["GM_RENUMBER"] == "1"
        self.renumber = (self.n_per >= self.RENUMBER_MIN_NODES) if renumber == "auto" else bool(renumber)
        self._renumber_ws = None

    @property
    def ragged(self):
        return getattr(self, "sizes", None) is not None

    def rows(self, g):
        """The rows of scene g of a ragged engine's arrays, as a slice of the node axis."""
        if not self.ragged:
            raise ValueError("rows(g) is a ragged engine's (sizes=)")
        return slice(self.offsets[g], self.offsets[g + 1])

    def _no_ragged(self, what):
        if self.ragged:
            raise ValueError(f"RolloutEngine.{what} is not available on a ragged engine (sizes=)")

    def _rank_rigid(self, obs):
        rank = torch.empty(self.n, dtype=torch.int32, device=self.device)
        cnt = torch.zeros(1, dtype=torch.int32, device=self.device)
        check(lib().gm_rigid_rank(ptr(obs), self.n, C.byref(self.fdesc), ptr(rank), ptr(cnt), current_stream()))
        return rank, cnt

    def set_scene(self, obs):
        """Classify rigid rows (material == 1, rollout_utils.py:20) once per scene."""
        _need_cuda(obs, "obs")
        assert obs.shape == (self.k, self.n, self.data_dim) and obs.dtype == torch.float32 and obs.is_contiguous()
        self.rigid_rank, cnt = self._rank_rigid(obs)
        self.n_rigid = int(cnt.item())
        self.rigid_rows = torch.nonzero(self.rigid_rank >= 0).flatten()   # ascending: row j of a rigid_target belongs to rigid_rows[j]
        return self.n_rigid

    def _check_tensor(self, t, name, shape, converted=False, min_rows=0):
        """The C entries take raw pointers: `t` must be a tensor on this engine's device, float32 and contiguous, of exactly `shape`,
        else ValueError.  A string in `shape` names a dimension that is free (the first one from `min_rows` up); an int in place
        of the tuple is an element count, whatever the dimensions.  converted: any dtype and layout pass (the caller makes the
        contiguous float32 copy itself)."""
        fits = isinstance(t, torch.Tensor) and t.device == self.device and (converted or (t.dtype == torch.float32 and t.is_contiguous()))
        if fits and isinstance(shape, int):
            fits = t.numel() == shape
        elif fits and t.shape != shape:   # (equal: the common case, settled without looking at the entries)
            fits = (t.dim() == len(shape) and all(isinstance(want, str) or want == got for want, got in zip(shape, t.shape))
                    and t.shape[0] >= min_rows)
        if not fits:
            want = f"with {shape} elements" if isinstance(shape, int) else "[" + ", ".join(str(d) for d in shape) + "]"
            given = f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{name} must be {'a tensor' if converted else 'contiguous float32'} {want} on {self.device}, got {given}")

    def _check_state(self, obs, rigid_target, pred_out, use_rigid):
        self._check_tensor(obs, "obs", (self.k, self.n, self.data_dim))
        if use_rigid and self.rigid_rank is None:
            raise RuntimeError("RolloutEngine.set_scene(obs) must be called before step()")
        if rigid_target is not None:
            if not use_rigid:
                raise ValueError("rigid_target needs use_rigid=True")
            self._check_tensor(rigid_target, "rigid_target", (self.n_rigid, 3))
        if pred_out is not None:
            self._check_tensor(pred_out, "pred_out", self.n * 3)

    def step(self, obs, rigid_target=None, pred_out=None, use_rigid=True):
        """One rollout step in place on ``obs`` [k, N, D]; rigid_target: [N_rigid, 3] scripted pose or None."""
        self._check_state(obs, rigid_target, pred_out, use_rigid)
        handle = self.model.device_handle(self.device)
        rr = self.rigid_rank if use_rigid else None
        if self.ragged:
            check(lib().gm_rollout_step_ragged(handle, ptr(obs), self._offsets_host, len(self.sizes), C.byref(self.fdesc), self.max_neighbours,
                                               ptr(rr), ptr(rigid_target), ptr(pred_out), ptr(self.ws), self.ws.numel(), current_stream()))
            return
        check(lib().gm_rollout_step(handle, ptr(obs), self.n, C.byref(self.fdesc), self.max_neighbours, ptr(rr),
                                    ptr(rigid_target), ptr(pred_out), ptr(self.ws), self.ws.numel(), current_stream()))

    def differentiable_step(self, obs, rigid_target=None, inputs_only=False):
        """One rollout step OUT of place, under autograd: returns (next_obs [k, N, D], pred [N, 3], edge_index [2, E]); ``obs`` is
        untouched.  The chain is ``step``'s: state_pre -> node features -> radius graph -> edge features -> ``model.forward`` ->
        integrate -> state_post.  Gradients flow to ``obs`` (position and control columns) and to ``rigid_target``, through the
        model (gm_epd_backward_inputs) and the HIP backward of each feature function.

        The radius graph is a constant of the step: connectivity is piecewise constant in the positions, so its gradient is
        zero wherever it exists; the graph is built on the detached last frame and returned so that a caller (or a test) can
        hold a reference computation to the same edges.  The two state updates -- control columns and scripted pose of the rigid
        rows (``rigid_rows``, set_scene), the window shift -- are torch indexing operations on the device.  ``candidates`` > 1:
        the batched radius graph, as in ``step``.  The forward reads ONE number back from the device, the edge count that sizes
        ``edge_index`` / ``edge_attr``; nothing else in the forward and nothing in the backward synchronises with the host.

        inputs_only: the model's parameters are constants of the step whatever their requires_grad flags say
        (``EncProcDecGNN.forward_inputs_only``: no weight-gradient work in the backward, no parameter's ``.grad`` touched)."""
        self._no_ragged("differentiable_step")
        self._check_state(obs, rigid_target, None, True)
        ga = self.graph_attr
        c0 = ga.cartesian_idx[0]
        rows = self.rigid_rows
        last = obs[-1]
        if ga.control_idx is not None:   # state_pre: control of the rigid rows <- scripted pose - current xyz (no pose: current xyz)
            u0 = ga.control_idx[0]
            cur = last[rows, c0:c0 + 3]
            last = last.clone()
            last[rows, u0:u0 + 3] = cur if rigid_target is None else rigid_target - cur
        obs_pre = torch.cat((obs[:-1], last.unsqueeze(0)))
        if torch.is_grad_enabled() and obs_pre.requires_grad:
            nodes = _NodeFeaturesFunction.apply(obs_pre, self.fdesc)
        else:
            nodes = _node_features(obs_pre, self.fdesc)
        pos = obs_pre[-1][:, c0:c0 + 3]
        senders, receivers = get_connectivity(pos.detach(), ga.conn_r, self.max_neighbours,
                                              self.n_per if self.candidates > 1 else None)
        edge_attr = get_edges_displacement(pos, senders, receivers, ga.conn_r)
        edge_index = torch.stack((senders, receivers))
        pred = (self.model.forward_inputs_only if inputs_only else self.model.forward)(nodes, edge_attr, edge_index)
        next_pos = get_position_from_prediction(ga.stats, ga.cartesian_idx, pred, obs_pre, _desc=self.fdesc)
        # state_post: window shift; p_{t+1} into the last frame; a rigid row keeps its pre-step row, with the scripted pose if given
        new_last = obs_pre[-1].clone()
        new_last[:, c0:c0 + 3] = next_pos
        keep = obs_pre[-1][rows]
        if rigid_target is not None:
            keep = keep.clone()
            keep[:, c0:c0 + 3] = rigid_target
        new_last[rows] = keep
        return torch.cat((obs_pre[1:], new_last.unsqueeze(0))), pred, edge_index

    def _training_model(self):
        """(gm_model handle, its parameter tensors, their pointer array, descriptor) of the model as the training entry points run
        it (``EncProcDecGNN._training_spec``).  The parameters are constants here."""
        with torch.no_grad():
            desc_t, handle, tensors, key = self.model._training_spec([p.detach() for p in self.model.parameters()])
        h = handle.get(desc_t, tensors, self.device, key)
        return (h,) + _device_arrays(tensors, self.device) + (ModelDesc(*desc_t),)

    def _backward_ws(self, mdesc):
        """The reverse sweep's workspace (the step's is its head): sized by n and max_neighbours, allocated at first use."""
        need = lib().gm_rollout_backward_workspace_bytes(C.byref(mdesc), C.byref(self.fdesc), self.n, self.max_neighbours)
        if need == 0:
            raise ValueError("RolloutEngine: no backward workspace for these sizes")
        if getattr(self, "_bwd_ws", None) is None or self._bwd_ws.numel() < need:
            self._bwd_ws = _ws(need, self.device)
        return self._bwd_ws

    def _check_param_grads(self, grads, tensors):
        if len(grads) != len(tensors):
            raise ValueError(f"grads must be {len(tensors)} tensors shaped like the training model's, got {len(grads)}")
        for g, t in zip(grads, tensors):
            self._check_tensor(g, "each of grads", t.shape)
        return _pointers(grads)

    def step_backward(self, obs_before, rigid_target, d_obs_after, return_edge_count=False, d_record=None, grads=None):
        """The vector-Jacobian product of one ``step`` inside the library (gm_rollout_step_backward_train): (d_obs_before [k, N, D],
        d_rigid_target [N_rigid, 3] or None without a target) from the pre-step window, the step's scripted pose and the gradient
        with respect to the window the step left.  ``set_scene`` must have been called; ``obs_before`` is not written.  One host
        synchronisation (the edge count, returned third when asked for).

        d_record: [N, D] or None, the gradient with respect to the step's record (the last frame after the control overwrite,
        what ``run(record=True)`` keeps of this step); it is added inside the same launch that sums the step's contributions.
        grads: None -- the model's parameters are constants -- or a list of float32 tensors shaped like the model's parameters
        (hidden sizes 64 / 128 / 256; like ``_training_model``'s padded tensors otherwise), which the parameter gradients are
        ACCUMULATED into: the caller zeroes them.  The two returned gradients have the same bits with and without ``grads``."""
        self._check_state(obs_before, rigid_target, None, True)
        self._check_tensor(d_obs_after, "d_obs_after", (self.k, self.n, self.data_dim))
        if d_record is not None:
            self._check_tensor(d_record, "d_record", (self.n, self.data_dim))
        h, tensors, t_arr, mdesc = self._training_model()
        g_arr = None if grads is None else self._check_param_grads(grads, tensors)
        ws = self._backward_ws(mdesc)
        d_obs = torch.empty_like(obs_before)
        d_tgt = None if rigid_target is None else torch.empty_like(rigid_target)
        e = C.c_int64(0)
        tail = (C.byref(self.fdesc), self.max_neighbours, ptr(self.rigid_rank), ptr(rigid_target), ptr(d_obs_after), ptr(d_record), g_arr,
                ptr(d_obs), ptr(d_tgt), C.byref(e), ptr(ws), ws.numel(), current_stream())
        if self.ragged:
            check(lib().gm_rollout_step_backward_train_ragged(h, t_arr, len(tensors), ptr(obs_before), self._offsets_host, len(self.sizes), *tail))
        else:
            check(lib().gm_rollout_step_backward_train(h, t_arr, len(tensors), ptr(obs_before), self.n, *tail))
        return (d_obs, d_tgt, int(e.value)) if return_edge_count else (d_obs, d_tgt)

    def _sweep_backward(self, windows, traj, steps, d_final, scene, need_traj, d_records=None, model=None, grads=None):
        """gm_rollout_backward_train on the windows a forward kept: (d_obs0, d_trajectory or None).  d_records: [steps, N, D] or
        None.  model: the training model the sweep runs, as ``_training_model()`` returns it -- None for that one; grads: tensors
        shaped like its tensors that the parameter gradients are accumulated into, or None."""
        rank, n_rigid = scene
        self._check_tensor(d_final, "d_final", (self.k, self.n, self.data_dim))
        if traj is not None:
            self._check_tensor(traj, "trajectory", ("T", n_rigid, 3))
        self._check_tensor(windows, "windows", (steps, self.k, self.n, self.data_dim))
        if d_records is not None:
            self._check_tensor(d_records, "d_records", (steps, self.n, self.data_dim))
        h, tensors, t_arr, mdesc = self._training_model() if model is None else model
        g_arr = None if grads is None else self._check_param_grads(grads, tensors)
        ws = self._backward_ws(mdesc)
        d_obs0 = torch.empty_like(d_final)
        d_traj = torch.empty_like(traj) if need_traj else None
        n_targets = 0 if traj is None else int(traj.shape[0])
        tail = (C.byref(self.fdesc), self.max_neighbours, ptr(rank), ptr(traj), n_targets, n_rigid, steps, ptr(d_final), ptr(d_records), g_arr,
                ptr(d_obs0), ptr(d_traj), ptr(ws), ws.numel(), current_stream())
        if self.ragged:
            check(lib().gm_rollout_backward_train_ragged(h, t_arr, len(tensors), ptr(windows), self._offsets_host, len(self.sizes), *tail))
        else:
            check(lib().gm_rollout_backward_train(h, t_arr, len(tensors), ptr(windows), self.n, *tail))
        return d_obs0, d_traj

    def differentiable_rollout(self, obs0, trajectory=None, horizon=None, return_edges=False, sweep="autograd", record=False,
                               params=False):
        """``rollout(obs0, trajectory, horizon)`` under autograd: returns the final state [k, N, D], bit-equal to ``rollout``'s
        (an engine that renumbers, see ``renumber``, sums a node's messages in another order inside ``rollout``: equal to
        rounding there), with gradients to ``obs0`` (position and control columns) and to ``trajectory`` [T, N_rigid, 3].  The
        model's parameters are CONSTANTS of this function: they get no gradient, whatever their requires_grad flags say, and
        their ``.grad`` is not touched.  On a model switched to ``set_precision('f16')`` the forward visits the fp16 mode's windows and
        the backward differentiates the FLOAT32 step at them (the training kernels have one arithmetic): the gradients are those of
        the float32 model along the fp16 trajectory, and do not depend on the switch for given windows.

        Memory does not grow with the horizon beyond one state window per step.  The forward is the inference rollout (``step``
        in place on a clone, no tape) and keeps each step's pre-step window, k N D floats.  The backward walks the steps in
        reverse: it re-runs ``differentiable_step`` on step t's saved window (inputs only: none of the weight-gradient work),
        feeds it the gradient with respect to the window after step t, and takes the gradient with respect to the window before
        it and to ``trajectory[t]``.  One step's tape is alive at a time.  Each recomputed step reads its edge count back from
        the device (the limit of ``differentiable_step``); the forward synchronises once, at its end.

        return_edges: the call returns (final state, edges), where ``edges`` is a list that the BACKWARD fills with the T
        ``edge_index`` tensors [2, E_t] of its recomputation (empty until then), so that a reference computation can be held to
        the same graphs.  ``candidates`` > 1 works as in ``differentiable_step``.

        sweep: "autograd" (the default) is the backward described above.  "library" keeps the windows in one [T, k, N, D] array and
        runs the whole reverse sweep as ONE library call (gm_rollout_backward: per step the same forward and backward entry
        points, the state updates' transposes and the sum of the contributions as HIP kernels, no autograd node and no Python
        between steps; still one edge-count read per step).  It hands out no edge lists: ``return_edges`` raises ValueError.

        record, params (sweep="library" only; ValueError otherwise): what a multi-step TRAINING loss needs.  record=True returns
        (final state, records [T, N, D]), both differentiable: ``rollout(..., record=True)``'s records (bit-equal on an engine
        that does not renumber), read off the windows the forward passes through anyway -- record t is frame k-2 of the state
        after step t.  params=True makes the model's parameters inputs of the rollout: the sweep accumulates their gradients
        over the steps (gm_rollout_backward_train, step T-1 first, step 0 last, no atomics) and they arrive in ``.grad`` like any
        other tensor's -- in the checkpoint's own shapes at a hidden size between 64 / 128 / 256 too, where the zero-padded tensors
        are built under autograd as in ``EncProcDecGNN.forward``; ``obs0`` need not require grad.  Peak memory still grows with
        the horizon only by the windows (and the records asked for): one tape and one set of parameter gradients are alive."""
        if sweep not in ("autograd", "library"):
            raise ValueError(f"sweep must be 'autograd' or 'library', got {sweep!r}")
        if sweep == "library" and return_edges:
            raise ValueError("sweep='library' hands out no edge lists: return_edges needs sweep='autograd'")
        if sweep != "library" and (record or params):
            raise ValueError("record=True / params=True need sweep='library' (the autograd sweep returns the final state alone, "
                             "with the parameters as constants)")
        if self.ragged and sweep != "library":
            raise ValueError("a ragged engine (sizes=) has the library's sweep only: differentiable_rollout(sweep='library')")
        steps = int(horizon) if horizon is not None else (int(trajectory.shape[0]) if trajectory is not None else 0)
        self._check_state(obs0, None, None, False)
        if trajectory is not None:
            self._check_tensor(trajectory, "trajectory", (f"T >= {steps}", "N_rigid", 3), converted=True, min_rows=steps)
        if sweep == "library":
            model, tensors = None, ()
            if params:   # the LIVE parameters: padded tensors are functions of them, and autograd takes the gradients back through those
                desc_t, handle, tensors, key = self.model._training_spec(list(self.model.parameters()))
                model = (handle.get(desc_t, tensors, self.device, key), ModelDesc(*desc_t))
            return _RolloutTrainFunction.apply(self, obs0, trajectory, steps, bool(record), model, *tensors)
        edges = [] if return_edges else None
        out = _RolloutFunction.apply(self, obs0, trajectory, steps, edges)
        return (out, edges) if return_edges else out

    def status(self):
        """Synchronises; raises on a device-side data error; returns the last step's edge count."""
        e = C.c_int64(0)
        check(lib().gm_rollout_status(ptr(self.ws), C.byref(self.mdesc), self.n, self.max_neighbours, C.byref(e), current_stream()))
        return int(e.value)

    def run(self, obs, trajectory=None, steps=None, record=False):
        """`steps` rollout steps in place on ``obs`` inside ONE library call (gm_rollout): no Python between steps.
        trajectory: [T, N_rigid, 3] contiguous device tensor of scripted poses or None.  Returns the recorded last
        frames [steps, N, D] when asked (the reference's per-step record), else None."""
        T = 0 if trajectory is None else int(trajectory.shape[0])
        steps = T if steps is None else int(steps)
        self._check_state(obs, None, None, True)
        if trajectory is not None:
            self._check_tensor(trajectory, "trajectory", ("T", self.n_rigid, 3))
        recs = torch.empty((steps, self.n, self.data_dim), dtype=torch.float32, device=self.device) if record else None
        handle = self.model.device_handle(self.device)  # resolved once per rollout
        if self.ragged:
            check(lib().gm_rollout_ragged(handle, ptr(obs), self._offsets_host, len(self.sizes), C.byref(self.fdesc), self.max_neighbours,
                                          ptr(self.rigid_rank), ptr(trajectory), T, self.n_rigid, steps, ptr(recs), ptr(self.ws),
                                          self.ws.numel(), current_stream()))
            return recs
        every, rws = self._renumbering(steps)
        check(lib().gm_rollout(handle, ptr(obs), self.n, C.byref(self.fdesc), self.max_neighbours, ptr(self.rigid_rank),
                           ptr(trajectory), T, self.n_rigid, steps, ptr(recs), every, ptr(rws), 0 if rws is None else rws.numel(),
                           ptr(self.ws), self.ws.numel(), current_stream()))
        return recs

    def _renumbering(self, steps):
        """(renumber_every, renumber workspace or None) of a library rollout of `steps` steps: rows in grid-cell order inside the
        library -- order, row maps, gathers and the write-back are device kernels of the same call, nothing is sorted or
        synchronised here."""
        if not (self.renumber and self.n > 0 and steps > 0):
            return 0, None
        if self._renumber_ws is None:
            self._renumber_ws = _ws(lib().gm_rollout_renumber_workspace_bytes(C.byref(self.fdesc), self.n), self.device)
        return self.RENUMBER_EVERY, self._renumber_ws

    def run_recorded(self, obs, frames, steps=None, record=False, record_pred=False):
        """`steps` steps of compute_rollout's ground-truth loop (rollout_utils.py:38-61 with ``args.cma_traj`` None) in place on
        ``obs`` inside ONE library call (gm_rollout_recorded): before step i the control columns of the rigid rows take those of
        ``frames[i]``, after it their xyz takes that of the same ``frames[i]`` (the reference's pose lags the window by one step).
        frames: [T, N, D] contiguous device tensor of recorded frames, T >= steps (default: all of them).  Returns
        (records [steps, N, D] -- the last frame after each control overwrite, the reference's ``prediction`` -- or None,
        predictions [steps, N, 3] -- the model's normalised acceleration of each step -- or None).  The same checks and the same
        renumbering as ``run``; no host synchronisation."""
        self._check_state(obs, None, None, True)
        self._check_tensor(frames, "frames", ("T", self.n, self.data_dim))
        steps = int(frames.shape[0]) if steps is None else int(steps)
        if not 0 <= steps <= frames.shape[0]:
            raise ValueError(f"steps must be between 0 and the {frames.shape[0]} frames given, got {steps}")
        recs = torch.empty((steps, self.n, self.data_dim), dtype=torch.float32, device=self.device) if record else None
        preds = torch.empty((steps, self.n, 3), dtype=torch.float32, device=self.device) if record_pred else None
        handle = self.model.device_handle(self.device)
        if self.ragged:
            check(lib().gm_rollout_recorded_ragged(handle, ptr(obs), self._offsets_host, len(self.sizes), C.byref(self.fdesc),
                                                   self.max_neighbours, ptr(self.rigid_rank), ptr(frames), steps, ptr(recs), ptr(preds),
                                                   ptr(self.ws), self.ws.numel(), current_stream()))
            return recs, preds
        every, rws = self._renumbering(steps)
        check(lib().gm_rollout_recorded(handle, ptr(obs), self.n, C.byref(self.fdesc), self.max_neighbours, ptr(self.rigid_rank),
                                        ptr(frames), steps, ptr(recs), ptr(preds), every, ptr(rws), 0 if rws is None else rws.numel(),
                                        ptr(self.ws), self.ws.numel(), current_stream()))
        return recs, preds

    def rollout_candidates(self, obs0, trajectories, horizon=None):
        """Roll `candidates` copies of one initial state [k, N, D] under per-candidate scripted rigid poses
        `trajectories` [B, T, N_rigid, 3] (the CMA-ES population of traj_utils.py:247-259, evaluated together
        instead of serially).  Returns the final states [B, k, N, D]."""
        self._no_ragged("rollout_candidates")
        b, k, n = self.candidates, self.k, self.n_per
        assert trajectories.shape[0] == b
        obs = obs0.unsqueeze(1).repeat(1, b, 1, 1).reshape(k, b * n, self.data_dim).contiguous()
        self.set_scene(obs)
        steps = horizon if horizon is not None else trajectories.shape[1]
        # [T, B * Nr, 3]: one step's poses of all candidates are contiguous, candidate-major like the rigid rows
        traj_t = trajectories.permute(1, 0, 2, 3).reshape(trajectories.shape[1], -1, 3).contiguous().float()
        self.run(obs, traj_t, steps)
        self.status()
        return obs.reshape(k, b, n, self.data_dim).permute(1, 0, 2, 3).contiguous()

    def rollout(self, obs0, trajectory=None, horizon=None, record=False):
        """cma_objective's loop (traj_utils.py:119-152).  trajectory: [T, N_rigid, 3] device tensor of scripted
        rigid poses (or None: no rigid overwrite).  Returns the final state (and the recorded last frames)."""
        obs = obs0.clone().contiguous()
        self.set_scene(obs)  # per call: the engine may be given another scene
        steps = horizon if horizon is not None else (trajectory.shape[0] if trajectory is not None else 0)
        traj = None if trajectory is None else trajectory.contiguous().float()
        recs = self.run(obs, traj, steps, record=record)
        self.status()
        if record:
            return obs, recs
        return obs


def get_rigid_body_trajectory_from_diff(trajectory, horizon, ty_init, rigid_particles):
    """rollout_utils.py:160-174: absolute (rotation [rad], translation) pairs -> [horizon, N_rigid, 3] poses on the device."""
    from .planner import get_rigid_body_trajectory
    return get_rigid_body_trajectory(trajectory[:, 0], trajectory[:, 1], horizon, ty_init, rigid_particles)


def extract_groundtruth(dataset, nof_steps, nof_particles=None, data_dim=None):
    """rollout_utils.py:84-93: last frame of every window, [nof_steps, N, D] (device)."""
    return torch.stack([dataset[i][0][-1] for i in range(nof_steps)]).float()


def compute_rollout(dataset, model, args):
    """Mirror of ``compute_rollout`` (rollout_utils.py:12-67): roll the model out from the first window of a
    ``CoffeeTestDataset``, driving the rigid body either with a planned trajectory (``args.cma_traj``: .npy of
    absolute [rotation, translation] per step) or with the recorded ground truth.  Returns the reference's
    ``prediction`` array [nof_steps, N, D] (numpy): the last frame of every step after the control overwrite.
    Both modes are one library call: gm_rollout under the planned poses, gm_rollout_recorded under the recorded frames
    (``RolloutEngine.run_recorded``) -- no Python and no host synchronisation between steps."""
    import numpy as np
    obs0, _ = dataset[0]
    k, n, dd = obs0.shape
    dev = obs0.device
    nof_steps = dataset.time_steps if args.cma_traj is not None else dataset.time_steps - args.k_steps
    # the ground-truth mode never renumbered (it stepped through gm_rollout_step): its records keep their bits at every size
    eng = RolloutEngine(model, dataset.graph_attr, n, k_steps=k, data_dim=dd, max_neighbours=20, device=dev,
                        renumber="auto" if args.cma_traj is not None else False)
    obs = obs0.clone().contiguous()
    eng.set_scene(obs)
    rigid = obs[0, :, dataset.material_id] == 1
    c0 = dataset.cartesian_idx[0]
    with torch.no_grad():
        if args.cma_traj is not None:
            npy_trajectory = np.load(args.cma_traj) if isinstance(args.cma_traj, str) else np.asarray(args.cma_traj)
            rigid_pos = obs[-1, rigid, c0:c0 + 3].contiguous()
            trajectory = get_rigid_body_trajectory_from_diff(npy_trajectory, nof_steps, [0.5, 0.5, 0.4], rigid_pos)
            _, recs = eng.rollout(obs, trajectory, horizon=nof_steps, record=True)
            return recs.cpu().numpy().astype(np.float64)
        groundtruth = extract_groundtruth(dataset, nof_steps).contiguous()
        # per step: control from the recording (:45), record, predict / integrate / shift, the recorded pose (:60)
        recs, _ = eng.run_recorded(obs, groundtruth, nof_steps, record=True)
        eng.status()
        return recs.cpu().numpy().astype(np.float64)


# SamplesLoss.batched over (step, simulation) pairs: the default block keeps gm_sinkhorn_batched_workspace_bytes under this
SINKHORN_WORKSPACE_CAP = 1 << 30


def _recorded_frames(sim, graph_attr, material_id):
    """A resident simulation [T, N, D0] as the windows' frames [T, N, D]: with control columns in the layout, frame t gets the
    control input of coffee_dataset.py:91-97 -- xyz[t + 1] - xyz[t] on the rigid rows (material == 1), 0 elsewhere and on the
    last frame -- so that frame t is ``dataset[t - k + 1][0][-1]``, bit for bit."""
    sim = sim.float()
    if graph_attr.control_idx is None:
        return sim.contiguous()
    c0 = graph_attr.cartesian_idx[0]
    ctr = torch.zeros(sim.shape[:2] + (3,), dtype=torch.float32, device=sim.device)
    ctr[:-1] = sim[1:, :, c0:c0 + 3] - sim[:-1, :, c0:c0 + 3]
    ctr = torch.where((sim[:, :, material_id] != 1).unsqueeze(-1), torch.zeros_like(ctr), ctr)
    return torch.cat((sim, ctr), dim=-1).contiguous()


def evaluate_rollout(dataset_or_sims, model, graph_attr=None, k_steps=6, max_neighbours=20, sinkhorn=True, blur=0.05, pair_block=None,
                     ragged=False):
    """How good is ``model`` on recorded simulations: the numbers of the reference's model comparison
    (scripts/plot_rmses.py:176-198), computed on the device.

    dataset_or_sims: a ``CoffeeTestDataset`` (its ``sims``, ``graph_attr`` and window length are used) or a list of resident
    [T, N, D] float32 device tensors with ``graph_attr`` given.  Each simulation is rolled T - k steps from its first window under
    the recorded drive (``RolloutEngine.run_recorded``: compute_rollout's ground-truth mode).  Simulations of equal (T, N) are
    evaluated together as one block-diagonal batch, others in groups of their own, in the order they first appear; one
    ``status()`` per group, after its rollout.  ragged=True: simulations of equal T on one device form ONE group whatever their N
    (at most 64 to a group), rolled as a ragged batch -- one engine (``RolloutEngine(sizes=...)``), one ``run_recorded``, one
    ``status()`` and one gm_rollout_errors_ragged per group; every tensor and every float returned is the default call's, bit for
    bit.  The Sinkhorn part groups the clouds by their number of coffee rows either way.

    Returns a list, one dict per simulation, in the order given:
      prediction, groundtruth   [steps, N, D] device tensors: the records of the rollout (the reference's ``prediction``) and
                                the recorded frames they stand against (``extract_groundtruth``); ``prediction[0]`` is
                                ``groundtruth[0]`` exactly;
      acceleration              [steps, N, 3] device tensor: the model's normalised acceleration of every step;
      sums                     [steps, 4] float64 host tensor, gm_rollout_errors' per-step sums: squared position error over
                                all rows, over the coffee rows (material == 0), squared error of the normalised acceleration
                                over the coffee rows, number of coffee rows;
      rmse_position, rmse_position_coffee, rmse_acceleration
                                floats formed on the host in float64 from the sums: sqrt(sum over steps and rows of |delta|^2 /
                                (steps * rows)), |delta| the 3-vector's norm.  The reference's ``get_rmse`` lives in a module
                                (``rollout_sand_dyn``) that is not in its tree: this definition is the engine's own and
                                UNPINNED against the reference.  NaN where there is no row to average over;
      sinkhorn, mean_sinkhorn   (sinkhorn=True) [steps] float32 device tensor and its mean as a float: entry i is
                                ``SamplesLoss("sinkhorn", p=2, blur=blur)(groundtruth_i[coffee, xyz], prediction_i[coffee, xyz])``,
                                the argument order of plot_rmses.py:188-191, bit-equal to that single call; None / NaN for a
                                simulation without coffee rows.
    pair_block: how many (step, simulation) pairs of a group one ``SamplesLoss.batched`` call takes, each pair with its own
    right-hand cloud (y_shared = 0); any value gives the same bits.  Default: as many as keep the call's workspace
    (gm_sinkhorn_batched_workspace_bytes) under SINKHORN_WORKSPACE_CAP (1 GiB), at least one.  The coffee rows are compacted into
    clouds with tensor indexing once per simulation, not per step; simulations of a group with equally many coffee rows share
    the calls."""
    from .losses import SamplesLoss
    if hasattr(dataset_or_sims, "sims"):
        sims, k = list(dataset_or_sims.sims), int(dataset_or_sims.k)
        graph_attr = dataset_or_sims.graph_attr if graph_attr is None else graph_attr
    else:
        sims, k = list(dataset_or_sims), int(k_steps)
    if graph_attr is None:
        raise ValueError("evaluate_rollout: a list of simulations needs graph_attr")
    mat, c0 = graph_attr.material_idx[0], graph_attr.cartesian_idx[0]
    groups = {}
    for s, sim in enumerate(sims):
        _need_cuda(sim, "every simulation")
        if sim.dim() != 3 or sim.shape[0] <= k:
            raise ValueError(f"evaluate_rollout: simulation {s} must be [T > {k}, N, D], got {tuple(sim.shape)}")
        key = (int(sim.shape[0]), None if ragged else int(sim.shape[1]), sim.device)
        part = 0   # a ragged group takes what one table holds; the simulations beyond it open the next group
        while ragged and len(groups.get(key + (part,), ())) >= 64:
            part += 1
        groups.setdefault(key + (part,), []).append(s)
    loss = SamplesLoss("sinkhorn", p=2, blur=blur) if sinkhorn else None
    results = [None] * len(sims)
    with torch.no_grad():
        for (T, _, dev, _), members in groups.items():
            G, steps = len(members), T - k
            off = [0]
            for s in members:
                off.append(off[-1] + int(sims[s].shape[1]))
            # the group's recording, simulations back to back along the node axis: [T, G * n, D]
            rec = torch.cat([_recorded_frames(sims[s], graph_attr, mat) for s in members], dim=1).contiguous()
            dd = int(rec.shape[2])
            if ragged:
                eng = RolloutEngine(model, graph_attr, k_steps=k, data_dim=dd, max_neighbours=max_neighbours, device=dev,
                                    sizes=[b - a for a, b in zip(off, off[1:])])
            else:
                eng = RolloutEngine(model, graph_attr, off[1], k_steps=k, data_dim=dd, max_neighbours=max_neighbours, device=dev, candidates=G)
            obs = rec[:k].clone().contiguous()
            if graph_attr.control_idx is not None:   # the first window as the dataset stores it: every frame's control looks at frame k
                u0 = graph_attr.control_idx[0]
                way = rec[k, :, c0:c0 + 3].unsqueeze(0) - obs[:, :, c0:c0 + 3]
                obs[:, :, u0:u0 + 3] = torch.where((obs[:, :, mat] != 1).unsqueeze(-1), torch.zeros_like(way), way)
            eng.set_scene(obs)
            frames = rec[k - 1:k - 1 + steps]
            pred, acc = eng.run_recorded(obs, frames, steps, record=True, record_pred=True)
            eng.status()
            sums = torch.empty((steps, G, 4), dtype=torch.float64, device=dev)
            if ragged:
                check(lib().gm_rollout_errors_ragged(ptr(pred), ptr(acc), ptr(rec), T, k - 1, steps, eng._offsets_host, G, C.byref(eng.fdesc),
                                                     ptr(sums), current_stream()))
            else:
                check(lib().gm_rollout_errors(ptr(pred), ptr(acc), ptr(rec), T, k - 1, steps, eng.n, C.byref(eng.fdesc), ptr(sums),
                                              current_stream()))
            sums = sums.cpu()
            coffee = rec[0, :, mat] == 0
            for g, s in enumerate(members):
                rows, n = slice(off[g], off[g + 1]), off[g + 1] - off[g]
                res = dict(prediction=pred[:, rows], groundtruth=frames[:, rows], acceleration=acc[:, rows], sums=sums[:, g].clone())
                tot = res["sums"].sum(dim=0)
                cnt = float(res["sums"][0, 3])
                mean = lambda v, rows_: float(torch.sqrt(v / (steps * rows_))) if steps * rows_ > 0 else float("nan")
                res["rmse_position"] = mean(tot[0], n)
                res["rmse_position_coffee"] = mean(tot[1], cnt)
                res["rmse_acceleration"] = mean(tot[2], cnt)
                if sinkhorn:
                    res["sinkhorn"], res["mean_sinkhorn"] = None, float("nan")
                results[s] = res
            if not sinkhorn or steps == 0:
                continue
            # the (step, simulation) pairs of the group: the coffee rows of a simulation compacted once, simulations with equally
            # many of them stacked into one list of pairs, which goes through SamplesLoss.batched block by block
            clouds = {}
            for g, s in enumerate(members):
                idx = torch.nonzero(coffee[off[g]:off[g + 1]]).flatten() + off[g]
                if idx.numel() > 0:
                    clouds.setdefault(int(idx.numel()), []).append((s, idx))
            for nc, items in clouds.items():
                x = torch.cat([frames[:, idx, c0:c0 + 3] for _, idx in items]).contiguous()     # [S * steps, Nc, 3] ground truth
                y = torch.cat([pred[:, idx, c0:c0 + 3] for _, idx in items]).contiguous()       # [S * steps, Nc, 3] prediction
                pairs = int(x.shape[0])
                block = pair_block
                if block is None:
                    block = pairs
                    while block > 1 and lib().gm_sinkhorn_batched_workspace_bytes(block, nc, nc) > SINKHORN_WORKSPACE_CAP:
                        block = (block + 1) // 2
                block = max(1, int(block))
                losses = torch.cat([loss.batched(x[b:b + block], y[b:b + block]) for b in range(0, pairs, block)])
                for j, (s, _) in enumerate(items):
                    results[s]["sinkhorn"] = losses[j * steps:(j + 1) * steps]
                    results[s]["mean_sinkhorn"] = float(results[s]["sinkhorn"].double().mean())
    return results
