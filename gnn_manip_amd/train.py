"""The training step of examples/train_dyn.py:49-72 in the library: ``Trainer`` owns a gm_model built from a module's parameters
and a gm_trainer (Adam's moments, the gradients, a device record) and runs forward, L1 loss, backward and Adam as ONE library call
per batch (gm_train_step) -- no autograd graph, no optimiser object, no host synchronisation.  The arithmetic of the loss and of
Adam is the contract stated in include/gnn_manip_hip.h.

The two learning-rate schedules of train_dyn.py:100-107,143-144 are one-line host formulas on ``trainer.lr``."""
import ctypes as C

import numpy as np
import torch

from ._lib import RAGGED_MAX_GRAPHS, GMError, ModelDesc, check, current_stream, lib, ptr
from .dataset import GraphData
from .epd_gnn import TRAIN_WIDTHS, DstCsr, _check_edge_index, _device_arrays, _Model, _pointers
from .graph import _need_cuda, _ws

PARAMS, EXP_AVG, EXP_AVG_SQ, GRADS = 1, 2, 3, 4   # GM_TRAINER_* of include/gnn_manip_hip.h


def normalise_material_col(material_col, node_dim):
    """The column of the node features that holds the material flag, as the library takes it: the reference indexes it from the
    end (train_dyn.py:60: ``-1 - len(control_idx)``, or ``-1`` without control columns)."""
    col = int(material_col)
    if col < 0:
        col += int(node_dim)
    if not 0 <= col < int(node_dim):
        raise ValueError(f"material_col={material_col} is outside the {node_dim} node feature columns")
    return col


def adam_state_dict(exp_avg, exp_avg_sq, step, lr, betas, eps):
    """``torch.optim.Adam.state_dict()``'s layout for one parameter group over ``len(exp_avg)`` parameters: what
    train_dyn.py:33-43 stores in a checkpoint, so that a run resumes in either direction."""
    ref = torch.optim.Adam([torch.zeros(1)], lr=float(lr), betas=tuple(float(b) for b in betas), eps=float(eps))
    group = dict(ref.state_dict()["param_groups"][0])     # every hyper-parameter key this torch's Adam expects, at its default
    group["params"] = list(range(len(exp_avg)))
    state = {i: {"step": torch.tensor(float(step)), "exp_avg": m, "exp_avg_sq": v} for i, (m, v) in enumerate(zip(exp_avg, exp_avg_sq))}
    return {"state": state, "param_groups": [group]}


def parse_adam_state_dict(sd, shapes):
    """The other direction: (exp_avg list or None, exp_avg_sq list or None, step, param group) of an Adam state_dict over parameters
    of `shapes`.  An optimiser that has not stepped has an empty state: the moments are then None (zeros) and step is 0."""
    groups = sd["param_groups"]
    if len(groups) != 1 or len(groups[0]["params"]) != len(shapes):
        raise ValueError(f"Trainer.load_state_dict: expected one parameter group of {len(shapes)} parameters")
    g = groups[0]
    if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
        raise ValueError("Trainer.load_state_dict: weight decay, AMSGrad and maximize are not part of the library's Adam")
    state = sd["state"]
    if len(state) == 0:
        return None, None, 0, g
    if sorted(state) != list(range(len(shapes))):
        raise ValueError("Trainer.load_state_dict: the state does not cover every parameter")
    steps = {int(float(state[i]["step"])) for i in range(len(shapes))}
    if len(steps) != 1:
        raise ValueError(f"Trainer.load_state_dict: the parameters disagree on the step count: {sorted(steps)}")
    for i, shape in enumerate(shapes):
        for key in ("exp_avg", "exp_avg_sq"):
            if tuple(state[i][key].shape) != tuple(shape):
                raise ValueError(f"Trainer.load_state_dict: {key} of parameter {i} has shape {tuple(state[i][key].shape)}, not {tuple(shape)}")
    return [state[i]["exp_avg"] for i in range(len(shapes))], [state[i]["exp_avg_sq"] for i in range(len(shapes))], steps.pop(), g


def exchange_bytes(local, gathered, group=None, staging=None):
    """The byte exchange of data-parallel training, and nothing else (no library call): every rank's ``local`` [bytes] arrives as
    row r of ``gathered`` [world, bytes] on every rank, in rank order.  Device tensors go through ``all_gather_into_tensor`` (RCCL):
    stream-ordered, nothing waits on the host.  Host tensors go through ``all_gather`` (gloo).  ``staging`` = (pinned [bytes],
    pinned [world, bytes]): device tensors are staged through these for a host collective -- the planner's rehearsal pattern --
    which synchronises."""
    import torch.distributed as dist
    if staging is not None:
        host_local, host_all = staging
        host_local.copy_(local)                                      # waits for the stream: the payload is complete
        dist.all_gather(list(host_all.unbind(0)), host_local, group=group)
        gathered.copy_(host_all, non_blocking=True)
    elif local.is_cuda:
        dist.all_gather_into_tensor(gathered.view(-1), local, group=group)
    else:
        dist.all_gather(list(gathered.unbind(0)), local, group=group)
    return gathered


class _Replicas:
    """What ``Trainer.distribute`` leaves on a trainer: the group, this rank in it, and the exchange buffers, allocated once."""

    def __init__(self, group, world, rank, nbytes, device, host):
        self.group, self.world, self.rank, self.host = group, world, rank, host
        self.local = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.gathered = torch.empty((world, nbytes), dtype=torch.uint8, device=device)
        self.staging = None
        if host:
            self.staging = (torch.empty(nbytes, dtype=torch.uint8).pin_memory(), torch.empty((world, nbytes), dtype=torch.uint8).pin_memory())


class _TrainerHandle:
    """A gm_trainer* and the gm_model it updates: the trainer is destroyed first."""

    def __init__(self, pointer, model):
        self._as_parameter_, self.model = pointer, model

    def __del__(self):
        try:
            lib().gm_trainer_destroy(self._as_parameter_)
        except Exception:
            pass
        self.model = None


class Trainer:
    """``Trainer(model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, sand_only=False, material_col=None)``: Adam on an ``EncProcDecGNN``
    with the L1 loss of train_dyn.py:58-65 -- ``sand_only`` is ``--use_updated_loss`` (the loss over the rows whose node feature
    ``material_col`` is below 0.5, divided by their count; ``material_col`` may be the reference's negative index).

    The trainer builds its OWN library model from the module's parameters, on the module's device, and trains that: the module's
    ``nn.Parameter`` s do not move until ``sync_module()`` copies the weights back.  ``step`` returns nothing and synchronises
    nothing: the loss goes into a slot on the device (``last_loss``, or the ``loss_out`` the caller passes); ``fit_epoch`` /
    ``eval_epoch`` return an epoch's losses after one synchronisation at its end.  ``lr`` is a plain attribute: set it between steps.

    A step whose edge_index holds an entry outside [0, N), or whose loss is not finite, is SKIPPED on the device: weights, moments
    and step count stay as they were, ``record()`` counts it, its loss slot holds NaN.  The edge_index error itself surfaces as
    ``GMError`` at a later step or at ``status()``, like a training forward's.

    ``step_rollout`` / ``evaluate_rollout`` / ``fit_rollout_epoch`` are the same for the other training mode, a loss on every
    frame of a T-step rollout against a recording: one library call per sample (gm_train_rollout_step).

    MINI-BATCHES AND THE CLIP.  ``zero_grad()``, then ``accumulate(batch)`` / ``accumulate_rollout(...)`` any
    number of times, then ``apply()``: one update from the MEAN of the samples' gradients, its norm clipped to ``max_grad_norm`` by
    ``torch.nn.utils.clip_grad_norm_``'s formula (a plain attribute like ``lr``, set after construction; None: no clip).  With
    ``max_grad_norm`` set, ``step`` and ``step_rollout`` are those three calls on one sample; with None they are the single
    library call.  One skipped sample skips its whole mini-batch.  ``fit_epoch(loader, accumulate=B)`` / ``fit_rollout_epoch(..., batch_size=B)`` run epochs
    of such mini-batches.  The clip is not part of ``state_dict()``.

    SEVERAL GPUS.  ``distribute()`` under ``torch.distributed`` makes the trainer one of ``world`` replicas:
    ``apply(samples_total=S)`` then merges the ranks' mini-batches before the update -- ``contribution()``, one all-gather,
    ``reduce()``: a float32 sum of the gradients in RANK ORDER, so every rank applies the same bits whatever the collective does --
    and ``fit_epoch`` / ``fit_rollout_epoch`` shard every mini-batch over the ranks.  A trainer that is never distributed runs
    exactly what it ran before.

    Hidden sizes 64 / 128 / 256 only.  A module of another hidden size trains zero-padded through ``model.forward`` under autograd
    with a torch optimiser (``EncProcDecGNN._padded_training``): that path stays with autograd."""

    max_grad_norm = None   # a plain attribute like ``lr``, set after construction: the clip of ``apply`` (None: no clip)

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, sand_only=False, material_col=None):
        if model.dims[3] not in TRAIN_WIDTHS:
            raise ValueError(f"Trainer: hidden_size={model.dims[3]}; the library step runs at hidden sizes 64, 128 and 256 "
                             "(other sizes train through model.forward under autograd)")
        self.model, self.lr = model, float(lr)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.sand_only = bool(sand_only)
        if self.sand_only and material_col is None:
            raise ValueError("Trainer: sand_only needs material_col, the node feature column of the material flag")
        self.mask_col = normalise_material_col(material_col, model.dims[0]) if self.sand_only else -1
        params = list(model.parameters())
        self.device = params[0].device
        _need_cuda(params[0], "the model's parameters")
        self._shapes = [tuple(p.shape) for p in params]
        self.desc = ModelDesc(*model.model_desc())
        L = lib()
        tensors, arr = _device_arrays(params, self.device)
        with torch.cuda.device(self.device):
            stream = current_stream(self.device)
            out = C.c_void_p()
            check(L.gm_model_create(C.byref(self.desc), arr, len(tensors), 1, stream, C.byref(out)))
            gm_model = _Model(out)
            out = C.c_void_p()
            check(L.gm_trainer_create(gm_model, self.betas[0], self.betas[1], self.eps, stream, C.byref(out)))
        self._h = _TrainerHandle(out, gm_model)
        self._ws = None
        self._rollout_ws, self._kept = None, None   # step_rollout's workspace and the shape of the windows at its head
        # a rollout batch's losses, given no losses_out: one per graph up to the library's cap
        self._batch_losses = torch.empty(RAGGED_MAX_GRAPHS, dtype=torch.float64, device=self.device)
        self._loss = torch.full((1,), float("nan"), dtype=torch.float64, device=self.device)
        self._loss_ws = _ws(L.gm_l1_loss_workspace_bytes(1, 1), self.device)
        self._pin_record = torch.zeros(4, dtype=torch.int64).pin_memory()
        self._pin_accum = torch.zeros(6, dtype=torch.int64).pin_memory()
        self._pin_losses = None
        self._grad_norm = torch.full((1,), float("nan"), dtype=torch.float64, device=self.device)
        self.last_epoch_grad_norms = None
        self._dp, self._dp_error = None, None       # distribute(): the replicas' exchange; a sample's GMError kept until apply

    # ------------------------------------------------------------------------------------------ one batch
    @property
    def last_loss(self):
        """The loss of the last ``step`` / ``evaluate`` that was given no ``loss_out``: a float64 device tensor of one element."""
        return self._loss

    def _batch(self, x, edge_attr, edge_index, y):
        if isinstance(x, GraphData):
            x, edge_attr, edge_index, y = x.x, x.edge_attr, x.edge_index, x.y
        _need_cuda(x, "x")
        x, edge_attr, y = x.contiguous().float(), edge_attr.contiguous().float(), y.contiguous().float()
        n, e = int(x.shape[0]), int(edge_attr.shape[0])
        if x.shape[1] != self.model.dims[0] or edge_attr.shape[1] != self.model.dims[1]:
            raise ValueError("x / edge_attr feature widths do not match the model")
        if tuple(y.shape) != (n, self.model.dims[2]):
            raise ValueError(f"y must be [{n}, {self.model.dims[2]}]")
        _check_edge_index(edge_index, n, e, ranges=False)
        return x, edge_attr, edge_index.contiguous(), y, n, e

    def _slot(self, loss_out):
        if loss_out is None:
            return self._loss
        if loss_out.dtype != torch.float64 or loss_out.numel() != 1 or loss_out.device != self.device:
            raise ValueError("loss_out must be one float64 element on the trainer's device")
        return loss_out

    def step(self, x, edge_attr=None, edge_index=None, y=None, loss_out=None):
        """One training step on a batch (four tensors, or a ``GraphData``): gm_train_step.  Nothing is returned and nothing waits."""
        self._not_distributed("step")
        if self.max_grad_norm is not None:
            self.zero_grad()
            self.accumulate(x, edge_attr, edge_index, y)
            return self.apply(loss_out=loss_out)
        self._one_batch(x, edge_attr, edge_index, y, self._slot(loss_out), True)

    def _one_batch(self, x, edge_attr, edge_index, y, slot, update):
        """gm_train_step (update) or gm_train_step_accumulate on a checked batch; slot: the loss's, or None."""
        x, edge_attr, edge_index, y, n, e = self._batch(x, edge_attr, edge_index, y)
        L = lib()
        if self.model.auto_status:
            self.model._reap_watched(block=False)
        need = L.gm_train_step_workspace_bytes(C.byref(self.desc), n, e)
        if self._ws is None or self._ws.numel() < need:
            self._ws = _ws(need, self.device)
        head = (self._h, ptr(x), n, ptr(edge_attr), ptr(edge_index), e, ptr(y), self.mask_col)
        tail = (ptr(slot), ptr(self._ws), self._ws.numel(), current_stream(x))
        check(L.gm_train_step(*head, self.lr, *tail) if update else L.gm_train_step_accumulate(*head, *tail))
        self.model._watch(self._ws)   # the workspace begins with the tape's CSR header: the edge_index verdict

    # ------------------------------------------------------------------------------------------ a mini-batch
    @property
    def last_grad_norm(self):
        """The norm of the mean gradient of the last ``apply`` that computed one and was given no ``norm_out``: a float64 device
        tensor of one element."""
        return self._grad_norm

    def _clipping(self):
        g = self.max_grad_norm
        if g is not None and float(g) != float(g):
            raise ValueError("max_grad_norm is NaN")
        return g is not None and 0.0 < float(g) < float("inf")

    def zero_grad(self):
        """Starts a mini-batch: gm_trainer_begin clears the gradients and the mini-batch's record."""
        check(lib().gm_trainer_begin(self._h, current_stream(self.device)))
        self._dp_error = None

    def _accumulated(self, call):
        if self._dp_error is not None:
            return                    # a distributed trainer whose mini-batch has failed already: it will be skipped as a whole
        try:
            call()
        except GMError as error:
            self.zero_grad()          # the failed sample may be partly in the gradients: the pending mini-batch is dropped
            if self._dp is None:
                raise
            self._dp_error = error    # the peers wait in apply's exchange: the error is raised there, after it

    def _not_distributed(self, what):
        if self._dp is not None:
            raise ValueError(f"Trainer.{what} updates this replica alone: on a distributed trainer use zero_grad / accumulate / "
                             "apply(samples_total=), or the epoch methods")

    def accumulate(self, x, edge_attr=None, edge_index=None, y=None, loss_out=None):
        """Adds a batch's gradient to the pending mini-batch (``step``'s arguments and checks): gm_train_step_accumulate.  The
        batch's own loss goes into ``loss_out`` when one is given.  A ``GMError`` drops the pending mini-batch."""
        slot = None if loss_out is None else self._slot(loss_out)
        self._accumulated(lambda: self._one_batch(x, edge_attr, edge_index, y, slot, False))

    def accumulate_rollout(self, engine, obs0, frames, steps=None, pos_scale=None, loss_out=None, state_material_col=None):
        """Adds a rollout sample's gradient to the pending mini-batch (``step_rollout``'s arguments and checks):
        gm_train_rollout_accumulate.  Samples of different scenes and sizes may share a mini-batch."""
        self._accumulated(lambda: self._rollout(engine, obs0, frames, steps, pos_scale, loss_out, state_material_col, "accumulate"))

    def accumulate_rollout_batch(self, engine, obs0, frames_list, steps=None, pos_scale=None, losses_out=None, state_material_col=None):
        """Adds a whole mini-batch of rollout windows of different sizes to the pending mini-batch as ONE ragged rollout, one loss,
        one reverse sweep and one update of the mini-batch's record: gm_train_rollout_accumulate_ragged.  ``engine`` is a ragged
        ``RolloutEngine(sizes=...)`` after ``set_scene(obs0)``; ``obs0`` [k, N, D] holds the windows side by side along the node
        axis; ``frames_list`` holds one [>= steps, n_g, D or D - 3] tensor per scene (views into resident recordings).  Every
        scene counts as one sample with its own loss (``accumulate_rollout``'s, with that scene's row count): ``apply`` divides by
        the number of scenes.  ``losses_out``: a float64 device tensor of one element per scene, or None.  The sweep reads one edge
        count per step back for the WHOLE batch.  Not on a distributed trainer."""
        self._not_distributed("accumulate_rollout_batch")
        self._accumulated(lambda: self._rollout_batch(engine, obs0, frames_list, steps, pos_scale, losses_out, state_material_col, 1))

    def evaluate_rollout_batch(self, engine, obs0, frames_list, steps=None, pos_scale=None, losses_out=None, state_material_col=None):
        """``accumulate_rollout_batch``'s rollout and per-scene losses without gradients or the record: changes nothing, needs no
        pending mini-batch and never synchronises."""
        self._not_distributed("evaluate_rollout_batch")
        self._rollout_batch(engine, obs0, frames_list, steps, pos_scale, losses_out, state_material_col, 0)

    def _rollout_batch(self, engine, obs0, frames_list, steps, pos_scale, losses_out, state_material_col, update):
        """gm_train_rollout_accumulate_ragged (update: accumulate, else evaluate) on checked arguments."""
        if not getattr(engine, "ragged", False):
            raise ValueError("a rollout batch needs a ragged engine: RolloutEngine(model, graph_attr, sizes=[...])")
        self._check_rollout_scene(engine, obs0)
        frames_list = list(frames_list)
        G = len(engine.sizes)
        if len(frames_list) != G:
            raise ValueError(f"frames_list must hold one tensor per scene ({G}), got {len(frames_list)}")
        frame_dim = int(frames_list[0].shape[-1]) if isinstance(frames_list[0], torch.Tensor) and frames_list[0].dim() == 3 else -1
        self._check_frame_width(engine, frame_dim)
        for g, f in enumerate(frames_list):
            engine._check_tensor(f, f"frames_list[{g}]", ("steps", engine.sizes[g], frame_dim))
        steps, col, scale = self._rollout_args(engine, min(int(f.shape[0]) for f in frames_list), steps, pos_scale, state_material_col, G)
        if losses_out is None:
            losses_out = self._batch_losses[:G]
        elif losses_out.dtype != torch.float64 or losses_out.numel() != G or losses_out.device != self.device or not losses_out.is_contiguous():
            raise ValueError(f"losses_out must be {G} contiguous float64 elements on the trainer's device")
        views = (C.c_void_p * G)(*[f.data_ptr() for f in frames_list])     # read during the call: the tensors outlive it in frames_list
        check(lib().gm_train_rollout_accumulate_ragged(self._h, ptr(obs0), engine._offsets_host, G, C.byref(engine.fdesc), engine.max_neighbours,
                                                       ptr(engine.rigid_rank), engine.n_rigid, views, frame_dim, steps, col, scale, int(update),
                                                       ptr(losses_out), ptr(self._rollout_ws), self._rollout_ws.numel(), current_stream(obs0)))

    def apply(self, loss_out=None, norm_out=None, want_norm=False, samples_total=None):
        """One Adam update from the MEAN of the accumulated gradients, clipped to ``max_grad_norm`` (None, <= 0 or inf: no clip)
        by ``clip_grad_norm_``'s formula: gm_trainer_apply.  The mean of the samples' losses goes into ``last_loss`` or
        ``loss_out``.  The gradient norm is computed when the clip is in force, ``want_norm`` is set or ``norm_out`` (one float64
        element on the device) is given, and goes into ``norm_out`` or ``last_grad_norm``.  A mini-batch with a skipped sample, or
        whose gradient norm is not finite, changes nothing: ``record()`` counts it, its loss is NaN.

        On a distributed trainer every rank calls it, with ``samples_total`` the samples of the mini-batch over ALL ranks (a rank
        may hold none): the ranks' gradients and records are merged first (``contribution``, one all-gather, ``reduce``), and the
        update, its loss and its norm are the global ones, the same bits on every rank.  A sample that raised ``GMError`` on this
        rank skips the update on every rank; the error is raised here, after the exchange."""
        slot = self._slot(loss_out)
        norm = None
        if self._clipping() or want_norm or norm_out is not None:
            norm = self._grad_norm if norm_out is None else self._slot(norm_out)
        mg = 0.0 if self.max_grad_norm is None else float(self.max_grad_norm)
        error = None
        if self._dp is not None:
            if samples_total is None or int(samples_total) < 1:
                raise ValueError("apply on a distributed trainer needs samples_total, the mini-batch's samples over all ranks")
            error, self._dp_error = self._dp_error, None
            local = self.contribution(out=self._dp.local, poisoned=error is not None)
            exchange_bytes(local, self._dp.gathered, self._dp.group, self._dp.staging)
            self.reduce(self._dp.gathered, samples_total)
        elif samples_total is not None:
            raise ValueError("samples_total belongs to a distributed trainer (distribute())")
        check(lib().gm_trainer_apply(self._h, self.lr, mg, ptr(slot), ptr(norm), current_stream(self.device)))
        if error is not None:
            raise error

    # ------------------------------------------------------------------------------------------ several replicas
    def contribution_bytes(self):
        """The bytes of one rank's contribution: the flat gradient buffer and the 32-byte tail (gm_trainer_contribution_bytes)."""
        return int(lib().gm_trainer_contribution_bytes(self._h))

    def contribution(self, out=None, poisoned=False):
        """What this rank brings to a shared mini-batch, as a ``uint8`` device tensor (``out``, or a new one): the accumulated
        gradients and {samples, bad, loss_sum, steps_applied} (gm_trainer_contribution).  ``poisoned``: zeros and one bad sample,
        which skips the update on every rank."""
        need = self.contribution_bytes()
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=self.device)
        if out.dtype != torch.uint8 or out.device != self.device or out.dim() != 1 or out.numel() < need or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of at least {need} bytes on the trainer's device")
        check(lib().gm_trainer_contribution(self._h, ptr(out), out.numel(), int(bool(poisoned)), current_stream(self.device)))
        return out

    def reduce(self, gathered, samples_total):
        """Merges the ranks' contributions, ``gathered`` [world, bytes] ``uint8`` in rank order, into this trainer's pending
        mini-batch: the gradients summed in float32 in rank order, the records merged (gm_trainer_reduce).  ``samples_total`` is
        the global sample count; ``apply()`` then updates from the merged mini-batch."""
        if gathered.dtype != torch.uint8 or gathered.device != self.device or gathered.dim() != 2 or not gathered.is_contiguous():
            raise ValueError("gathered must be a contiguous [world, bytes] uint8 tensor on the trainer's device")
        check(lib().gm_trainer_reduce(self._h, ptr(gathered), int(gathered.shape[0]), int(gathered.shape[1]), int(samples_total),
                                      current_stream(self.device)))

    def distribute(self, group=None, collective_device=None, src=0):
        """Makes this trainer one replica of ``torch.distributed``'s ``group`` (None: the default group).  Rank ``src``'s weights,
        both moments and step count are broadcast to the group, the exchange buffers are allocated once, and ``apply`` from now on
        merges the ranks' mini-batches before it updates.  ``collective_device=None``: the payload stays on the device
        (``all_gather_into_tensor`` on RCCL, stream-ordered; the trainer adds no host synchronisation, an epoch keeps its single
        one).  ``collective_device="cpu"``: staged through pinned host memory for gloo, which synchronises at every update -- the
        planner's rehearsal pattern, for several ranks on one GPU."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            raise RuntimeError("Trainer.distribute: torch.distributed is not initialised")
        host = collective_device is not None and torch.device(collective_device).type == "cpu"
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        steps = torch.tensor([self.record()["steps_applied"]], dtype=torch.int64, device="cpu" if host else self.device)
        dist.broadcast(steps, src=src, group=group)
        state = {}
        for what in (PARAMS, EXP_AVG, EXP_AVG_SQ):
            flat = torch.cat([t.reshape(-1) for t in self.export(what)])
            payload = flat.cpu() if host else flat
            dist.broadcast(payload, src=src, group=group)
            state[what] = [t.view(s) for t, s in zip(payload.to(self.device).split([int(np.prod(s)) for s in self._shapes]), self._shapes)]
        if dist.get_rank() != src:
            self._import(EXP_AVG, state[EXP_AVG], int(steps[0]))
            self._import(EXP_AVG_SQ, state[EXP_AVG_SQ])
            self._import(PARAMS, state[PARAMS])
        self._dp = _Replicas(group, world, rank, self.contribution_bytes(), self.device, host)
        self._dp_error = None
        return self

    def replicas_in_step(self):
        """True when every replica of the group holds the same weights and step count: a float64 gm_grad_sumsq of the exported
        weights and ``steps_applied``, compared bit for bit across the ranks.  Synchronises; for use between epochs."""
        if self._dp is None:
            raise ValueError("replicas_in_step: the trainer is not distributed")
        L = lib()
        flat = torch.cat([t.reshape(-1) for t in self.export(PARAMS)])
        mine = torch.empty(2, dtype=torch.float64, device=self.device)
        mine[1] = float(self.record()["steps_applied"])
        ws = _ws(L.gm_grad_sumsq_workspace_bytes(flat.numel()), self.device)
        check(L.gm_grad_sumsq(ptr(flat), flat.numel(), ptr(mine), ptr(ws), ws.numel(), current_stream(self.device)))
        local = mine.view(torch.uint8)
        everyone = torch.empty((self._dp.world, local.numel()), dtype=torch.uint8, device=self.device)
        staging = None
        if self._dp.host:
            staging = (torch.empty_like(local, device="cpu").pin_memory(), torch.empty_like(everyone, device="cpu").pin_memory())
        exchange_bytes(local, everyone, self._dp.group, staging)
        return bool((everyone.cpu() == everyone[0].cpu()).all())

    def accum_record(self):
        """{'samples', 'bad', 'loss_sum', 'sumsq', 'grad_norm', 'scale'} of the mini-batch's device record (synchronises)."""
        check(lib().gm_trainer_accum_record(self._h, C.c_void_p(self._pin_accum.data_ptr()), current_stream(self.device)))
        torch.cuda.current_stream(self.device).synchronize()
        f = self._pin_accum[2:].view(torch.float64)
        return {"samples": int(self._pin_accum[0]), "bad": int(self._pin_accum[1]), "loss_sum": float(f[0]), "sumsq": float(f[1]),
                "grad_norm": float(f[2]), "scale": float(f[3])}

    def evaluate(self, x, edge_attr=None, edge_index=None, y=None, loss_out=None):
        """train_dyn.py's ``test_epoch`` on one batch: the inference forward of the trainer's weights and the same loss, no update."""
        x, edge_attr, edge_index, y, n, e = self._batch(x, edge_attr, edge_index, y)
        slot = self._slot(loss_out)
        L = lib()
        if self.model.auto_status:
            self.model._reap_watched(block=False)
        csr = DstCsr(edge_index, n, flow=self.model.convention[0])
        fwd = _ws(L.gm_forward_workspace_bytes(C.byref(self.desc), n, e), self.device)
        out = torch.empty((n, self.model.dims[2]), dtype=torch.float32, device=self.device)
        check(L.gm_epd_forward(self._h.model, ptr(x), n, ptr(edge_attr), 0, ptr(csr.ws), e, ptr(out), ptr(fwd), fwd.numel(), current_stream(x)))
        check(L.gm_l1_loss(ptr(out), ptr(y), n, self.model.dims[2], ptr(x), self.model.dims[0], self.mask_col, ptr(slot), None, None,
                           ptr(self._loss_ws), self._loss_ws.numel(), current_stream(x)))
        self.model._last_csr = csr
        if self.model.auto_status:
            self.model._watch(csr)

    # ------------------------------------------------------------------------------------------ an epoch
    def _epoch(self, loader, one):
        losses = torch.full((max(len(loader), 1),), float("nan"), dtype=torch.float64, device=self.device)
        count = 0
        for batch in loader:
            if count == losses.numel():
                losses = torch.cat((losses, torch.full_like(losses, float("nan"))))
            one(batch, loss_out=losses[count:count + 1])
            count += 1
        if self._pin_losses is None or self._pin_losses.numel() < losses.numel():
            self._pin_losses = torch.empty(losses.numel(), dtype=torch.float64).pin_memory()
        host = self._pin_losses[:losses.numel()]
        host.copy_(losses, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()   # the epoch's one synchronisation
        return host[:count].numpy().copy()

    def _epoch_of_mini_batches(self, items, size, accumulate_one):
        """Consecutive `size` items of `items` form a mini-batch (the last may be shorter): zero_grad, accumulate_one(item) each,
        apply.  One float64 loss per UPDATE, the gradient norms in ``last_epoch_grad_norms``, one synchronisation at the end."""
        size = int(size)
        if size < 1:
            raise ValueError(f"a mini-batch holds at least one sample, got {size}")
        slots = torch.full((2, max(-(-len(items) // size), 1)), float("nan"), dtype=torch.float64, device=self.device)   # losses, norms
        with_norm = self._clipping()
        updates = pending = 0

        def update():
            nonlocal slots, updates
            if updates == slots.shape[1]:
                slots = torch.cat((slots, torch.full_like(slots, float("nan"))), dim=1)
            self.apply(loss_out=slots[0, updates:updates + 1], norm_out=slots[1, updates:updates + 1] if with_norm else None)
            updates += 1
        for item in items:
            if pending == 0:
                self.zero_grad()
            try:
                accumulate_one(item)
            except GMError:
                pending = 0
                raise
            pending += 1
            if pending == size:
                update()
                pending = 0
        if pending:
            update()
        return self._updates_of_epoch(slots, updates)

    def _epoch_of_shared_mini_batches(self, items, size, accumulate_one, total=None):
        """``_epoch_of_mini_batches`` on a distributed trainer: `size` is the GLOBAL mini-batch.  Of every group of `size`
        consecutive items this rank accumulates the contiguous block ``planner.shard_range(len(group), world, rank)`` and calls
        ``apply`` even when that block is empty.  `items` is the global sequence, of which the other ranks' items are passed over
        unused -- or, with `total` (the global item count), an iterable of this rank's items alone, in order.  The losses and norms
        are the global ones, identical on all ranks.  An item that raises ``GMError`` poisons its mini-batch on every rank; the
        error is raised after that mini-batch's exchange, and the epoch ends there ON THIS RANK."""
        from .planner import shard_range
        size = int(size)
        if size < 1:
            raise ValueError(f"a mini-batch holds at least one sample, got {size}")
        own_only = total is not None
        total = int(total) if own_only else len(items)
        slots = torch.full((2, max(-(-total // size), 1)), float("nan"), dtype=torch.float64, device=self.device)   # losses, norms
        with_norm = self._clipping()
        it = iter(items)
        updates = 0
        for first in range(0, total, size):
            count = min(size, total - first)
            lo, hi = shard_range(count, self._dp.world, self._dp.rank)
            self.zero_grad()
            for j in range(count):
                if lo <= j < hi:
                    accumulate_one(next(it))
                elif not own_only:
                    next(it)
            self.apply(loss_out=slots[0, updates:updates + 1], norm_out=slots[1, updates:updates + 1] if with_norm else None,
                       samples_total=count)
            updates += 1
        return self._updates_of_epoch(slots, updates)

    def _updates_of_epoch(self, slots, updates):
        """The losses of an epoch's updates on the host, their norms in ``last_epoch_grad_norms``: the epoch's one synchronisation."""
        if self._pin_losses is None or self._pin_losses.numel() < slots.numel():
            self._pin_losses = torch.empty(slots.numel(), dtype=torch.float64).pin_memory()
        host = self._pin_losses[:slots.numel()].view(slots.shape)
        host.copy_(slots, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()   # the epoch's one synchronisation
        self.last_epoch_grad_norms = host[1, :updates].numpy().copy()
        return host[0, :updates].numpy().copy()

    def fit_epoch(self, loader, accumulate=1):
        """``step`` over every batch of `loader` (a ``GraphLoader``, fused and prefetching or not): the per-batch losses as a
        float64 numpy array, after a single synchronisation at the end.  A skipped batch's loss is NaN.

        ``accumulate`` > 1: every ``accumulate`` consecutive batches (the last group may be shorter) form a mini-batch with ONE
        update from the mean of their gradients (``zero_grad`` / ``accumulate`` / ``apply``); the array then holds one loss per
        update, the mean over its batches.  ``last_epoch_grad_norms`` holds the updates' gradient norms, NaN where none was
        computed (no clip in force).

        On a distributed trainer ``accumulate`` is the GLOBAL mini-batch, shared out over the ranks block by block; `loader` is a
        ``GraphLoader(..., shard=(rank, world, accumulate))``, which builds this rank's batches only, or any sequence of all the
        batches.  The losses and norms are the global ones, the same on every rank."""
        if self._dp is not None:
            shard = getattr(loader, "shard", None)
            if shard is None:
                return self._epoch_of_shared_mini_batches(loader, accumulate, self.accumulate)
            if tuple(int(v) for v in shard) != (self._dp.rank, self._dp.world, int(accumulate)):
                raise ValueError(f"fit_epoch: the loader's shard {tuple(shard)} is not (rank, world, accumulate) = "
                                 f"{(self._dp.rank, self._dp.world, int(accumulate))}")
            return self._epoch_of_shared_mini_batches(loader, accumulate, self.accumulate, total=loader.batches_in_all)
        if int(accumulate) == 1 and self.max_grad_norm is None:
            losses = self._epoch(loader, self.step)
            self.last_epoch_grad_norms = np.full(len(losses), np.nan)
            return losses
        return self._epoch_of_mini_batches(loader, accumulate, self.accumulate)

    def eval_epoch(self, loader):
        """``evaluate`` over every batch of `loader`, as ``fit_epoch``."""
        return self._epoch(loader, self.evaluate)

    # ------------------------------------------------------------------------------------------ a rollout
    # What a rollout call and a rollout batch share around their own check of the frames: the scene before it, the frames' width
    # where each of them knows it, and everything from the step count to the workspace after it.
    @staticmethod
    def _check_rollout_scene(engine, obs0):
        if engine.rigid_rank is None:
            raise ValueError("engine.set_scene(obs0) must be called before a rollout step")
        engine._check_tensor(obs0, "obs0", (engine.k, engine.n, engine.data_dim))

    @staticmethod
    def _check_frame_width(engine, frame_dim):
        if frame_dim not in (engine.data_dim, engine.data_dim - 3):
            raise ValueError(f"frames must have {engine.data_dim} or {engine.data_dim - 3} columns, got {frame_dim}")

    def _rollout_args(self, engine, most, steps, pos_scale, state_material_col, graphs=None):
        """`most`: the frames given; `graphs`: the scenes of a ragged batch.  Grows the rollout workspace, notes the shape
        ``kept_windows`` views, and returns (steps, the state's material column or -1, pos_scale as c_double[3] or None)."""
        steps = most if steps is None else int(steps)
        if not 1 <= steps <= most:
            raise ValueError(f"steps={steps} outside 1..{most}, the frames given")
        if engine.device != self.device:
            raise ValueError(f"the engine is on {engine.device}, the trainer on {self.device}")
        scale = None
        if pos_scale is not None:
            scale = [float(v) for v in np.asarray(pos_scale, np.float64).reshape(-1)]
            if len(scale) != 3 or not all(v == v and v != 0.0 for v in scale):
                raise ValueError("pos_scale must be three non-zero numbers")
            scale = (C.c_double * 3)(*scale)
        col = -1
        if self.sand_only:
            col = engine.fdesc.material_col if state_material_col is None else int(state_material_col)
            if col < 0:
                col += engine.data_dim
            if not 0 <= col < engine.data_dim:
                raise ValueError(f"state_material_col={state_material_col} is outside the {engine.data_dim} state columns")
        L = lib()
        sizes = (C.byref(self.desc), C.byref(engine.fdesc), engine.n, engine.n_rigid)
        if graphs is None:
            need = L.gm_train_rollout_step_workspace_bytes(*sizes, engine.max_neighbours, steps)
        else:
            need = L.gm_train_rollout_ragged_workspace_bytes(*sizes, graphs, engine.max_neighbours, steps)
        if need == 0:
            raise ValueError("Trainer: no rollout workspace for these sizes")
        if self._rollout_ws is None or self._rollout_ws.numel() < need:
            self._rollout_ws = _ws(need, self.device)
        self._kept = (steps + 1, engine.k, engine.n, engine.data_dim)
        return steps, col, scale

    def _rollout(self, engine, obs0, frames, steps, pos_scale, loss_out, state_material_col, mode):
        """gm_train_rollout_step (mode "step" / "evaluate") or gm_train_rollout_accumulate ("accumulate") on checked arguments."""
        self._check_rollout_scene(engine, obs0)
        engine._check_tensor(frames, "frames", ("steps", engine.n, "frame_dim"))
        frame_dim = int(frames.shape[2])
        self._check_frame_width(engine, frame_dim)
        steps, col, scale = self._rollout_args(engine, int(frames.shape[0]), steps, pos_scale, state_material_col)
        slot = None if mode == "accumulate" and loss_out is None else self._slot(loss_out)
        L = lib()
        head = (self._h, ptr(obs0), engine.n, C.byref(engine.fdesc), engine.max_neighbours, ptr(engine.rigid_rank), engine.n_rigid,
                ptr(frames), frame_dim, steps, col, scale)
        tail = (ptr(slot), ptr(self._rollout_ws), self._rollout_ws.numel(), current_stream(obs0))
        if mode == "accumulate":
            check(L.gm_train_rollout_accumulate(*head, *tail))
        else:
            check(L.gm_train_rollout_step(*head, self.lr, int(mode == "step"), *tail))

    def step_rollout(self, engine, obs0, frames, steps=None, pos_scale=None, loss_out=None, state_material_col=None):
        """One training step on a ``steps``-step rollout: gm_train_rollout_step.  ``engine`` is a
        ``RolloutEngine`` after ``set_scene``: it supplies the feature descriptor, the rigid rows and the neighbour cap; the model
        that runs is the TRAINER's.  ``obs0`` [k, N, D] is the window the rollout starts from (not written); ``frames``
        [>= steps, N, D or D - 3] the recorded frame that follows each step, which may be a view into a resident recording.  The
        rigid rows follow the recording, the loss is the L1 distance of every other row's predicted position to the recorded one,
        each axis divided by ``pos_scale`` (three numbers; None: ones), over ``steps`` x the rows counted.  ``sand_only`` counts
        the rows whose STATE material column (the engine's, or ``state_material_col``) is below 0.5 in ``obs0``'s last frame.
        Nothing is returned; the loss goes into ``last_loss`` or ``loss_out``.  The reverse sweep reads one edge count per step
        back, so the call synchronises ``steps`` times; a non-finite loss skips the update on the device like ``step``."""
        self._not_distributed("step_rollout")
        if self.max_grad_norm is not None:
            self.zero_grad()
            self.accumulate_rollout(engine, obs0, frames, steps, pos_scale=pos_scale, state_material_col=state_material_col)
            return self.apply(loss_out=loss_out)
        self._rollout(engine, obs0, frames, steps, pos_scale, loss_out, state_material_col, "step")

    def evaluate_rollout(self, engine, obs0, frames, steps=None, pos_scale=None, loss_out=None, state_material_col=None):
        """``step_rollout``'s rollout and loss without the update: a validation pass that changes nothing and never synchronises."""
        self._rollout(engine, obs0, frames, steps, pos_scale, loss_out, state_material_col, "evaluate")

    def kept_windows(self):
        """[steps + 1, k, N, D]: the windows the last ``step_rollout`` / ``evaluate_rollout`` passed through, a view of its
        workspace -- window t < steps the state before step t, the last one the final state -- valid until the next such call."""
        count = int(np.prod(self._kept))
        return self._rollout_ws[:4 * count].view(torch.float32).view(self._kept)

    def fit_rollout_epoch(self, dataset, engine, steps, starts=None, seed=0, pos_scale=None, batch_size=1, shuffle=False, batched=False):
        """``step_rollout`` over the samples ``starts`` of ``dataset`` (default: every non-overlapping start, ``steps`` apart, of
        every recording that has ``steps`` frames behind the window), each built by ``dataset.rollout_sample(start, steps, seed,
        stream=start)``.  ``engine.set_scene`` is called whenever the recording changes.  The per-sample losses come back as a
        float64 numpy array after the last step; a skipped sample's loss is NaN.

        ``batch_size`` > 1: every ``batch_size`` consecutive samples (the last group may be shorter) form a mini-batch with ONE
        update from the mean of their gradients -- samples of different recordings and sizes may share one: for recordings of
        different node counts ``engine`` is a dict {node count: RolloutEngine}; the array then holds one loss per update, the mean over its samples.  ``shuffle``: the starts in a
        permutation seeded by ``seed``.  ``last_epoch_grad_norms`` holds the updates' gradient norms, NaN where none was computed.

        ``batched=True`` with ``batch_size`` > 1: a mini-batch is ONE ragged rollout instead of ``batch_size`` rollouts one after
        the other -- ``zero_grad``, one ``torch.cat`` of its windows along the node axis, a ragged ``RolloutEngine(sizes=...)`` per
        distinct tuple of sizes (made at first use and kept for the epoch; ``engine`` may be None: ``graph_attr``, ``k``, the
        state's width and the neighbour cap come from the dataset, or from the engine(s) given), ``set_scene``,
        ``accumulate_rollout_batch``, ``apply``.  The losses are those of the unbatched epoch on the same weights; the gradients
        differ in the order the samples' contributions are added.  Opt-in: INTEGRATION.md 2e has the measurement.

        On a distributed trainer every rank passes the same ``starts`` and ``seed``; ``batch_size`` is the GLOBAL mini-batch, of
        which this rank runs its contiguous block; the losses and norms are the global ones, the same on every rank.
        ``batched=True`` raises ValueError there."""
        steps = int(steps)
        if batched and self._dp is not None:
            raise ValueError("fit_rollout_epoch(batched=True) is not available on a distributed trainer")
        if starts is None:
            starts, first = [], 0
            for sim in dataset.sims:
                last = int(sim.shape[0]) - dataset.k - steps       # the last start whose frames are all recorded
                starts += [first + t for t in range(0, last + 1, steps)]
                first += int(sim.shape[0]) - dataset.k
        starts = [int(i) for i in starts]
        if shuffle:
            starts = [starts[i] for i in np.random.default_rng(seed).permutation(len(starts))]
        scene = [None]

        def sample(start):
            window, frames = dataset.rollout_sample(start, steps, seed=seed, stream=start)
            eng = engine
            if isinstance(engine, dict):
                if int(window.shape[1]) not in engine:
                    raise ValueError(f"fit_rollout_epoch: no engine for a recording of {int(window.shape[1])} nodes")
                eng = engine[int(window.shape[1])]
            if scene[0] != dataset.index[start][0]:
                eng.set_scene(window)
                scene[0] = dataset.index[start][0]
            return eng, window, frames

        def one(start, loss_out):
            eng, window, frames = sample(start)
            self.step_rollout(eng, window, frames, steps, pos_scale=pos_scale, loss_out=loss_out)

        def accumulate_one(start):
            eng, window, frames = sample(start)
            self.accumulate_rollout(eng, window, frames, steps, pos_scale=pos_scale)
        if batched and int(batch_size) > 1:
            return self._rollout_epoch_batched(dataset, engine, steps, starts, seed, pos_scale, int(batch_size))
        if self._dp is not None:
            return self._epoch_of_shared_mini_batches(starts, batch_size, accumulate_one)
        if int(batch_size) == 1 and self.max_grad_norm is None:
            losses = self._epoch(starts, one)
            self.last_epoch_grad_norms = np.full(len(losses), np.nan)
            return losses
        return self._epoch_of_mini_batches(starts, batch_size, accumulate_one)

    def _rollout_epoch_batched(self, dataset, engine, steps, starts, seed, pos_scale, size):
        """fit_rollout_epoch(batched=True): every `size` consecutive starts are one ragged rollout."""
        from .rollout import RolloutEngine
        given = next(iter(engine.values())) if isinstance(engine, dict) and engine else (None if isinstance(engine, dict) else engine)
        engines = {}
        slots = torch.full((2, max(-(-len(starts) // size), 1)), float("nan"), dtype=torch.float64, device=self.device)   # losses, norms
        with_norm = self._clipping()
        updates = 0
        for first in range(0, len(starts), size):
            samples = [dataset.rollout_sample(start, steps, seed=seed, stream=start) for start in starts[first:first + size]]
            sizes = tuple(int(w.shape[1]) for w, _ in samples)
            if sizes not in engines:
                window = samples[0][0]
                engines[sizes] = RolloutEngine(
                    self.model, dataset.graph_attr if given is None else given.graph_attr, k_steps=int(window.shape[0]),
                    data_dim=int(window.shape[2]), max_neighbours=getattr(dataset, "max_neighbours", 20) if given is None else given.max_neighbours,
                    device=self.device, sizes=sizes)
            eng = engines[sizes]
            self.zero_grad()
            obs0 = torch.cat([w for w, _ in samples], dim=1).contiguous()
            eng.set_scene(obs0)
            self.accumulate_rollout_batch(eng, obs0, [f for _, f in samples], steps, pos_scale=pos_scale)
            self.apply(loss_out=slots[0, updates:updates + 1], norm_out=slots[1, updates:updates + 1] if with_norm else None)
            updates += 1
        return self._updates_of_epoch(slots, updates)

    # ------------------------------------------------------------------------------------------ state
    def record(self):
        """{'steps_applied', 'steps_skipped', 'beta1_pow', 'beta2_pow'} of the device record (synchronises)."""
        check(lib().gm_trainer_record(self._h, C.c_void_p(self._pin_record.data_ptr()), current_stream(self.device)))
        torch.cuda.current_stream(self.device).synchronize()
        powers = self._pin_record[2:].view(torch.float64)
        return {"steps_applied": int(self._pin_record[0]), "steps_skipped": int(self._pin_record[1]),
                "beta1_pow": float(powers[0]), "beta2_pow": float(powers[1])}

    def status(self):
        """Raises ``GMError`` if a step or evaluation so far had an edge_index entry outside [0, N) (synchronises)."""
        return self.model.status()

    def export(self, what=PARAMS):
        """Copies of one of the trainer's buffers (PARAMS, EXP_AVG, EXP_AVG_SQ, GRADS), shaped like the module's parameters."""
        tensors = [torch.empty(s, dtype=torch.float32, device=self.device) for s in self._shapes]
        check(lib().gm_trainer_export(self._h, int(what), _pointers(tensors), len(tensors), current_stream(self.device)))
        return tensors

    def _import(self, what, tensors, step_count=0):
        tensors, arr = _device_arrays(tensors, self.device)
        check(lib().gm_trainer_import(self._h, int(what), arr, len(tensors), int(step_count), current_stream(self.device)))

    def sync_module(self):
        """Copies the trained weights into the module's ``nn.Parameter`` s and has the module re-pack its own images."""
        with torch.no_grad():
            for p, w in zip(self.model.parameters(), self.export(PARAMS)):
                p.data.copy_(w)
        self.model.invalidate_packed_weights()

    def load_module(self):
        """The other direction: the module's current parameters become the trainer's weights (moments and step count stay)."""
        self._import(PARAMS, list(self.model.parameters()))

    def state_dict(self):
        """``torch.optim.Adam``'s layout (``state[i] = {step, exp_avg, exp_avg_sq}``, ``param_groups``): with ``sync_module()`` and
        the module's own state_dict, the checkpoint of train_dyn.py:33-43."""
        return adam_state_dict(self.export(EXP_AVG), self.export(EXP_AVG_SQ), self.record()["steps_applied"], self.lr, self.betas, self.eps)

    def load_state_dict(self, sd):
        """Resumes from an Adam state_dict (the trainer's, or ``torch.optim.Adam``'s over the same parameters).  The betas and eps
        must be the trainer's; the learning rate is taken over."""
        m, v, step, group = parse_adam_state_dict(sd, self._shapes)
        if tuple(float(b) for b in group["betas"]) != self.betas or float(group["eps"]) != self.eps:
            raise ValueError(f"Trainer.load_state_dict: betas / eps {group['betas']} / {group['eps']} are not the trainer's "
                             f"{self.betas} / {self.eps}")
        zeros = lambda: [torch.zeros(s, dtype=torch.float32, device=self.device) for s in self._shapes]
        self._import(EXP_AVG, zeros() if m is None else m, step)
        self._import(EXP_AVG_SQ, zeros() if v is None else v)
        self.lr = float(group["lr"])
