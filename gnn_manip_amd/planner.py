"""Planner-side pieces of the hot path: the scripted cup pose (``compute_particles_tmatrix``,
``interpolate_trajectory``, ``get_rigid_body_trajectory_from_diff``; gnn_manip/utils/traj_utils.py:87-103,
167-228) and candidate-parallel evaluation of CMA-ES populations across the GPUs of a node
(SURVEY.md section 8e): candidates are independent rollouts (traj_utils.py:114-159), so each rank
evaluates a contiguous block; one broadcast of the candidate matrix and one all-gather of the
per-candidate results per generation (RCCL over xGMI when the backend is ``nccl``).
"""
import ctypes as C

import numpy as np
import torch

from ._lib import check, current_stream, lib, ptr


def interpolate_trajectory(x, n_points, rx_init, scale_rot, scale_ty, max_rot, max_ty):
    """TrajectoryCMAsolver.interpolate_trajectory (traj_utils.py:206-228); host float64 like the reference.
    rx_init / max_rot in radians."""
    prev_r, prev_t = rx_init, 0.0
    rot, ty = [rx_init], [0.0]
    for i in range(n_points):
        inc_r = np.clip(np.deg2rad(scale_rot * np.rad2deg(x[i])), -max_rot, max_rot)
        inc_t = np.clip(scale_ty * x[i + n_points], -max_ty, max_ty)
        prev_r = prev_r + inc_r
        prev_t = prev_t + inc_t
        rot.append(prev_r)
        ty.append(prev_t)
    return rot, ty


def compute_particles_tmatrix(rotation, translation, ty_init, rigid_particles):
    """traj_utils.py:167-194 for ONE pose; rigid_particles: [Nr, 3] CUDA tensor."""
    return get_rigid_body_trajectory([rotation], [translation], 1, ty_init, rigid_particles)[0]


def get_rigid_body_trajectory(traj_rot, traj_ty, horizon, ty_init, rigid_particles):
    """Body of get_rigid_body_trajectory_from_diff (traj_utils.py:97-99): [horizon, Nr, 3] on the device.
    cos / sin are evaluated on the host in float64 and rounded to float32, as the reference does when it
    builds the 4x4 float32 matrix (traj_utils.py:171-172)."""
    rp = rigid_particles.contiguous().float()
    assert rp.is_cuda
    if len(traj_rot) < horizon or len(traj_ty) < horizon:
        # the reference indexes traj[i] for i < horizon (traj_utils.py:97-99) and raises IndexError on a short trajectory
        raise IndexError(f"trajectory of {min(len(traj_rot), len(traj_ty))} poses is shorter than the horizon {horizon}")
    rot = np.asarray(traj_rot[:horizon], dtype=np.float64)
    ty = np.asarray(traj_ty[:horizon], dtype=np.float64)
    cst = np.stack((np.cos(rot), np.sin(rot), float(ty_init[1]) + ty), axis=1).astype(np.float32)
    cst_d = torch.from_numpy(cst).to(rp.device)
    out = torch.empty((horizon, rp.shape[0], 3), dtype=torch.float32, device=rp.device)
    t3 = (C.c_float * 3)(*[float(v) for v in ty_init])
    check(lib().gm_rigid_transform(ptr(rp), rp.shape[0], ptr(cst_d), horizon, C.byref(t3), ptr(out), current_stream()))
    return out


def interpolate_trajectory_torch(x, n_points, rx_init, scale_rot, scale_ty, max_rot, max_ty):
    """``interpolate_trajectory`` restated in float64 torch, differentiable in ``x`` (a 1-D float64 tensor): the clipped
    increments (``clamp``: zero gradient beyond the limits) and their running sums, in the reference's order of additions.
    Returns (rot, ty), each [n_points + 1]."""
    inc_r = torch.clamp(torch.deg2rad(scale_rot * torch.rad2deg(x[:n_points])), -max_rot, max_rot)
    inc_t = torch.clamp(scale_ty * x[n_points:2 * n_points], -max_ty, max_ty)
    first = lambda v: torch.tensor([v], dtype=x.dtype, device=x.device)
    return torch.cumsum(torch.cat((first(rx_init), inc_r)), 0), torch.cumsum(torch.cat((first(0.0), inc_t)), 0)


class _RigidTransformFunction(torch.autograd.Function):
    """gm_rigid_transform under autograd in its (cos, sin, ty) rows: the backward is gm_rigid_transform_backward."""

    @staticmethod
    def forward(ctx, rp, cst, ty_init):
        steps = int(cst.shape[0])
        out = torch.empty((steps, rp.shape[0], 3), dtype=torch.float32, device=rp.device)
        t3 = (C.c_float * 3)(*[float(v) for v in ty_init])
        check(lib().gm_rigid_transform(ptr(rp), rp.shape[0], ptr(cst), steps, C.byref(t3), ptr(out), current_stream(rp.device)))
        ctx.t3 = t3
        ctx.save_for_backward(rp, cst)
        return out

    @staticmethod
    def backward(ctx, d_out):
        rp, cst = ctx.saved_tensors
        d_out = d_out.contiguous().float()
        d_cst = torch.empty_like(cst)
        check(lib().gm_rigid_transform_backward(ptr(rp), rp.shape[0], ptr(cst), int(cst.shape[0]), C.byref(ctx.t3), ptr(d_out),
                                                ptr(d_cst), current_stream(rp.device)))
        return None, d_cst, None


def rigid_body_trajectory(rot, ty, horizon, ty_init, rigid_particles):
    """``get_rigid_body_trajectory`` for tensors: rot, ty are float64 tensors (any device) of at least ``horizon`` entries, and
    the [horizon, Nr, 3] poses are differentiable in both.  cos / sin are evaluated in float64 torch and rounded to float32, so
    the poses are bit-equal to ``get_rigid_body_trajectory``'s for the same numbers; the transform is gm_rigid_transform, its
    backward gm_rigid_transform_backward (a fixed-order sum over the rigid particles), the rest of the chain is autograd's."""
    rp = rigid_particles.detach().contiguous().float()
    assert rp.is_cuda
    if rot.dtype != torch.float64 or ty.dtype != torch.float64 or rot.dim() != 1 or ty.dim() != 1:
        raise ValueError("rot and ty must be 1-D float64 tensors")
    if rot.shape[0] < horizon or ty.shape[0] < horizon:
        raise IndexError(f"trajectory of {min(rot.shape[0], ty.shape[0])} poses is shorter than the horizon {horizon}")
    rot, ty = rot[:horizon], ty[:horizon]
    cst = torch.stack((torch.cos(rot), torch.sin(rot), float(ty_init[1]) + ty), dim=1).to(torch.float32).to(rp.device).contiguous()
    return _RigidTransformFunction.apply(rp, cst, ty_init)


def shard_range(n_items, world_size, rank):
    """Contiguous block [lo, hi) of `n_items` candidates owned by `rank` (blocks differ by at most one)."""
    base, rem = divmod(n_items, world_size)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


class CandidateEvaluator:
    """Evaluates a population of candidates in parallel over the ranks of a torch.distributed group.

    evaluate_fn(candidate: np.ndarray) -> 1-D float tensor/array of fixed length `result_dim`
    (e.g. a loss, or final particle statistics).  Rank 0 supplies the population; every rank
    returns the full [popsize, result_dim] result matrix.
    """

    def __init__(self, evaluate_fn, result_dim=1, group=None, device=None):
        self.fn = evaluate_fn
        self.result_dim = int(result_dim)
        self.group = group
        self.device = device
        self.collective_s = 0.0   # wall time spent in the broadcast / all-gather calls so far (host clock around each call)

    def _dist(self):
        import torch.distributed as dist
        return dist if (dist.is_available() and dist.is_initialized()) else None

    def evaluate_blocks(self, population, block_fn):
        """Like evaluate(), but the rank's whole block goes to block_fn(list of candidates) -> list of results at once
        (batched rollouts on the device)."""
        self._block_fn = block_fn
        try:
            return self.evaluate(population)
        finally:
            self._block_fn = None

    _block_fn = None

    def evaluate(self, population):
        dist = self._dist()
        world = dist.get_world_size(self.group) if dist else 1
        rank = dist.get_rank(self.group) if dist else 0
        dev = self.device if self.device is not None else torch.device("cpu")
        import time
        if dist:
            t_c = time.perf_counter()
            shape = torch.zeros(2, dtype=torch.int64, device=dev)
            if rank == 0:
                pop = torch.as_tensor(np.asarray(population, dtype=np.float64), device=dev)
                shape[0], shape[1] = pop.shape
            dist.broadcast(shape, src=0, group=self.group)
            if rank != 0:
                pop = torch.empty((int(shape[0]), int(shape[1])), dtype=torch.float64, device=dev)
            dist.broadcast(pop, src=0, group=self.group)
            pop_np = pop.cpu().numpy()
            self.collective_s += time.perf_counter() - t_c
        else:
            pop_np = np.asarray(population, dtype=np.float64)
        n = pop_np.shape[0]
        per = -(-n // world)  # padded block so that all_gather sees equal shapes
        lo, hi = shard_range(n, world, rank)
        local = torch.zeros((per, self.result_dim), dtype=torch.float64, device=dev)
        if self._block_fn is not None:
            res = self._block_fn([pop_np[c] for c in range(lo, hi)]) if hi > lo else []
            for j, r in enumerate(res):
                local[j] = torch.as_tensor(r, dtype=torch.float64).reshape(-1).to(dev)
        else:
            for j, c in enumerate(range(lo, hi)):
                r = self.fn(pop_np[c])
                local[j] = torch.as_tensor(r, dtype=torch.float64).reshape(-1).to(dev)
        if not dist:
            return local[:n].cpu().numpy()
        t_c = time.perf_counter()   # includes the wait for the slowest rank: load imbalance shows up here
        gathered = [torch.empty_like(local) for _ in range(world)]
        dist.all_gather(gathered, local, group=self.group)
        out = np.zeros((n, self.result_dim))
        for r in range(world):
            a, b = shard_range(n, world, r)
            out[a:b] = gathered[r][:b - a].cpu().numpy()
        self.collective_s += time.perf_counter() - t_c
        return out


def projected_adam(objective, x0, half_widths, iters=20, lr=0.01, betas=(0.9, 0.999), eps=1e-8):
    """Projected Adam on P starts at once, in float64 on the host.  objective(X [P, dim]) -> (values [P], gradients [P, dim]);
    half_widths [dim] > 0: the box is |x_j| <= half_widths[j], and the iteration runs in z = x / half_widths, so that ``lr``
    bounds a step by about that fraction of a half-width per coordinate.  The starts are clamped to the box (iterate 0), every
    update is textbook Adam with bias correction followed by the clamp, and iterate k is evaluated by the k-th call of
    ``objective``: ``iters + 1`` calls, the last one for its values alone.  Starts do not interact (the state is per row).
    Returns (x_best [P, dim], f_best [P], info): per start the iterate of the lowest value, the earliest one among equals;
    info["f"] [P, iters + 1] the values and info["x"] [P, iters + 1, dim] the iterates."""
    hw = np.asarray(half_widths, dtype=np.float64).reshape(-1)
    x0 = np.asarray(x0, dtype=np.float64)
    if x0.ndim != 2 or x0.shape[1] != hw.shape[0] or not (hw > 0).all():
        raise ValueError(f"projected_adam: starts [P, dim] and positive half-widths [dim], got {x0.shape} and {hw.shape}")
    b1, b2 = float(betas[0]), float(betas[1])
    z = np.clip(x0 / hw, -1.0, 1.0)
    m, v = np.zeros_like(z), np.zeros_like(z)
    xs = np.empty((z.shape[0], iters + 1, z.shape[1]))
    fs = np.empty((z.shape[0], iters + 1))
    for k in range(iters + 1):
        xs[:, k] = z * hw
        f, g = objective(xs[:, k].copy())
        fs[:, k] = np.asarray(f, dtype=np.float64).reshape(-1)
        if k == iters:
            break
        g = np.asarray(g, dtype=np.float64).reshape(z.shape) * hw
        m = b1 * m + (1.0 - b1) * g
        v = b2 * v + (1.0 - b2) * g * g
        step = (m / (1.0 - b1 ** (k + 1))) / (np.sqrt(v / (1.0 - b2 ** (k + 1))) + eps)
        z = np.clip(z - lr * step, -1.0, 1.0)
    best = np.argmin(fs, axis=1)   # the first of equal minima
    rows = np.arange(z.shape[0])
    return xs[rows, best].copy(), fs[rows, best].copy(), {"f": fs, "x": xs}


def refine_starts(block_objective, x0, half_widths, iters=20, lr=0.01, betas=(0.9, 0.999), eps=1e-8, collective_device=None):
    """``projected_adam`` with the starts sharded over the ranks of torch.distributed (one process: the plain call).  Rank 0's
    starts are broadcast, each rank refines its contiguous block for all iterations on its own -- block_objective sees that
    block's rows only -- and one all-gather of [f_best, x_best..., f_0...f_iters] rows hands every rank the full result.
    ``info`` then holds "f" alone."""
    import torch.distributed as dist
    kw = dict(iters=iters, lr=lr, betas=betas, eps=eps)
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return projected_adam(block_objective, x0, half_widths, **kw)
    dim = int(np.asarray(half_widths).reshape(-1).shape[0])

    def block(xs):
        xb, fb, info = projected_adam(block_objective, np.stack(xs), half_widths, **kw)
        return list(np.concatenate((fb[:, None], xb, info["f"]), axis=1))

    rows = CandidateEvaluator(None, result_dim=1 + dim + iters + 1, device=collective_device).evaluate_blocks(x0, block)
    return rows[:, 1:1 + dim].copy(), rows[:, 0].copy(), {"f": rows[:, 1 + dim:].copy()}


def density_target(cloud, cell):
    """A particle cloud [M, 3] as a density on a grid of side ``cell``: (centres [M', 3] float32, weights [M'] float32), one entry
    per occupied cell -- the mean of the cell's members and count / M (the weights sum to 1).  A point belongs to the cell
    floor(p / cell) (float64); the cells come in ascending order of that integer key (x, then y, then z), whatever the order of
    the points.  Plain torch, on the cloud's device; what ``SamplesLoss``'s weighted call takes as (y, b)."""
    if cloud.dim() != 2 or cloud.shape[1] != 3 or cloud.shape[0] == 0 or not cell > 0:
        raise ValueError("density_target: cloud must be [M, 3] with M >= 1, cell > 0")
    pts = cloud.detach().double()
    _, inverse, counts = torch.unique(torch.floor(pts / float(cell)).long(), dim=0, return_inverse=True, return_counts=True)
    order = torch.sort(inverse, stable=True).indices
    run = torch.cumsum(pts[order], dim=0)                  # a cell's sum: the running sum at its last member minus at the previous cell's
    ends = torch.cumsum(counts, dim=0) - 1
    sums = run[ends] - torch.cat((torch.zeros_like(run[:1]), run[ends[:-1]]))
    return (sums / counts[:, None]).float(), (counts.double() / cloud.shape[0]).float()


class TrajectoryCMAsolver:
    """Mirror of the reference's ``TrajectoryCMAsolver`` (traj_utils.py:14-76,197-285) with the population of a
    CMA-ES generation evaluated TOGETHER on the device(s) instead of one ``cma_objective`` call per candidate:

    * ``cma_objective(x)``: one candidate, the reference's loop (rollout on the device, no PCIe per step);
    * ``population_losses(X)``: the generation is cut into blocks of ``candidates_per_gpu`` block-diagonal
      batched rollouts (``RolloutEngine(candidates=B)``) and, under ``torch.distributed``, sharded over the ranks
      (``CandidateEvaluator``: one broadcast of X, one all-gather of the losses per generation);
    * ``optimize_trajectory(desired_position)``: ``cmaes.fmin2`` over that (the reference: ``cma.fmin2``, :257);
    * ``loss_and_grad(x)`` / ``population_loss_and_grad(X)`` / ``refine(X0)``: the objective's gradient with respect to the search
      vector, for one candidate and for blocks of them, and the projected Adam that runs on it (not in the reference).

    ``desired_weights`` (None: the reference's behaviour, every point of ``desired_pos`` weighs 1/M): the masses [M] of the points of
    ``desired_pos``, float32 on the device -- the goal as a density (``set_density_target(cloud, cell)`` sets both from a cloud
    binned on a grid; ``optimize_trajectory`` replaces ``desired_pos`` alone).  Every objective above then compares the uniform end
    cloud with the weighted goal (``SamplesLoss``'s four-argument call).

    Same constructor arguments as the reference (``state_init`` = (obs [k, N, D], next positions) on the device).
    The rollouts follow the model's ``set_precision``: ``model.set_precision('f16')`` before planning ranks the candidates with the
    fp16 single-product kernels (what that costs in accuracy and buys in time: DESIGN.md section 6.1).
    """

    def __init__(self, model, graph_attr, state_init, rx_init, ty_init, scale_rot, scale_ty, alpha, beta, gamma, penalty,
                 rho, device, cma_iter=10, cma_var=0.5, cma_popsize=21, cma_rand=1234, max_rot=1.9337, max_ty=6.67e-4,
                 total_steps=300, traj_points=10, candidates_per_gpu=8):
        from . import cmaes
        from .losses import SamplesLoss
        from .rollout import RolloutEngine
        self.initial_state = state_init
        self.rx_init = np.deg2rad(rx_init)
        self.ty_init = ty_init
        self.sample_traj = None
        self.desired_pos = None
        self.desired_weights = None
        self.model, self.graph_attr = model, graph_attr
        self.horizon = total_steps
        self.device = torch.device(device)
        self.collective_device = None   # where the broadcast / all-gather payloads live; None: self.device (RCCL).  "cpu" for gloo
        self.scale_rot, self.scale_ty = scale_rot, scale_ty
        self.nr_traj_points = traj_points
        self.traj_points = int(self.horizon / self.nr_traj_points)
        self.alpha, self.beta, self.gamma, self.penalty, self.rho = alpha, beta, gamma, penalty, rho
        self.max_rot = np.deg2rad(max_rot)
        self.max_ty = max_ty
        self.total_steps = total_steps
        # limits of the boundary penalties (traj_utils.py:57-61)
        self.left_limit, self.right_limit = 0.3, 0.7
        self.scale_ty = (self.ty_init[0] - self.left_limit) / self.scale_rot
        self.rotation_limit = 2.8973
        obs = self.initial_state[0]
        mat = graph_attr.material_idx[0]
        c0 = graph_attr.cartesian_idx[0]
        self.rigid_particles_idx = obs[-1, :, mat] == 1
        self.coffee_particles_idx = obs[-1, :, mat] == 0
        self._coffee_rows = torch.nonzero(self.coffee_particles_idx).reshape(-1)   # taken once: a boolean-mask index synchronises per use
        self.rigid_particles = obs[-1, self.rigid_particles_idx, c0:c0 + 3].contiguous()
        self.loss = SamplesLoss(loss="sinkhorn", p=2, blur=.05)
        self.cma_options = cmaes.CMAOptions()
        self.cma_options['seed'] = cma_rand
        self.cma_options['maxiter'] = cma_iter
        self.cma_options['popsize'] = cma_popsize
        self.cma_initial_var = cma_var
        self.candidates_per_gpu = int(candidates_per_gpu)
        k, n, dd = obs.shape
        self._mk_engine = lambda b: RolloutEngine(model, graph_attr, n, k_steps=k, data_dim=dd, device=self.device, candidates=b)
        self._engines = {}

    # ---- trajectory parametrisation (traj_utils.py:199-228)
    def set_sample_traj(self, sample_traj):
        sample_traj = np.asarray(sample_traj)
        d = sample_traj[2:] - sample_traj[1:-1]
        self.sample_traj = np.stack((np.deg2rad(d[:, 0] / self.scale_rot), d[:, 1] / self.scale_ty)).T

    def interpolate_trajectory(self, x):
        return interpolate_trajectory(x, self.sample_traj.shape[0], self.rx_init, self.scale_rot, self.scale_ty, self.max_rot,
                                      self.max_ty)

    def get_rigid_body_trajectory_from_diff(self, x, demo=False):
        if demo:
            traj_rot, traj_ty = x[:, 0], x[:, 1]
        else:
            traj_rot, traj_ty = self.interpolate_trajectory(x)
        traj = get_rigid_body_trajectory(traj_rot, traj_ty, self.horizon, self.ty_init, self.rigid_particles)
        actions = np.zeros((self.horizon, 2))
        actions[:, 0] = traj_rot[:self.horizon]
        actions[:, 1] = traj_ty[:self.horizon]
        return traj, actions

    # ---- loss terms (traj_utils.py:161-165,230-285)
    @staticmethod
    def compute_vel_acc(actions):
        return actions[1:, :] - actions[:-1, :], actions[2:, :] - 2 * actions[1:-1, :] + actions[:-2, :]

    def compute_vel_loss(self, vel):
        return float(np.linalg.norm(vel / np.array([self.max_rot, self.max_ty])[None, :]))

    def compute_acc_loss(self, acc):
        return float(np.linalg.norm(acc / np.array([self.max_rot, self.max_ty])[None, :]))

    def compute_boundaries_penalty(self, actions):
        rot = actions[:, 0]
        if rot.max() > self.rx_init + self.rotation_limit or rot.min() < self.rx_init - self.rotation_limit:
            return 20.0
        return 0.0

    def compute_loss(self, end_position, actions, cup_states=None, coffee_states=None, x=None):
        """traj_utils.py:275-285 for one candidate (one device loss, one transfer)."""
        return self._assemble_loss(float(self._wasserstein(end_position).item()), actions, x)

    def set_density_target(self, cloud, cell):
        """The goal as a density: ``density_target(cloud, cell)`` becomes ``desired_pos`` and ``desired_weights``."""
        centres, weights = density_target(torch.as_tensor(cloud, dtype=torch.float32, device=self.device), cell)
        self.desired_pos, self.desired_weights = centres.contiguous(), weights.contiguous()

    def _wasserstein(self, end):
        """The loss of one end cloud [Nc, 3] (uniform) against the goal, weighted where ``desired_weights`` is set (the batched calls
        pass ``b=self.desired_weights`` themselves)."""
        if self.desired_weights is None:
            return self.loss(end, self.desired_pos)
        return self.loss(None, end, self.desired_weights, self.desired_pos)

    def _assemble_loss(self, wasserstein_loss, actions, x=None):
        """Everything of compute_loss but the Wasserstein term itself: host float64 like the reference."""
        vel, acc = self.compute_vel_acc(actions)
        vel_loss, acc_loss = self.compute_vel_loss(vel), self.compute_acc_loss(acc)
        bound_penalty = self.compute_boundaries_penalty(actions)
        loss = self.beta * wasserstein_loss + self.penalty * bound_penalty + self.alpha * vel_loss + self.gamma * acc_loss
        return loss, wasserstein_loss, vel_loss, acc_loss, bound_penalty, 0.0

    # ---- objective
    def _engine(self, b):
        if b not in self._engines:
            self._engines[b] = self._mk_engine(b)
        return self._engines[b]

    def _end_positions(self, final_states):
        """final_states [B, k, N, D] -> the coffee particles' end positions [B, Nc, 3] (traj_utils.py:154-155)."""
        c0 = self.graph_attr.cartesian_idx[0]
        return final_states[:, -1].index_select(1, self._coffee_rows)[:, :, c0:c0 + 3].contiguous()

    def cma_objective(self, x):
        """traj_utils.py:114-159 for one candidate."""
        return self._local_losses([np.asarray(x, dtype=np.float64)])[0]

    def _block_ends(self, xs):
        """Block-diagonal batched rollout of the candidates xs: their end clouds [B, Nc, 3] (device) and action arrays."""
        trajs, acts = zip(*[self.get_rigid_body_trajectory_from_diff(x) for x in xs])
        eng = self._engine(len(xs))
        with torch.no_grad():
            finals = eng.rollout_candidates(self.initial_state[0].contiguous(), torch.stack(trajs), horizon=self.horizon)
        return self._end_positions(finals), list(acts)

    def population_losses(self, X):
        """Losses of a whole generation.  Under torch.distributed rank 0's X is broadcast and every rank evaluates
        a contiguous block; returns the full list on every rank."""
        import torch.distributed as dist
        X = [np.asarray(x, dtype=np.float64) for x in X]
        world = dist.get_world_size() if (dist.is_available() and dist.is_initialized()) else 1
        if world > 1:
            ev = CandidateEvaluator(None, result_dim=1, device=self.collective_device or self.device)
            return ev.evaluate_blocks(X, self._local_losses).reshape(-1).tolist()
        return self._local_losses(X)

    _loss_takes_x = False   # InterpolatedCMAsolver.compute_loss reads the search variables too

    def _local_losses(self, X):
        """This rank's candidates: rollouts in blocks of `candidates_per_gpu`, then the Wasserstein terms of ALL of them in one
        batched launch sequence (SamplesLoss.batched) and ONE transfer of the values; the penalty terms on the host."""
        if not len(X):
            return []
        ends, acts = [], []
        for b in range(0, len(X), self.candidates_per_gpu):
            e, a = self._block_ends(X[b:b + self.candidates_per_gpu])
            ends.append(e)
            acts += a
        w = self.loss.batched(torch.cat(ends), self.desired_pos, b=self.desired_weights).double().cpu().numpy()
        return [self._assemble_loss(float(w[i]), acts[i], X[i] if self._loss_takes_x else None)[0] for i in range(len(X))]

    # ---- gradient of the objective
    def loss_and_grad(self, x, edges=None, sweep="autograd"):
        """The objective of ``cma_objective(x)`` and its gradient with respect to the search vector: (loss: float, grad: array like
        x).  The map from x to the poses is restated in float64 torch (``interpolate_trajectory_torch``: clip, running sums;
        ``rigid_body_trajectory``), the rollout is ``RolloutEngine.differentiable_rollout`` (memory of one step's tape whatever the
        horizon; the model's parameters are constants), the end cloud goes into the differentiable ``SamplesLoss``, and the
        velocity / acceleration norms are float64 torch.  The boundary penalty is piecewise constant in x: it is added to the
        value and contributes nothing to the gradient.  ``population_loss_and_grad`` is this call for a block of candidates at once,
        ``refine`` the projected Adam that runs on it.
        edges: a list that receives the ``edge_index`` of every step of the backward's recomputation (diagnostics, tests).
        sweep: ``differentiable_rollout``'s keyword -- "library" runs the rollout's reverse sweep as one library call (and hands out no
        edge lists: ``edges`` must then be None)."""
        x_np = np.asarray(x, dtype=np.float64)
        xt = torch.tensor(x_np.reshape(-1), dtype=torch.float64, requires_grad=True)
        rot, ty = interpolate_trajectory_torch(xt, self.sample_traj.shape[0], float(self.rx_init), self.scale_rot, self.scale_ty,
                                               float(self.max_rot), self.max_ty)
        h = self.horizon
        traj = rigid_body_trajectory(rot, ty, h, self.ty_init, self.rigid_particles)
        out = self._engine(1).differentiable_rollout(self.initial_state[0].contiguous(), traj, horizon=h, return_edges=edges is not None,
                                                     sweep=sweep)
        final, step_edges = out if edges is not None else (out, None)
        c0 = self.graph_attr.cartesian_idx[0]
        end = final[-1].index_select(0, self._coffee_rows)[:, c0:c0 + 3]
        wasserstein = self._wasserstein(end).double().cpu()
        actions = torch.stack((rot[:h], ty[:h]), dim=1)
        limits = torch.tensor([float(self.max_rot), float(self.max_ty)], dtype=torch.float64)
        vel = actions[1:] - actions[:-1]
        acc = actions[2:] - 2 * actions[1:-1] + actions[:-2]
        loss = self.beta * wasserstein + self.alpha * torch.linalg.norm(vel / limits) + self.gamma * torch.linalg.norm(acc / limits)
        loss.backward()
        if edges is not None:
            edges[:] = step_edges
        bound_penalty = self.compute_boundaries_penalty(actions.detach().numpy())
        return float(loss.detach()) + self.penalty * bound_penalty, xt.grad.numpy().reshape(x_np.shape)

    def _block_loss_and_grad(self, xs, sweep):
        """``loss_and_grad`` of the candidates xs (at most a block) through ONE block-diagonal rollout: every candidate has its own
        float64 leaf and pose chain, the poses are laid side by side along the rigid axis ([h, B Nr, 3], ``rollout_candidates``'
        layout) and the initial state B times along the node axis; one ``differentiable_rollout`` on ``_engine(B)``, one batched
        Sinkhorn call, one backward of the sum of the B objectives.  No term couples two candidates, so each leaf receives the
        gradient of its own objective."""
        b, h, n_points = len(xs), self.horizon, self.sample_traj.shape[0]
        leaves = [torch.tensor(x.reshape(-1), dtype=torch.float64, requires_grad=True) for x in xs]
        chains = [interpolate_trajectory_torch(xt, n_points, float(self.rx_init), self.scale_rot, self.scale_ty, float(self.max_rot),
                                               self.max_ty) for xt in leaves]
        traj = torch.cat([rigid_body_trajectory(rot, ty, h, self.ty_init, self.rigid_particles) for rot, ty in chains], dim=1)
        eng = self._engine(b)
        obs = self.initial_state[0]
        obs = obs.unsqueeze(1).repeat(1, b, 1, 1).reshape(eng.k, b * eng.n_per, eng.data_dim).contiguous()
        final = eng.differentiable_rollout(obs, traj, horizon=h, sweep=sweep)
        c0 = self.graph_attr.cartesian_idx[0]
        ends = final[-1].reshape(b, eng.n_per, eng.data_dim).index_select(1, self._coffee_rows)[:, :, c0:c0 + 3]
        wasserstein = self.loss.batched(ends, self.desired_pos, b=self.desired_weights).double().cpu()
        limits = torch.tensor([float(self.max_rot), float(self.max_ty)], dtype=torch.float64)
        losses, penalties = [], []
        for i, (rot, ty) in enumerate(chains):
            actions = torch.stack((rot[:h], ty[:h]), dim=1)
            vel = actions[1:] - actions[:-1]
            acc = actions[2:] - 2 * actions[1:-1] + actions[:-2]
            losses.append(self.beta * wasserstein[i] + self.alpha * torch.linalg.norm(vel / limits) + self.gamma * torch.linalg.norm(acc / limits))
            penalties.append(self.compute_boundaries_penalty(actions.detach().numpy()))
        torch.stack(losses).sum().backward()
        return [float(l.detach()) + self.penalty * p for l, p in zip(losses, penalties)], [xt.grad.numpy() for xt in leaves]

    def _local_loss_and_grad(self, X, sweep="library"):
        """This rank's candidates in blocks of ``candidates_per_gpu`` (the last one may be shorter): (losses [P], grads [P, dim])."""
        X = np.asarray(X, dtype=np.float64)
        losses, grads = [], []
        for b in range(0, len(X), self.candidates_per_gpu):
            l, g = self._block_loss_and_grad(list(X[b:b + self.candidates_per_gpu]), sweep)
            losses += l
            grads += g
        return np.asarray(losses, dtype=np.float64), np.asarray(grads, dtype=np.float64).reshape(X.shape)

    def population_loss_and_grad(self, X, sweep="library"):
        """``loss_and_grad`` of a whole population: (losses [P], grads [P, dim]) as float64 arrays, row p what
        ``loss_and_grad(X[p], sweep=sweep)`` returns, from one block-diagonal rollout, one reverse sweep and one batched Sinkhorn
        call per block of ``candidates_per_gpu`` candidates.  Under torch.distributed rank 0's X is broadcast, every rank takes
        a contiguous block, and the [loss, grad...] rows are all-gathered (``population_losses``' pattern)."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            def rows_of(xs):
                losses, grads = self._local_loss_and_grad(xs, sweep)
                return list(np.concatenate((losses[:, None], grads), axis=1))

            ev = CandidateEvaluator(None, result_dim=1 + 2 * self.sample_traj.shape[0], device=self.collective_device or self.device)
            rows = ev.evaluate_blocks(X, rows_of)
            return rows[:, 0].copy(), rows[:, 1:].copy()
        return self._local_loss_and_grad(X, sweep)

    def box_half_widths(self):
        """Per search variable, the half-width of the box outside which ``interpolate_trajectory`` clips the increment (beyond it
        the objective is flat in that variable): max_rot / scale_rot for the rotation entries, max_ty / scale_ty for the
        translation entries, float64."""
        n_points = self.sample_traj.shape[0]
        return np.concatenate((np.full(n_points, abs(float(self.max_rot) / float(self.scale_rot))),
                               np.full(n_points, abs(float(self.max_ty) / float(self.scale_ty)))))

    def refine(self, X0, iters=20, lr=0.01, betas=(0.9, 0.999), eps=1e-8, sweep="library"):
        """Gradient refinement of P trajectories at once: ``projected_adam`` on ``population_loss_and_grad``, in variables
        normalised by ``box_half_widths()`` and clamped to that box after every update (and before the first evaluation: outside
        it the gradient is zero and a start would never move).  ``lr`` is in those units: a step moves a variable by at most about
        ``lr`` of its admissible increment.  Returns (x_best [P, dim], f_best [P], info): per start the best iterate by the full
        objective, boundary penalty included, the start itself (clamped) being iterate 0; info["f"] [P, iters + 1] holds the
        objective sequences.  The values are the sweep's forward, the inference rollout: ``cma_objective``'s.  ``iters + 1``
        gradient evaluations; deterministic.  Under torch.distributed rank 0's starts are broadcast and each rank refines its
        block on its own, with one all-gather at the end (``refine_starts``)."""
        return refine_starts(lambda xs: self._local_loss_and_grad(xs, sweep), X0, self.box_half_widths(), iters=iters, lr=lr, betas=betas,
                             eps=eps, collective_device=self.collective_device or self.device)

    def _start_point(self):
        """The search starts at the sample trajectory: all rotation variables, then all translation variables."""
        return np.ascontiguousarray(self.sample_traj.T, dtype=np.float64).reshape(-1)

    def optimize_trajectory(self, desired_position, refine=None):
        """traj_utils.py:247-259.  refine: None, or the keywords of ``refine`` as a dict (``iters``, ``lr``, ``sweep``): after the
        search, ``es.result.xbest`` and ``es.result.xfavorite`` are refined together, the refined points are ranked against
        ``xbest`` by the search's own objective (one more ``population_losses`` call), and the best of the three is returned in
        ``xbest``'s place -- a refined point only where its objective is strictly below ``es.result.fbest``.
        ``es.refined = {"x", "f", "info"}`` keeps what ``refine`` returned."""
        from . import cmaes
        initial_traj = self._start_point()
        self.desired_pos = desired_position.clone()
        xopt, es = cmaes.fmin2(self.cma_objective, initial_traj.tolist(), self.cma_initial_var, options=self.cma_options,
                               parallel_objective=self.population_losses)
        if refine is None:
            return xopt, es
        x, f, info = self.refine(np.stack((np.asarray(es.result.xbest, dtype=np.float64), np.asarray(es.result.xfavorite, dtype=np.float64))),
                                 **refine)
        es.refined = {"x": x, "f": f, "info": info}
        ranked = self.population_losses(list(x))
        best = int(np.argmin(ranked))
        return (x[best].copy(), es) if ranked[best] < es.result.fbest else (xopt, es)


class InterpolatedCMAsolver(TrajectoryCMAsolver):
    """Mirror of the reference's ``InterpolatedCMAsolver`` (traj_utils.py:288-452): the search variables are key
    points (every ``traj_points``-th step) of the rotation / translation, PCHIP-interpolated to one pose per step;
    increments between key points are constrained (``ineq_constraint``, solved with ``cmaes.fmin_con``) and the
    rotation is box-bounded.  Objective evaluation (batched rollouts, device loss) is inherited."""

    def set_sample_traj(self, sample_traj):
        """traj_utils.py:296-304: the key points are every ``traj_points``-th pose after the first, as offsets from the
        initial pose in search-variable units (column 0 rotation [deg in the file], column 1 translation)."""
        keys = np.asarray(sample_traj, dtype=np.float64)[self.nr_traj_points::self.nr_traj_points]
        offset = np.array([self.rx_init, self.ty_init[0]])
        scale = np.array([self.scale_rot, self.scale_ty])
        self.sample_traj = (np.column_stack((np.deg2rad(keys[:, 0]), keys[:, 1])) - offset) / scale

    def interpolate_trajectory(self, x, type_interp='pchip'):
        from scipy.interpolate import interp1d, pchip_interpolate
        x = np.asarray(x, dtype=np.float64)
        k = self.sample_traj.shape[0]
        rot_points = [self.rx_init] + (self.rx_init + x[:k] * self.scale_rot).tolist()
        ty_points = [0.0] + (x[k:] * self.scale_ty).tolist()
        traj_idx = np.arange(0, self.horizon + 1, self.nr_traj_points)
        idx_interp = np.arange(self.horizon)
        if type_interp == 'cubic':
            return (interp1d(x=traj_idx, y=rot_points, kind='cubic')(idx_interp),
                    interp1d(x=traj_idx, y=ty_points, kind='cubic')(idx_interp))
        return pchip_interpolate(traj_idx, rot_points, idx_interp), pchip_interpolate(traj_idx, ty_points, idx_interp)

    def compute_acc_loss(self, acc):
        return float(np.linalg.norm(acc / np.array([2.2e-4, 1.45e-4])[None, :]))  # fixed means, traj_utils.py:343-353

    def compute_vel_loss(self, vel):
        return float(np.linalg.norm(vel / np.array([1e-2, 4e-4])[None, :]))        # traj_utils.py:355-364

    def compute_vel_noninterp(self, x):
        x = np.asarray(x, dtype=np.float64)
        rot, ty = x[:self.traj_points] * self.scale_rot, x[self.traj_points:] * self.scale_ty
        ineq_rot = np.abs(rot[1:] - rot[:-1]) - self.max_rot * self.nr_traj_points
        ineq_ty = np.abs(ty[1:] - ty[:-1]) - self.max_ty * self.nr_traj_points
        return float(np.exp(max(ineq_rot.max(), ineq_ty.max())))

    def ineq_constraint(self, x):
        x = np.asarray(x, dtype=np.float64)
        actions = np.zeros((self.traj_points + 1, 2))
        actions[1:, 0] = x[:self.traj_points] * self.scale_rot
        actions[1:, 1] = x[self.traj_points:] * self.scale_ty
        vel, _ = self.compute_vel_acc(actions)
        upper = np.abs(vel) - np.array([self.max_rot * self.nr_traj_points, self.max_ty * self.nr_traj_points])
        return np.concatenate((upper[:, 0] / self.scale_rot, upper[:, 1] / self.scale_ty))

    def loss_and_grad(self, x):
        raise NotImplementedError("loss_and_grad: the PCHIP parametrisation (scipy, on the host) has no gradient")

    def population_loss_and_grad(self, X, sweep="library"):
        raise NotImplementedError("population_loss_and_grad: the PCHIP parametrisation (scipy, on the host) has no gradient")

    def refine(self, X0, **kwargs):
        raise NotImplementedError("refine: the PCHIP parametrisation (scipy, on the host) has no gradient")

    _loss_takes_x = True

    def _assemble_loss(self, wasserstein_loss, actions, x=None):
        vel, acc = self.compute_vel_acc(actions)
        vel_loss, acc_loss = self.compute_vel_loss(vel), self.compute_acc_loss(acc)
        interp_loss = self.compute_vel_noninterp(x) if x is not None else 0.0
        loss = self.beta * wasserstein_loss + self.alpha * vel_loss + self.gamma * acc_loss + self.rho * interp_loss
        return loss, wasserstein_loss, vel_loss, acc_loss, interp_loss, 0.0

    def optimize_trajectory(self, desired_position):
        """traj_utils.py:324-337."""
        from . import cmaes
        self.cma_options['bounds'] = [-self.rotation_limit / self.scale_rot, self.rotation_limit / self.scale_rot]
        initial_traj = self._start_point()
        self.desired_pos = desired_position.clone()
        return cmaes.fmin_con(self.cma_objective, initial_traj.tolist(), self.cma_initial_var, g=self.ineq_constraint,
                              options=self.cma_options, parallel_objective=self.population_losses)
