"""Cases and numpy restatements of mini-batches and gradient clipping in the library (csrc/train_step.hip: gm_trainer_begin,
gm_train_step_accumulate, gm_train_rollout_accumulate, gm_trainer_apply, gm_grad_sumsq; the contract is in
include/gnn_manip_hip.h) -- a plain helper module (no test) of tests/test_train_accum_cases.py (CPU: the restatements against
torch's clip_grad_norm_ and Adam, the regimes of the GPU cases), tests/test_abi_train_accum.py and tests/test_gpu_train_accum.py
(the kernels against the restatements, bit for bit).

gm_trainer_apply, from the SUM g of S samples' gradients, with float64 scalars:
    norm  = sqrt(sumsq(g)) / S                                        -- the norm of the mean gradient
    coef  = min(1.0, max_grad_norm / (norm + 1e-6)) when 0 < max_grad_norm < inf, else 1.0      (clip_grad_norm_'s formula)
    scale = float32(coef / S)
then per element g1 = scale * g in float32, rounded on its own, and train_step_cases.adam_restated on g1.  The loss of an update
is the running sum of its samples' losses, in arrival order, divided by S."""
import functools
import math

import numpy as np

import train_step_cases as sc

# ---------------------------------------------------------------------------------------------- gm_grad_sumsq
SUMSQ_WG, SUMSQ_GRID_MAX = 256, 128      # threads of a workgroup, workgroups at most: the loss kernels' geometry
# around one workgroup and its float4 groups; 128 x 256 threads with one element each; 128 x 256 threads with one float4 each
SUMSQ_COUNTS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 32_767, 32_768, 32_769, 131_071, 131_072, 131_077)
# the float64 sum of non-negative terms: at most (elements per thread + tree depths) x 2^-53 relative -- below 3e-14 for these
# counts and for the largest model (6 M parameters: 183 elements per thread, 8 + 7 levels of the two trees)
SUMSQ_RTOL = 1e-12


def sumsq_case(count, seed=0):
    return np.random.default_rng([seed, count]).standard_normal(count).astype(np.float32)


def sumsq_exact(x):
    """math.fsum of the float64 squares: the correctly rounded sum."""
    return math.fsum((np.asarray(x, np.float32).astype(np.float64) ** 2).tolist())


# ---------------------------------------------------------------------------------------------- the apply arithmetic
def clipping(max_grad_norm):
    return max_grad_norm is not None and 0.0 < float(max_grad_norm) < float("inf")


def clip_coef(norm, max_grad_norm):
    """float64: what multiplies the mean gradient."""
    return min(1.0, float(max_grad_norm) / (float(norm) + 1e-6)) if clipping(max_grad_norm) else 1.0


def scale_of(norm, samples, max_grad_norm):
    """float32: what multiplies every element of the SUM of `samples` gradients whose mean has the float64 norm `norm`."""
    return np.float32(clip_coef(norm, max_grad_norm) / float(samples))


def norm_of(grads, samples):
    """float64: the norm of the mean of `samples` gradients whose sum is `grads` (a list of arrays)."""
    return math.sqrt(math.fsum(sumsq_exact(np.asarray(g, np.float32).reshape(-1)) for g in grads)) / float(samples)


def scaled_adam_restated(params, grads, state, lr, scale, betas=(0.9, 0.999), eps=1e-8):
    """gm_trainer_apply's update: g1 = scale * g in float32, rounded on its own, then the library's Adam on g1."""
    scale = np.float32(scale)
    g1 = [scale * np.asarray(g, np.float32) for g in grads]
    assert all(g.dtype == np.float32 for g in g1)
    return sc.adam_restated(params, g1, state, lr, betas, eps)


def mean_loss(losses):
    """The loss of an update: the samples' losses added in arrival order, divided by their number, in float64."""
    total = 0.0
    for value in losses:
        total += float(value)
    return total / float(len(losses))


# ---------------------------------------------------------------------------------------------- the stub gradients of the CPU tests
STUB_SHAPES = ((64, 25), (64,), (3, 64), (3,), (17, 5))
STUB_SAMPLES, STUB_UPDATES, STUB_LR = 3, 6, 1e-3


def stub_gradients(seed=11):
    """[updates][samples][tensor] float32 gradients, of a magnitude that grows from update to update (0.01 .. 30 per element) so
    that a clip at STUB_MAX_NORM is inactive for the first updates and active for the last, and the start parameters."""
    rng = np.random.default_rng(seed)
    grads = [[[(10.0 ** (-2.0 + 0.7 * u) * rng.standard_normal(s)).astype(np.float32) for s in STUB_SHAPES] for _ in range(STUB_SAMPLES)]
             for u in range(STUB_UPDATES)]
    return grads, [rng.standard_normal(s).astype(np.float32) for s in STUB_SHAPES]


STUB_MAX_NORM = 5.0


# ---------------------------------------------------------------------------------------------- the mini-batch of the GPU tests
DIMS = sc.SMALL                                  # hidden 64, 2 layers, 2 message-passing steps
LR = 1e-3
# (nodes, side of the scene, seed): three sizes, one past a 256-row edge by one row, one below a tile
SAMPLES = ((257, 0.048, 411), (300, 0.05, 412), (64, 0.03, 413))
PARAM_SEED = 410


@functools.lru_cache(maxsize=None)
def sample(i):
    """(nodes, edge_attr, edge_index, target) of sample i, read-only."""
    n, side, seed = SAMPLES[i]
    nodes, ea, ei = sc.scene_graph(seed, n=n, side=side)
    out = (nodes, ea, ei, sc.step_target(nodes, DIMS[2], seed))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def params():
    from oracle import epd_oracle as orc
    return orc.init_params(*DIMS, PARAM_SEED)


@functools.lru_cache(maxsize=None)
def oracle_gradients(dtype_name="float64"):
    """(per-sample losses, {name: the SUM of the three samples' gradients}) of the float64 (or float32) oracle."""
    import torch
    from oracle import torch_epd
    losses, total = [], None
    for i in range(len(SAMPLES)):
        nodes, ea, ei, target = sample(i)
        _, loss, g = torch_epd.loss_and_grads(params(), nodes, ea, ei, target, DIMS[4], DIMS[5], getattr(torch, dtype_name))
        losses.append(loss)
        total = g if total is None else {k: total[k] + g[k] for k in g}
    return losses, total


def oracle_flip_allowance():
    """The ReLU flip allowance of the summed gradient: the samples' allowances added, per tensor; and the units behind them."""
    from oracle import torch_epd
    total, units = None, 0
    for i in range(len(SAMPLES)):
        nodes, ea, ei, target = sample(i)
        a, n_units = torch_epd.relu_flip_allowance(params(), nodes, ea, ei, target, DIMS[4], DIMS[5])
        total = a if total is None else {k: total[k] + a[k] for k in a}
        units += n_units
    return total, units


def oracle_norm():
    """The float64 norm of the oracle's MEAN gradient over the three samples."""
    _, g = oracle_gradients()
    return math.sqrt(sum(float((v.astype(np.float64) ** 2).sum()) for v in g.values())) / len(SAMPLES)


# The two regimes of the clip on that mini-batch: about half and about twice the oracle's norm (tests/test_train_accum_cases.py
# holds each to a factor 1.5 of the edge).
CLIP_ACTIVE, CLIP_INACTIVE = 0.5, 2.0
