"""Cases and the numpy restatement of the optimiser driven through the contribution door (csrc/train_step.hip: gm_rank_sum,
gm_grad_sumsq, the apply scalars, adam_flat_kernel; gnn_manip_amd/train.py: Trainer.zero_grad / reduce / apply) -- a plain helper
module (no test) of tests/test_optim_cases.py (CPU) and tests/test_gpu_optim.py (the kernels against the restatement, bit for bit).

A contribution is a caller-made buffer: `alloc` float32 gradients laid out like the model's flat weight buffer, and a 32-byte tail.
zero_grad(), reduce(gathered, samples_total), apply() therefore run the rank sum, the norm, the apply scalars and Adam on ANY
gradients, with no forward or backward -- chosen here for what real model gradients never reach in a few steps: second moments in
the float32 denormal range and at inf, moments decaying under zero gradients, non-finite elements, and a flat buffer longer than
one pass of the flat kernels' grid (GRID_PASS floats)."""
import math

import numpy as np

import train_accum_cases as ac
import train_dp_cases as dp
import train_step_cases as sc

GRID_PASS = 2048 * 256 * 4      # floats the flat kernels (adam_flat_kernel, rank_sum_kernel) walk in ONE pass of their capped grid
TAIL_MODELS = tuple((25, 4, od, 64, 2, 2) for od in (1, 2, 3, 4))        # flat count % 4 == 1, 2, 3, 0
BIG = (25, 4, 3, 256, 2, 3)                                               # GRID_PASS < flat count < 2 * GRID_PASS
OD3 = TAIL_MODELS[2]
STEPS = 12
F32_TINY = float(np.finfo(np.float32).tiny)


# ---------------------------------------------------------------------------------------------- the flat layout
class Layout:
    """Per-tensor offset and count in the flat buffer: every tensor starts on 16 bytes; `count` is the end of the last tensor
    (what Adam walks), `alloc` is `count` rounded up to four floats (the buffer, and a contribution's gradient part)."""

    def __init__(self, dims):
        self.dims, self.shapes = tuple(dims), sc.tensor_shapes(dims)
        self.offsets, self.counts, off = [], [], 0
        for s in self.shapes:
            n = int(np.prod(s))
            self.offsets.append(off)
            self.counts.append(n)
            off += (n + 3) & ~3
        self.count = self.offsets[-1] + self.counts[-1]
        self.alloc = (self.count + 3) & ~3
        self.used = np.zeros(self.alloc, bool)
        for o, n in zip(self.offsets, self.counts):
            self.used[o:o + n] = True

    def to_flat(self, tensors):
        flat = np.zeros(self.alloc, np.float32)
        for o, n, a in zip(self.offsets, self.counts, tensors):
            flat[o:o + n] = np.asarray(a, np.float32).reshape(-1)
        return flat

    def from_flat(self, flat):
        return [np.asarray(flat)[o:o + n].reshape(s) for o, n, s in zip(self.offsets, self.counts, self.shapes)]

    def packed(self, flat):
        """The tensors' elements without the gaps: what the exported tensors hold, one after the other."""
        return np.asarray(flat)[self.used]

    def beyond(self, floats):
        """Indices of the tensors that lie wholly at or beyond float `floats` of the flat buffer."""
        return [i for i, o in enumerate(self.offsets) if o >= floats]


# ---------------------------------------------------------------------------------------------- gradient schedules
SCHEDULES = ("mixed", "tiny", "huge", "decay", "spike")
ALWAYS_ZERO = 7                    # the first elements of `mixed` are zero at every step
SPIKE_STEP = 2
# the seeds below were chosen once so that tests/test_optim_cases.py's conditions hold with room to spare; they are part of the cases
SEEDS = {"mixed": 21, "tiny": 22, "huge": 23, "decay": 24, "spike": 21}


def _log_uniform(rng, lo, hi, shape):
    return (10.0 ** rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)


def spike_places(lay):
    """(element of the +inf, element of the NaN) of `spike`: one in the 16-byte groups, one in the last tensor (the scalar tail)."""
    return lay.offsets[3] + 5, lay.count - 1


def schedule(name, lay, steps=STEPS, rank=0):
    """[steps, alloc] float32, zero in the gaps.  `rank`: another draw of the same law, for a further rank's row."""
    rng = np.random.default_rng([SEEDS[name], SCHEDULES.index("mixed" if name == "spike" else name), lay.alloc, rank])
    shape = (steps, lay.alloc)
    if name in ("mixed", "decay", "spike"):                  # train_step_cases.adam_gradients' law
        g = _log_uniform(rng, -6, 1, shape)
        g[rng.random(shape) < 0.1] = 0.0
        g[:, :ALWAYS_ZERO] = 0.0
        if name == "decay":
            g[1:] = 0.0
        if name == "spike" and rank == 0:
            where_inf, where_nan = spike_places(lay)
            g[SPIKE_STEP, where_inf] = np.inf
            g[SPIKE_STEP, where_nan] = np.nan
    elif name == "tiny":
        g = _log_uniform(rng, -30, -15, shape)
    elif name == "huge":
        g = _log_uniform(rng, 15, 22, shape)
    else:
        raise KeyError(name)
    g[:, ~lay.used] = 0.0
    return g


def rank_rows(name, lay, steps, world):
    """[steps, world, alloc]: one draw of the schedule per rank; the mini-batch's gradient is their float32 sum in rank order."""
    return np.stack([schedule(name, lay, steps, rank=r) for r in range(world)], axis=1)


def tails_of(samples_total, world, steps_applied, bad=0):
    """The ranks' tails (samples, bad, loss_sum, steps_applied): the samples shared out in blocks, a loss per rank."""
    base, rem = divmod(int(samples_total), world)
    out = []
    for r in range(world):
        s = base + (1 if r < rem else 0)
        out.append((s, bad if r == world - 1 else 0, 0.37 * s + 0.011 * r, int(steps_applied)))
    return out


def start_weights(lay, seed=29):
    w = np.random.default_rng([seed, lay.alloc]).standard_normal(lay.alloc).astype(np.float32)
    w[~lay.used] = 0.0
    return w


def start_state(lay, weights=None, m=None, v=None, steps=0, betas=(0.9, 0.999)):
    """The state the restated drive works on: flat float32 arrays and the trainer's record."""
    z = lambda a: np.zeros(lay.alloc, np.float32) if a is None else np.asarray(a, np.float32).copy()
    b1p, b2p = running_powers_fixed(betas[0], betas[1], steps)
    return {"p": start_weights(lay) if weights is None else np.asarray(weights, np.float32).copy(), "m": z(m), "v": z(v),
            "b1p": b1p, "b2p": b2p, "steps": int(steps), "skipped": 0}


def late_moments(lay, seed=31):
    """Moments of a run that has gone on for a while: a random exp_avg and a positive exp_avg_sq spanning 1e-12 .. 1e2."""
    rng = np.random.default_rng([seed, lay.alloc])
    m = (rng.standard_normal(lay.alloc) * 10.0 ** rng.uniform(-6, 0, lay.alloc)).astype(np.float32)
    v = (10.0 ** rng.uniform(-12, 2, lay.alloc)).astype(np.float32)
    m[~lay.used] = 0.0
    v[~lay.used] = 0.0
    return m, v


# ---------------------------------------------------------------------------------------------- the restated drive
def _flush(x):
    return np.where(np.abs(x) < np.float32(F32_TINY), np.float32(0.0), x).astype(np.float32)


def adam_variant(p, g, state, lr, betas, eps, wrong=None):
    """train_step_cases.adam_restated on flat arrays, in place on `state`; `wrong` names ONE treatment the contract rules out:
    "m_once" (the first moment rounded once, as a contracted multiply-add would), "v_order" (o2 * (g * g)), "flush" (denormal
    gradients and moments flushed to zero).  wrong=None IS adam_restated (tests/test_optim_cases.py holds it to that)."""
    f = np.float32
    state["b1p"] *= betas[0]
    state["b2p"] *= betas[1]
    state["steps"] += 1
    step = f(lr / (1.0 - state["b1p"]))
    s2 = f(math.sqrt(1.0 - state["b2p"]))
    b1, o1, b2, o2, e = f(betas[0]), f(1.0 - betas[0]), f(betas[1]), f(1.0 - betas[1]), f(eps)
    if wrong == "flush":
        g = _flush(g)
    if wrong == "m_once":      # both products are exact in float64: one rounding of the sum to 53 bits, then one to 24
        m = (np.float64(b1) * state["m"].astype(np.float64) + np.float64(o1) * g.astype(np.float64)).astype(f)
    else:
        m = (b1 * state["m"]) + (o1 * g)
    if wrong == "v_order":
        v = (b2 * state["v"]) + (o2 * (g * g))
    else:
        v = (b2 * state["v"]) + ((o2 * g) * g)
    if wrong == "flush":
        m, v = _flush(m), _flush(v)
    state["m"], state["v"] = m, v
    state["p"] = p - step * (m / ((np.sqrt(v) / s2) + e))
    assert state["p"].dtype == f and m.dtype == f and v.dtype == f


def drive_restated(state, rows, tails, samples_total, lr, max_grad_norm=None, betas=(0.9, 0.999), eps=1e-8, want_norm=False,
                   wrong=None):
    """One mini-batch on arrays, in place on `state` (start_state): gm_trainer_reduce of the rank rows [world, alloc] and tails,
    then gm_trainer_apply.  Returns the mini-batch's record {'samples', 'bad', 'loss_sum', 'grad_norm', 'scale', 'loss', 'skipped',
    'grad', 'g1'}.  The header's skip rule: bad > 0, or a REQUESTED norm that is not finite; without a requested norm a non-finite
    gradient goes through.  `wrong`: adam_variant's, or "reversed" (the rank rows added from the last rank to the first)."""
    rows = np.ascontiguousarray(rows, np.float32)
    with np.errstate(all="ignore"):
        grad = dp.rank_sum_restated(rows[::-1] if wrong == "reversed" else rows)
        rec = dp.merge_restated(tails, samples_total)
        S = rec["samples"]
        have_norm = ac.clipping(max_grad_norm) or want_norm
        norm = ac.norm_of([grad], S) if have_norm else float("nan")
        scale = ac.scale_of(norm, S, max_grad_norm)
        skip = rec["bad"] > 0 or (have_norm and not math.isfinite(norm))
        rec.update(grad_norm=norm, scale=float(scale), loss=float("nan") if skip else rec["loss_sum"] / float(S), skipped=skip, grad=grad,
                   g1=None)
        if skip:
            state["skipped"] += 1
            return rec
        rec["g1"] = np.float32(scale) * grad
        if wrong in (None, "reversed"):
            inner = {"m": [state["m"]], "v": [state["v"]], "b1p": state["b1p"], "b2p": state["b2p"], "steps": state["steps"]}
            state["p"] = ac.scaled_adam_restated([state["p"]], [grad], inner, lr, scale, betas, eps)[0]
            state.update(m=inner["m"][0], v=inner["v"][0], b1p=inner["b1p"], b2p=inner["b2p"], steps=inner["steps"])
        else:
            adam_variant(state["p"], rec["g1"], state, lr, betas, eps, wrong)
    return rec


def denormals(x):
    x = np.abs(np.asarray(x, np.float32))
    return int(((x > 0) & (x < np.float32(F32_TINY))).sum())


def census(state, lay):
    """{array: (denormal, inf, NaN) entries} of the tensors of a state."""
    out = {}
    for key in ("p", "m", "v"):
        a = lay.packed(state[key])
        out[key] = (denormals(a), int(np.isinf(a).sum()), int(np.isnan(a).sum()))
    return out


def words_differing(a, b):
    """Words of two float32 arrays that differ, a NaN on both sides counting as equal."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return int(((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))).sum())


# ---------------------------------------------------------------------------------------------- the beta powers
def running_powers(beta1, beta2, steps):
    """The trainer's beta powers after `steps` steps: running products, the plain loop."""
    b1p = b2p = 1.0
    for _ in range(int(steps)):
        b1p *= beta1
        b2p *= beta2
    return b1p, b2p


def running_powers_fixed(beta1, beta2, steps):
    """The same, stopping once neither product changes any more: a product ends at a fixed point of the rounded multiplication --
    zero for a beta up to 0.5, a non-zero denormal above it."""
    b1p = b2p = 1.0
    for _ in range(int(steps)):
        if b1p * beta1 == b1p and b2p * beta2 == b2p:
            break
        b1p *= beta1
        b2p *= beta2
    return b1p, b2p
