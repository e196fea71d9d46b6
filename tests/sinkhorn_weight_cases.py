"""Seeded weighted point-cloud pairs for the weighted Sinkhorn kernels (csrc/sinkhorn.hip, gm_sinkhorn_divergence_weighted) -- a plain
helper module shared by test_sinkhorn_weight_cases.py (CPU) and test_gpu_sinkhorn_weights.py (GPU), beside sinkhorn_cases.py (whose
bars, bounding box and schedule length it imports).

A case is (x, y, a, b, blur, scaling): a cloud shape on the edges of the kernels' tiling (4 rows per wave, 16 per workgroup, 64
lanes), crossed with a weight pattern.  A side's weights may be None (uniform through the NULL pointer, the uniform kernel
instantiation): "dirichlet" is the planner's case, a uniform x against a weighted target, "one_point" a one-hot a against a
uniform y.  Every case runs with the bounding-box diameter and with DIAMETER_GIVEN.

float64_reference() is oracle.sinkhorn_divergence's algorithm with la = log a, lb = log b and the weighted means, dense and in the
log domain, with the gradient of the last extrapolation in closed form (autograd_gradient() is the same gradient by torch autograd,
held against it by the CPU tests).  Its sums run over the summed cloud one point after the other, so a term that is exactly +0
-- a zero-weight point -- changes no bit wherever it stands.  f32_restatement() is the kernels' arithmetic in numpy float32, in
the style of sinkhorn_cases.f32_restatement.

Pure numpy (PCG64): a seed gives the same case on every machine; only autograd_gradient uses torch."""
import functools
from dataclasses import dataclass

import numpy as np

import sinkhorn_cases as sc

F32 = sc.F32
DIAMETER_GIVEN = 0.8                                  # the `diameter=` variant of every case (the bounding boxes are 0.3 to 0.5)
SHAPES = ((150, 130), (17, 63), (64, 65), (1, 300))   # row tail of a wave and of a workgroup, lane tail of a sweep, a single point
PATTERNS = ("uniform", "dirichlet", "lognormal", "third_zero", "one_point", "multiplicity")


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _blob(rng, n, centre, spread):
    return (np.asarray(centre, np.float64) + spread * rng.standard_normal((n, 3))).astype(F32)


def weights(pattern, k, rng):
    """k float32 weights of a pattern; they sum to 1 up to float32 rounding (nothing downstream normalises them)."""
    if pattern == "uniform":
        w = np.full(k, 1.0 / k)
    elif pattern == "dirichlet":
        w = rng.dirichlet(np.ones(k))
    elif pattern == "lognormal":                      # sigma 3: about 1e-8 to 0.3 at k = 150
        w = rng.lognormal(0.0, 3.0, k)
    elif pattern == "third_zero":                     # every third weight zero (never the first: a cloud of one point keeps its mass)
        w = rng.uniform(0.5, 1.5, k)
        w[2::3] = 0.0
    elif pattern == "one_point":                      # one point carries everything
        w = np.zeros(k)
        w[k // 2] = 1.0
    elif pattern == "multiplicity":                   # integer multiplicities 1..4 over their sum
        w = rng.integers(1, 5, k).astype(np.float64)
    else:
        raise ValueError(pattern)
    return (w / w.sum()).astype(F32)


@dataclass(frozen=True)
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    a: np.ndarray          # [n] float32, or None: uniform
    b: np.ndarray          # [m] float32, or None
    blur: float = 0.05
    scaling: float = 0.5

    def diameter(self, given):
        return DIAMETER_GIVEN if given else None


def _build_cases():
    cases = []
    settings = [(n, m, 0.05, 0.5) for n, m in SHAPES] + [(150, 130, 0.02, 0.9)]
    for k, (n, m, blur, scaling) in enumerate(settings):
        rng = _rng(700 + k)
        x, y = _blob(rng, n, (0.45, 0.5, 0.5), 0.06), _blob(rng, m, (0.55, 0.5, 0.52), 0.05)
        for p, pattern in enumerate(PATTERNS):
            wr = _rng(7000 + 10 * k + p)
            a = None if pattern == "dirichlet" else weights(pattern, n, wr)
            b = None if pattern == "one_point" else weights(pattern, m, wr)
            cases.append(Case(f"{n}_{m}_blur{blur}_sc{scaling}_{pattern}", x, y, a, b, blur, scaling))
    for c in cases:
        for arr in (c.x, c.y, c.a, c.b):
            if arr is not None:
                arr.setflags(write=False)
    return tuple(cases)


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)


def dense(w, k):
    """A side's weights as float64 numbers: the values given (the cases' are float32), or 1/k."""
    return np.full(k, 1.0 / k) if w is None else np.asarray(w, np.float64)


# ------------------------------------------------------------------------------------------ float64, dense, log domain
def _cost_t(P, Q):
    """C transposed, [S, R]: the cloud summed over comes first, so that the sums below run over it in its order."""
    return ((Q[:, None, :] - P[None, :, :]) ** 2).sum(-1) / 2


def _softmin(eps, Ct, h):
    """-eps log sum_j exp(h_j - C_ij / eps), summed over j one point after the other (numpy reduces an outer axis row by row)."""
    with np.errstate(divide="ignore"):
        v = h[:, None] - Ct / eps
        mx = v.max(axis=0)
        return -eps * (mx + np.log(np.add.reduce(np.exp(v - mx[None, :]), axis=0)))


def _schedule(x, y, blur, scaling, diameter):
    if diameter is None:
        diameter = sc.bbox_diameter(x, y)
    d = float(F32(diameter))
    return d, [d ** 2] + [float(np.exp(e)) for e in np.arange(2 * np.log(d), 2 * np.log(blur), 2 * np.log(scaling))] + [blur ** 2]


def float64_potentials(x, y, a, b, blur, scaling, diameter):
    """The weighted schedule up to the input of the last extrapolation: (eps list, la, lb, (a_x, b_y, a_y, b_x), transposed costs)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d, eps_s = _schedule(x, y, blur, scaling, diameter)
    with np.errstate(divide="ignore"):
        la, lb = np.log(dense(a, x.shape[0])), np.log(dense(b, y.shape[0]))
    Ct = dict(xx=_cost_t(x, x), yy=_cost_t(y, y), yx=_cost_t(y, x), xy=_cost_t(x, y))     # key "pq": rows p, summed over q
    eps = eps_s[0]
    a_x, b_y = _softmin(eps, Ct["xx"], la), _softmin(eps, Ct["yy"], lb)
    a_y, b_x = _softmin(eps, Ct["yx"], la), _softmin(eps, Ct["xy"], lb)
    for eps in eps_s:
        at_x, bt_y = _softmin(eps, Ct["xx"], la + a_x / eps), _softmin(eps, Ct["yy"], lb + b_y / eps)
        at_y, bt_x = _softmin(eps, Ct["yx"], la + b_x / eps), _softmin(eps, Ct["xy"], lb + a_y / eps)
        a_x, b_y = 0.5 * (a_x + at_x), 0.5 * (b_y + bt_y)
        a_y, b_x = 0.5 * (a_y + at_y), 0.5 * (b_x + bt_x)
    return eps_s, la, lb, (a_x, b_y, a_y, b_x), Ct


def float64_reference(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter=None):
    """(S, dS/dx, dS/dy) in float64.  S = sum_i a_i (b_x - a_x)_i + sum_j b_j (a_y - b_y)_j after the last extrapolation; the gradient
    is that extrapolation's, with the potentials and the right-hand cloud of every cost detached:
    dS/dx_i = a_i (T_xx(x_i) - T_xy(x_i)), dS/dy_j = b_j (T_yy(y_j) - T_yx(y_j)), T the softmax barycentres.  The weighted sums of
    S run in index order as well."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if _schedule(x, y, blur, scaling, diameter)[0] == 0.0:
        return 0.0, np.zeros(x.shape), np.zeros(y.shape)
    eps_s, la, lb, (a_x, b_y, a_y, b_x), Ct = float64_potentials(x, y, a, b, blur, scaling, diameter)
    eps = eps_s[-1]
    wa, wb = dense(a, x.shape[0]), dense(b, y.shape[0])

    def last(key, l, f, Q):
        """The last extrapolation over Q and its rows' barycentres: softmax weights [S, R] summed over Q point after point."""
        h = l + f / eps
        out = _softmin(eps, Ct[key], h)
        with np.errstate(divide="ignore"):
            p = np.exp(h[:, None] - Ct[key] / eps + out[None, :] / eps)
        return out, np.add.reduce(p[:, :, None] * Q[:, None, :], axis=0) / np.add.reduce(p, axis=0)[:, None]

    fa_x, T_xx = last("xx", la, a_x, x)
    fb_y, T_yy = last("yy", lb, b_y, y)
    fa_y, T_yx = last("yx", la, b_x, x)
    fb_x, T_xy = last("xy", lb, a_y, y)
    S = float(np.cumsum(wa * (fb_x - fa_x))[-1]) + float(np.cumsum(wb * (fa_y - fb_y))[-1])
    return S, wa[:, None] * (T_xx - T_xy), wb[:, None] * (T_yy - T_yx)


def autograd_gradient(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter=None):
    """(S, dS/dx, dS/dy) with the last extrapolation differentiated by torch autograd (C_xy = cost(x, y.detach()) and so on),
    from float64_potentials' potentials: what float64_reference states in closed form."""
    import torch
    eps_s, la, lb, pots, _ = float64_potentials(x, y, a, b, blur, scaling, diameter)
    t = lambda v: torch.as_tensor(np.asarray(v, np.float64))
    X, Y, la, lb = t(x), t(y), t(la), t(lb)
    a_x, b_y, a_y, b_x = (t(p) for p in pots)
    wa, wb = t(dense(a, X.shape[0])), t(dense(b, Y.shape[0]))
    xg, yg = X.clone().requires_grad_(), Y.clone().requires_grad_()
    eps = eps_s[-1]
    cost = lambda p, q: ((p[:, None, :] - q[None, :, :]) ** 2).sum(-1) / 2
    softmin = lambda C, h: -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)
    fa_x, fb_y = softmin(cost(xg, X), la + a_x / eps), softmin(cost(yg, Y), lb + b_y / eps)
    fa_y, fb_x = softmin(cost(yg, X), la + b_x / eps), softmin(cost(xg, Y), lb + a_y / eps)
    S = (wa * (fb_x - fa_x)).sum() + (wb * (fa_y - fb_y)).sum()
    dx, dy = torch.autograd.grad(S, (xg, yg))
    return float(S.detach()), dx.numpy(), dy.numpy()


@functools.lru_cache(maxsize=None)
def reference(name, given):
    """float64_reference of case `name` with the bounding-box diameter (given False) or DIAMETER_GIVEN.  Computed once, read-only."""
    c = BY_NAME[name]
    S, dx, dy = float64_reference(c.x, c.y, c.a, c.b, c.blur, c.scaling, c.diameter(given))
    for arr in (dx, dy):
        arr.setflags(write=False)
    return S, dx, dy


def expand(points, mult):
    """The cloud with point i repeated mult[i] times, and for every copy the index of its point."""
    idx = np.repeat(np.arange(len(mult)), mult)
    return np.ascontiguousarray(points[idx]), idx


def multiplicity_pair(seed=731, n=45, m=38):
    """Distinct points with integer multiplicities 1..4 on both sides: (x, y, kx, ky)."""
    rng = _rng(seed)
    x, y = _blob(rng, n, (0.45, 0.5, 0.5), 0.06), _blob(rng, m, (0.55, 0.5, 0.52), 0.05)
    return x, y, rng.integers(1, 5, n), rng.integers(1, 5, m)


# ------------------------------------------------------------------------------------------ batches
B4_SPREADS = (0.004, 0.3, 0.02, 0.1)                  # diameters 0.03 to 2: schedules of 2 to 8 entries share the batch


@functools.lru_cache(maxsize=None)
def batch(shared):
    """(X [4, 37, 3], Y [29, 3] or [4, 29, 3], A [4, 37], Bw [29] or [4, 29], w [4]): clouds of four spreads, Dirichlet weights with
    every fifth one zero, and the weights of the pairs' losses in the scalar that is differentiated."""
    rng = _rng(741 if shared else 742)
    n, m = 37, 29
    X = np.stack([_blob(rng, n, (0.5, 0.5, 0.5), sp) for sp in B4_SPREADS])
    Y = _blob(rng, m, (0.506, 0.5, 0.497), 0.004) if shared else np.stack([_blob(rng, m, (0.5 + 2 * sp, 0.5, 0.5 - sp), 0.8 * sp) for sp in B4_SPREADS])

    def w(k):
        v = rng.dirichlet(np.ones(k))
        v[4::5] = 0.0
        return (v / v.sum()).astype(F32)

    A = np.stack([w(n) for _ in B4_SPREADS])
    Bw = w(m) if shared else np.stack([w(m) for _ in B4_SPREADS])
    return X, Y, A, Bw, rng.uniform(0.2, 2.0, len(B4_SPREADS)).astype(F32)


# ------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
def f32_restatement(x, y, a=None, b=None, blur=0.05, scaling=0.5, diameter=None):
    """csrc/sinkhorn.hip's weighted path in numpy float32 -> dict(S, dx, dy, W), as sinkhorn_cases.f32_restatement states the uniform
    one: lw = log w in float32 per point (the scalar -log n for a None side), h_j = lw_j + f_j / eps, the two passes (max, then sum of
    exp), the 0.5 old + 0.5 new updates, the last extrapolation, S = sum a_i (b_x - a_x)_i + sum b_j (a_y - b_y)_j in float64
    (a None side: the mean), and the one-pass gradient weights w = exp(h_j - C_ij * hc + g_i / eps) with
    dS/dp_i = a_i (D_c / W_c - D_s / W_s), exactly 0 for a row of weight zero.  W: (min, max) of the row sums of the weights."""
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    n, m = x.shape[0], y.shape[0]
    d = float(F32(diameter)) if diameter is not None else sc.bbox_diameter(x, y)
    n_eps = sc.schedule_length(d, blur, scaling)

    def eps_of(it):
        if it <= 0:
            return d * d
        if it >= n_eps - 1:
            return float(blur) * float(blur)
        return float(np.exp(2.0 * np.log(d) + (it - 1) * 2.0 * np.log(float(scaling))))

    def sqdist(P, Q):
        df = P[:, None, :] - Q[None, :, :]
        return df, (df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]

    sq = {k: sqdist(*pq)[1] for k, pq in dict(xx=(x, x), yy=(y, y), yx=(y, x), xy=(x, y)).items()}
    with np.errstate(divide="ignore"):
        lwa = np.full(n, -np.log(F32(n)), F32) if a is None else np.log(np.asarray(a, F32))
        lwb = np.full(m, -np.log(F32(m)), F32) if b is None else np.log(np.asarray(b, F32))
    assert lwa.dtype == F32 and lwb.dtype == F32

    def softmin(key, f, lw, it, old=None):
        eps_d = eps_of(it)
        inv_eps, eps = F32(1.0 / eps_d), F32(eps_d)
        hc = F32(0.5) * inv_eps
        h = lw + (f * inv_eps if f is not None else F32(0.0))
        v = h[None, :] - sq[key] * hc
        mx = v.max(axis=1)
        s = np.exp(v - mx[:, None]).sum(axis=1, dtype=F32)
        new = -eps * (mx + np.log(s))
        return new if old is None else F32(0.5) * old + F32(0.5) * new

    o = [softmin("xx", None, lwa, 0), softmin("yy", None, lwb, 0), softmin("yx", None, lwa, 0), softmin("xy", None, lwb, 0)]
    for it in range(n_eps):
        o = [softmin("xx", o[0], lwa, it, o[0]), softmin("yy", o[1], lwb, it, o[1]),
             softmin("yx", o[3], lwa, it, o[2]), softmin("xy", o[2], lwb, it, o[3])]
    last = n_eps - 1
    q = [softmin("xx", o[0], lwa, last), softmin("yy", o[1], lwb, last), softmin("yx", o[3], lwa, last), softmin("xy", o[2], lwb, last)]
    assert all(p.dtype == F32 for p in o + q)
    tx, ty = q[3].astype(np.float64) - q[0].astype(np.float64), q[2].astype(np.float64) - q[1].astype(np.float64)
    S = float((tx / n).sum() if a is None else (np.asarray(a, F32).astype(np.float64) * tx).sum())
    S += float((ty / m).sum() if b is None else (np.asarray(b, F32).astype(np.float64) * ty).sum())

    inv_eps = F32(1.0 / eps_of(last))
    hc = F32(0.5) * inv_eps
    w_range = [np.inf, -np.inf]

    def bary(P, Q, f, lw, g):
        df, c = sqdist(P, Q)
        w = np.exp((lw + f * inv_eps)[None, :] - c * hc + (g * inv_eps)[:, None])
        W = w.sum(axis=1, dtype=F32)
        w_range[0], w_range[1] = min(w_range[0], float(W.min())), max(w_range[1], float(W.max()))
        return (w[..., None] * df).sum(axis=1, dtype=F32) / W[:, None]

    def rows(w, k, v):
        if w is None:
            return (F32(1.0) / F32(k)) * v
        w = np.asarray(w, F32)
        return np.where(w[:, None] > 0, w[:, None] * v, F32(0.0)).astype(F32)

    dx = rows(a, n, bary(x, y, o[2], lwb, q[3]) - bary(x, x, o[0], lwa, q[0]))
    dy = rows(b, m, bary(y, x, o[3], lwa, q[2]) - bary(y, y, o[1], lwb, q[1]))
    assert dx.dtype == F32 and dy.dtype == F32
    return dict(S=S, dx=dx, dy=dy, W=tuple(w_range), n_eps=n_eps)
