"""Seeded point-cloud pairs and batches for the Sinkhorn kernels (csrc/sinkhorn.hip) away from the one make the other Sinkhorn tests
use (a Gaussian blob near 0.5, blur .05, scaling .5, a few hundred points) -- a plain helper module shared by test_sinkhorn_cases.py
(CPU) and test_gpu_sinkhorn_cases.py (GPU).

A case is (x, y, blur, scaling, diameter) plus `want`, the regime it was built for; regime() measures the same quantities on the
arrays: n_eps (2 + the numpy.arange length, as in the oracle), A = d^2 / (2 blur^2) -- the size each of the three terms of the
gradient kernel's exponent h - C / eps + g / eps reaches before they cancel --, and where the sizes sit against the kernels' tiling
(4 rows per wave, 16 per workgroup, 64 lanes over the other cloud).

f32_restatement() is the kernels' arithmetic in numpy float32: what float32 alone does to a case, without __expf, fused
multiply-adds or the device's summation order.  test_sinkhorn_cases.py holds it to the GPU bars for every case, so that a GPU miss
is the kernel's and not the case's.

Pure numpy (PCG64): a seed gives the same case on every machine; only the float64 gradient reference (sinkhorn_grad_ref) uses torch."""
import functools
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
SK_RB, SK_WG_ROWS, SK_LANES = 4, 16, 64      # rows per wave, rows per workgroup, lanes striding the other cloud (csrc/sinkhorn.hip)
FWD_REL, GRAD_REL = 1e-5, 1e-4               # the project's bars: |S - ref| <= 1e-5 |ref|; |dS - ref| <= 1e-4 max |ref| per element

# The noise-level case ("shortest_coincident": blur >= diameter, y = x moved by 1e-4): S = 1.1e-10 is the mean of differences of
# potentials -eps (max + log sum) whose bracket is ~log n = 5.7 at eps = blur^2 = 0.25, each rounded to 2^-24 * 1.4 = 8.5e-8; the mean
# over 300 + 300 such roundings is ~3e-9 whatever the arithmetic.  The gradient is (1/n) times the difference of two barycentres that
# agree to 1e-4 of their size: 4.5e-8 at most.  The relative bars mean nothing there; the case's bars are absolute floors, each 4 times
# the float32 restatement's own error measured on the CPU (the device sums in another order and uses __expf):
#   forward:  measured |S_f32 - S_f64| = 2.89e-9                       -> floor 1.2e-8
#   gradient: measured max |d_f32 - d_f64| = 3.5e-10 (dx), 4.0e-10 (dy) -> floor 1.6e-9  (3.6 % of max |ref|; one barycentre is 1e-3)
# test_sinkhorn_cases.py holds the restatement to half of each floor (the measured quarter moves with the last bit of the host's exp).
NOISE_MARGIN = 4
NOISE_FWD_F32_ERR, NOISE_GRAD_F32_ERR = 3.0e-9, 4.0e-10
NOISE_FWD_FLOOR, NOISE_GRAD_FLOOR = NOISE_MARGIN * NOISE_FWD_F32_ERR, NOISE_MARGIN * NOISE_GRAD_F32_ERR


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def bbox_diameter(x, y):
    """The plan kernel's diameter: the float32 bounding box of both clouds, squares summed in float32 in axis order."""
    both = np.concatenate((np.asarray(x, F32).reshape(-1, 3), np.asarray(y, F32).reshape(-1, 3)))
    return float(np.sqrt(((both.max(0) - both.min(0)).astype(F32) ** 2).sum(dtype=F32)))


def schedule_length(diameter, blur, scaling):
    """n_eps as the oracle builds it: [d^2] + exp(arange(2 log d, 2 log blur, 2 log scaling)) + [blur^2]."""
    d = float(F32(diameter))
    return 2 + len(np.arange(2 * np.log(d), 2 * np.log(blur), 2 * np.log(scaling)))


@dataclass(frozen=True)
class Case:
    name: str
    x: np.ndarray
    y: np.ndarray
    blur: float = 0.05
    scaling: float = 0.5
    diameter: float = None          # None: the bounding box (the default path)
    want: dict = field(default_factory=dict)
    noise: bool = False             # the forward bar is the absolute floor

    @property
    def d(self):
        return float(F32(self.diameter)) if self.diameter is not None else bbox_diameter(self.x, self.y)


def regime(c):
    n, m = c.x.shape[0], c.y.shape[0]
    return dict(n_eps=schedule_length(c.d, c.blur, c.scaling), A=c.d ** 2 / (2 * c.blur ** 2), n=n, m=m,
                n_mod_4=n % SK_RB, n_mod_16=n % SK_WG_ROWS, m_mod_64=m % SK_LANES, m_mod_4=m % SK_RB, n_mod_64=n % SK_LANES)


def _blob(rng, n, centre, spread):
    return (np.asarray(centre, np.float64) + spread * rng.standard_normal((n, 3))).astype(F32)


def _box(rng, n, lo, side):
    return (np.asarray(lo, np.float64) + side * rng.random((n, 3))).astype(F32)


def _pin_corners(x, lo, side):
    """Two rows on opposite corners of the box: the union's diameter is side * sqrt(3) whatever the seed."""
    x[0] = np.asarray(lo, np.float64)
    x[1] = np.asarray(lo, np.float64) + side
    return x


# ------------------------------------------------------------------------------------------ single pairs
def _schedule_pair(seed, n=300, m=260, side=0.55 / np.sqrt(3.0)):
    rng = _rng(seed)
    x = _pin_corners(_box(rng, n, (0.3, 0.3, 0.3), side), (0.3, 0.3, 0.3), side)
    y = _box(rng, m, (0.3 + 0.1 * side, 0.3, 0.3), 0.8 * side)
    return x, y


def _build_cases():
    cases = []

    def add(name, x, y, **kw):
        cases.append(Case(name, np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32), **kw))

    # -- schedules: diameter 0.55 (two rows pinned on the box's corners) unless said otherwise
    x, y = _schedule_pair(101)
    add("scaling_0.9", x, y, scaling=0.9, want=dict(n_eps=25))
    x, y = _schedule_pair(102)
    add("scaling_0.2", x, y, scaling=0.2, want=dict(n_eps=4))
    x, y = _schedule_pair(103)
    add("scaling_0.1", x, y, scaling=0.1, want=dict(n_eps=4))
    x, y = _schedule_pair(104, side=0.35 / np.sqrt(3.0))     # diameter 0.35 (0.44 with the shifted copy) <= blur 0.5: the list [d^2, blur^2]
    add("shortest_shifted", x, x[:260] + np.array([0.06, -0.04, 0.05], F32), blur=0.5, want=dict(n_eps=2, A_max=0.5))
    rng = _rng(105)
    add("shortest_coincident", x, (x.astype(np.float64) + 1e-4 * rng.standard_normal(x.shape)).astype(F32), blur=0.5,
        want=dict(n_eps=2, A_max=0.5), noise=True)
    x, y = _schedule_pair(106, side=0.6 / np.sqrt(3.0))
    add("blur_0.01", x, y, blur=0.01, want=dict(n_eps=8, A_min=1.7e3))
    x, y = _schedule_pair(107, side=0.6 / np.sqrt(3.0))
    add("blur_0.003", x, y, blur=0.003, want=dict(n_eps=10, A_min=1.9e4))

    # -- sizes against the tiling: single points, the row tail of a wave, the lane tail of a sweep, one workgroup and two
    for k, (n, m, want) in enumerate([
            (1, 300, dict(n=1, n_mod_4=1)), (300, 1, dict(m=1)), (2, 65, dict(n_mod_4=2, m_mod_64=1)), (65, 2, dict(n_mod_4=1, n_mod_64=1)),
            (5, 64, dict(n_mod_4=1, m_mod_64=0)), (17, 63, dict(n_mod_16=1, n_mod_4=1, m_mod_64=63)), (16, 129, dict(n_mod_16=0, m_mod_64=1))]):
        rng = _rng(200 + k)
        add(f"size_{n}_{m}", _blob(rng, n, (0.45, 0.5, 0.5), 0.06), _blob(rng, m, (0.55, 0.5, 0.52), 0.05), want={**dict(n=n, m=m), **want})
    rng = _rng(210)
    add("size_4_4", _blob(rng, 4, (0.4, 0.5, 0.5), 0.1), _blob(rng, 4, (0.6, 0.5, 0.5), 0.1), want=dict(n=4, m=4, n_mod_4=0, distinct=True))

    # -- geometry
    rng = _rng(301)
    far = np.array([2.8, 0.0, 0.0]) @ _rotation(rng)
    xb, yb = _blob(rng, 230, (0.1, 0.2, 0.3), 0.02), _blob(rng, 190, np.array([0.1, 0.2, 0.3]) + far, 0.02)
    add("far_blobs_blur_0.05", xb, yb, want=dict(A_min=1.5e3, centre_distance=2.8))
    add("far_blobs_blur_0.01", xb, yb, blur=0.01, want=dict(A_min=3.9e4, centre_distance=2.8))
    rng = _rng(302)
    add("offset_1000", _blob(rng, 210, (1000.45, 1000.5, 1000.5), 0.05), _blob(rng, 170, (1000.52, 1000.5, 1000.55), 0.06),
        want=dict(min_coordinate=999.0))
    rng = _rng(303)
    add("duplicates", np.repeat(_blob(rng, 20, (0.5, 0.5, 0.5), 0.08), 10, axis=0), _blob(rng, 150, (0.53, 0.5, 0.5), 0.07),
        want=dict(distinct_x=20, n=200))
    rng = _rng(304)
    xs = _blob(rng, 300, (0.5, 0.5, 0.5), 0.07)
    add("subset", xs, xs[:117].copy(), want=dict(m=117, subset=True))
    rng = _rng(305)
    u = np.array([1.0, 2.0, -1.5]) / np.linalg.norm([1.0, 2.0, -1.5])
    add("collinear", (np.array([0.5, 0.4, 0.6]) + 0.3 * rng.random((181, 1)) * u).astype(F32),
        (np.array([0.5, 0.4, 0.6]) + (0.05 + 0.3 * rng.random((149, 1))) * u).astype(F32), want=dict(collinear=True))
    rng = _rng(306)
    add("two_clusters", np.concatenate((_blob(rng, 120, (0.2, 0.5, 0.5), 0.03), _blob(rng, 135, (0.8, 0.5, 0.5), 0.03))),
        _blob(rng, 201, (0.5, 0.5, 0.5), 0.03), want=dict(between=True))
    return tuple(cases)


def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


CASES = _build_cases()
BY_NAME = {c.name: c for c in CASES}
NAMES = tuple(BY_NAME)
DIAMETER_CASES = ("scaling_0.9", "scaling_0.2", "scaling_0.1", "shortest_shifted")     # run through the `diameter=` keyword as well
SINGLE_POINT = ("size_1_300", "size_300_1")
PERMUTED = ("scaling_0.9", "size_17_63", "far_blobs_blur_0.01", "duplicates")
BLUR_SCALING = tuple(sorted({(c.blur, c.scaling) for c in CASES}))


def self_cloud():
    """The cloud of the loss(x, x) tests and its shifted copy (which gives the scale of a gradient of this cloud)."""
    x, _ = _schedule_pair(401, n=257, side=0.6 / np.sqrt(3.0))
    return x, (x + F32(0.03)).astype(F32)


def check_case(c):
    """Every entry of c.want against what regime() and the arrays say."""
    r = regime(c)
    assert c.x.dtype == F32 and c.y.dtype == F32 and c.x.shape == (r["n"], 3) and c.y.shape == (r["m"], 3), c.name
    assert max(r["n"], r["m"]) <= 600 and np.isfinite(c.x).all() and np.isfinite(c.y).all(), c.name
    for key, val in c.want.items():
        if key in r:
            assert r[key] == val, (c.name, key, r[key], val)
        elif key == "A_min":
            assert r["A"] >= val, (c.name, r["A"])
        elif key == "A_max":
            assert r["A"] <= val and c.blur >= c.d, (c.name, r["A"], c.d)
        elif key == "distinct":
            assert len(np.unique(np.concatenate((c.x, c.y)), axis=0)) == r["n"] + r["m"], c.name
        elif key == "centre_distance":
            dist = np.linalg.norm(c.x.mean(0, dtype=np.float64) - c.y.mean(0, dtype=np.float64))
            assert abs(dist - val) < 0.01 and max(c.x.std(0).max(), c.y.std(0).max()) < 0.025, (c.name, dist)
        elif key == "min_coordinate":
            assert min(c.x.min(), c.y.min()) >= val and c.d < 1.0, c.name
        elif key == "distinct_x":
            rows, counts = np.unique(c.x, axis=0, return_counts=True)
            assert len(rows) == val and (counts == r["n"] // val).all(), c.name
        elif key == "subset":
            assert np.array_equal(c.y, c.x[:r["m"]]) and r["m"] < r["n"], c.name
        elif key == "collinear":
            both = np.concatenate((c.x, c.y)).astype(np.float64)
            sv = np.linalg.svd(both - both.mean(0), compute_uv=False)
            assert sv[1] <= 1e-6 * sv[0], (c.name, sv)      # float32 rounding of the coordinates only
        elif key == "between":
            left, right = c.x[c.x[:, 0] < 0.5], c.x[c.x[:, 0] >= 0.5]
            assert len(left) >= 100 and len(right) >= 100 and left[:, 0].max() < c.y[:, 0].min() and c.y[:, 0].max() < right[:, 0].min(), c.name
        else:
            raise AssertionError((c.name, key))
    return r


# ------------------------------------------------------------------------------------------ batches
@dataclass(frozen=True)
class Batch:
    name: str
    X: np.ndarray          # [B, n, 3]
    Y: np.ndarray          # [m, 3] (shared), or [B, m, 3]
    w: np.ndarray          # [B] weights of the pairs' losses in the scalar that is differentiated
    blur: float = 0.05
    scaling: float = 0.5

    @property
    def shared(self):
        return self.Y.ndim == 2

    def pair(self, b):
        return Case(f"{self.name}[{b}]", self.X[b], self.Y if self.shared else self.Y[b], self.blur, self.scaling)


B6_SPREADS = (0.004, 0.3, 0.02, 1.0, 0.1, 0.05)      # the diameters of the pairs: 0.03 (n_eps 2) ... 7 (n_eps 10)


@functools.lru_cache(maxsize=None)
def batches():
    out = {}
    rng = _rng(501)
    n, m = 130, 97
    X = np.stack([_blob(rng, n, (0.5, 0.5, 0.5), sp) for sp in B6_SPREADS])
    Y = np.stack([_blob(rng, m, (0.5 + 2 * sp, 0.5, 0.5 - sp), 0.8 * sp) for sp in B6_SPREADS])
    w6 = rng.uniform(0.2, 2.0, len(B6_SPREADS)).astype(F32)
    out["b6_per_pair_y"] = Batch("b6_per_pair_y", X, Y, w6)
    out["b6_shared_y"] = Batch("b6_shared_y", X, _blob(rng, m, (0.506, 0.5, 0.497), 0.004), w6)
    rng = _rng(502)
    out["b1"] = Batch("b1", _blob(rng, 150, (0.5, 0.5, 0.5), 0.05)[None], _blob(rng, 131, (0.52, 0.5, 0.5), 0.06)[None], np.ones(1, F32))
    rng = _rng(503)
    spreads = rng.uniform(0.01, 0.4, 70)
    X = np.stack([_blob(rng, 40, 0.5 + 0.1 * rng.standard_normal(3), sp) for sp in spreads])
    out["b70_shared_y"] = Batch("b70_shared_y", X, _blob(rng, 33, (0.52, 0.5, 0.5), 0.05), rng.uniform(0.2, 2.0, 70).astype(F32))
    return out


# ------------------------------------------------------------------------------------------ the kernels' arithmetic in float32
def f32_restatement(x, y, blur=0.05, scaling=0.5, diameter=None):
    """csrc/sinkhorn.hip in numpy float32 -> dict(S, dx, dy, W): the schedule in float64 as sk_eps forms it, then per softmin the
    two passes (max, then sum of exp) over h_j - |p_i - q_j|^2 * (0.5 / eps) with the differences taken before squaring, the
    0.5 old + 0.5 new updates, the last extrapolation, the means in float64 (sinkhorn_cost_kernel), and the one-pass gradient
    weights w = exp(h_j - C_ij * hc + g_i / eps) with dS/dp_i = (1/R) (D_c / W_c - D_s / W_s).  W: (min, max) of the row sums of
    the weights, which the one-pass form relies on being near 1."""
    x, y = np.ascontiguousarray(x, F32), np.ascontiguousarray(y, F32)
    n, m = x.shape[0], y.shape[0]
    d = float(F32(diameter)) if diameter is not None else bbox_diameter(x, y)
    if d == 0.0:
        return dict(S=0.0, dx=np.zeros_like(x), dy=np.zeros_like(y), W=(1.0, 1.0))
    n_eps = schedule_length(d, blur, scaling)

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
    logwa, logwb = -np.log(F32(n)), -np.log(F32(m))

    def softmin(key, f, logw, it, old=None):
        eps_d = eps_of(it)
        inv_eps, eps = F32(1.0 / eps_d), F32(eps_d)
        hc = F32(0.5) * inv_eps
        h = logw + (f * inv_eps if f is not None else F32(0.0))
        v = h[None, :] - sq[key] * hc if f is not None else h - sq[key] * hc
        mx = v.max(axis=1)
        s = np.exp(v - mx[:, None]).sum(axis=1, dtype=F32)
        new = -eps * (mx + np.log(s))
        return new if old is None else F32(0.5) * old + F32(0.5) * new

    o = [softmin("xx", None, logwa, 0), softmin("yy", None, logwb, 0), softmin("yx", None, logwa, 0), softmin("xy", None, logwb, 0)]
    for it in range(n_eps):
        o = [softmin("xx", o[0], logwa, it, o[0]), softmin("yy", o[1], logwb, it, o[1]),
             softmin("yx", o[3], logwa, it, o[2]), softmin("xy", o[2], logwb, it, o[3])]
    last = n_eps - 1
    q = [softmin("xx", o[0], logwa, last), softmin("yy", o[1], logwb, last), softmin("yx", o[3], logwa, last), softmin("xy", o[2], logwb, last)]
    assert all(a.dtype == F32 for a in o + q)
    S = float(((q[3].astype(np.float64) - q[0].astype(np.float64)) / n).sum() + ((q[2].astype(np.float64) - q[1].astype(np.float64)) / m).sum())

    inv_eps = F32(1.0 / eps_of(last))
    hc = F32(0.5) * inv_eps
    w_range = [np.inf, -np.inf]

    def bary(P, Q, f, logw, g):
        df, c = sqdist(P, Q)
        w = np.exp((logw + f * inv_eps)[None, :] - c * hc + (g * inv_eps)[:, None])
        W = w.sum(axis=1, dtype=F32)
        w_range[0], w_range[1] = min(w_range[0], float(W.min())), max(w_range[1], float(W.max()))
        return (w[..., None] * df).sum(axis=1, dtype=F32) / W[:, None]

    dx = (F32(1.0) / F32(n)) * (bary(x, y, o[2], logwb, q[3]) - bary(x, x, o[0], logwa, q[0]))
    dy = (F32(1.0) / F32(m)) * (bary(y, x, o[3], logwa, q[2]) - bary(y, y, o[1], logwb, q[1]))
    assert dx.dtype == F32 and dy.dtype == F32
    return dict(S=S, dx=dx, dy=dy, W=tuple(w_range), n_eps=n_eps)


# ------------------------------------------------------------------------------------------ float64 references, computed once
def sinkhorn_grad_ref(x, y, blur=0.05, scaling=0.5, diameter=None):
    """(S, dS/dx, dS/dy) in float64: oracle.sinkhorn_divergence's schedule (oracle/epd_oracle.py, sinkhorn_divergence) run
    without autograd, then the last extrapolation at blur^2 differentiated with C_xx = cost(x, x.detach()),
    C_yy = cost(y, y.detach()), C_xy = cost(x, y.detach()), C_yx = cost(y, x.detach())."""
    import torch
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    y = torch.as_tensor(np.asarray(y), dtype=torch.float64)
    n, m = x.shape[0], y.shape[0]
    if diameter is None:   # as the oracle: the bounding box of both clouds in float32
        both = np.concatenate((x.numpy(), y.numpy())).astype(np.float32)
        diameter = float(np.sqrt(((both.max(0) - both.min(0)).astype(np.float32) ** 2).sum(dtype=np.float32)))
    diameter = float(np.float32(diameter))
    if diameter == 0.0:
        return 0.0, np.zeros(tuple(x.shape)), np.zeros(tuple(y.shape))
    eps_s = [diameter ** 2] + [float(np.exp(e)) for e in np.arange(2 * np.log(diameter), 2 * np.log(blur), 2 * np.log(scaling))] + [blur ** 2]

    def cost(a, b):
        return ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1) / 2

    def softmin(eps, C, h):
        return -eps * torch.logsumexp(h[None, :] - C / eps, dim=1)

    la = torch.full((n,), -np.log(n), dtype=torch.float64)
    lb = torch.full((m,), -np.log(m), dtype=torch.float64)
    with torch.no_grad():
        C_xx, C_yy, C_xy, C_yx = cost(x, x), cost(y, y), cost(x, y), cost(y, x)
        eps = eps_s[0]
        a_x, b_y = softmin(eps, C_xx, la), softmin(eps, C_yy, lb)
        a_y, b_x = softmin(eps, C_yx, la), softmin(eps, C_xy, lb)
        for eps in eps_s:
            at_x, bt_y = softmin(eps, C_xx, la + a_x / eps), softmin(eps, C_yy, lb + b_y / eps)
            at_y, bt_x = softmin(eps, C_yx, la + b_x / eps), softmin(eps, C_xy, lb + a_y / eps)
            a_x, b_y = 0.5 * (a_x + at_x), 0.5 * (b_y + bt_y)
            a_y, b_x = 0.5 * (a_y + at_y), 0.5 * (b_x + bt_x)
        del C_xx, C_yy, C_xy, C_yx
    xg, yg = x.clone().requires_grad_(), y.clone().requires_grad_()
    eps = blur ** 2
    fa_x = softmin(eps, cost(xg, x), la + a_x / eps)
    fb_y = softmin(eps, cost(yg, y), lb + b_y / eps)
    fa_y = softmin(eps, cost(yg, x), la + b_x / eps)
    fb_x = softmin(eps, cost(xg, y), lb + a_y / eps)
    S = (fb_x - fa_x).mean() + (fa_y - fb_y).mean()
    dx, dy = torch.autograd.grad(S, (xg, yg))
    return float(S.detach()), dx.numpy(), dy.numpy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(S, dS/dx, dS/dy) of case `name` in float64: oracle.sinkhorn_divergence and sinkhorn_grad_ref.  Computed once, read-only."""
    return pair_reference(BY_NAME[name])


def pair_reference(c):
    from oracle import epd_oracle as orc
    S = orc.sinkhorn_divergence(c.x, c.y, blur=c.blur, scaling=c.scaling, diameter=c.diameter)
    Sg, dx, dy = sinkhorn_grad_ref(c.x, c.y, blur=c.blur, scaling=c.scaling, diameter=c.diameter)
    assert abs(S - Sg) <= 1e-9 * abs(S) + 1e-15, (c.name, S, Sg)      # the two float64 restatements of one schedule
    for a in (dx, dy):
        a.setflags(write=False)
    return S, dx, dy


def forward_bar(c, S_ref):
    """|S - ref| of a case: 1e-5 relative; for the noise-level case the absolute floor."""
    return NOISE_FWD_FLOOR if c.noise else FWD_REL * abs(S_ref)


def grad_bar(c, ref):
    """max |dS - ref| of a case, per element: 1e-4 of max |ref|; for the noise-level case the absolute floor."""
    return NOISE_GRAD_FLOOR if c.noise else GRAD_REL * float(np.abs(ref).max())
