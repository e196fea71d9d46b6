"""Seeded recordings for the dataset statistics (csrc/dataset_stats.hip, gm_recording_stats) and the neighbour census
(gm_neighbour_census in csrc/graph.hip), with the references they are held to -- a plain helper module shared by
test_dataset_stats_cases.py (CPU), test_abi_dataset_stats.py (CPU) and test_gpu_dataset_stats.py (GPU).

Pure numpy (PCG64): a seed gives the same recording on every machine.

The references
  * ``recipe``: the reference's recipe restated (simulation/generate_metadata.py:24-45): np.diff over the frames, np.diff again,
    reshape to rows, np.mean and np.std (ddof = 0) -- in float64 on the float32-rounded recording.
  * ``fsum_moments``: the same quantities with exactly rounded sums: mean = fsum(x) / n, M2 = fsum((x - mean)^2), variance =
    M2 / n.  This is what the GPU is held to; the CPU tests hold the recipe to it within the recipe's own summation bound.

The kernel's launch shape, as this module assumes it (the GPU test asserts it through the header's constant and the workspace
query): at most MAX_WORKGROUPS workgroups of THREADS threads, one node per thread and grid pass.
"""
import functools
import math
from dataclasses import dataclass

import numpy as np

F32 = np.float32
THREADS, MAX_WORKGROUPS, RECORD_DOUBLES = 256, 1024, 24
ONE_PASS = THREADS * MAX_WORKGROUPS              # nodes of one pass of the grid
N_PAST_ONE_PASS = ONE_PASS + 77                  # every thread of the first 77 takes a second node

T_SIZES = (3, 4, 9)
N_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)
MERGE_SIZES = ((3, 65), (4, 257), (9, 1000))     # three recordings of different (T, N), merged by Chan's formula
FIXTURE_KINDS = ("jitter", "drift", "scales")    # tests/golden/dataset_stats_metadata.json: the reference's own script on these
FIXTURE_SIZES = ((9, 65), (9, 257), (9, 1000))   # ... as three files of one T (the script takes one --timesteps)
D = 8                                            # columns of a recording: [id, material, x, y, z, cx, cy, cz] (scene.make_scene)
MAT_COL = 1
U = 2.0 ** -53


def _rng(*seed):
    return np.random.Generator(np.random.PCG64(list(seed)))


@dataclass(frozen=True)
class Kind:
    """How a case's recordings are drawn and read: the columns (cart0, dim), the filter, and per axis the drift and the jitter of
    the velocities."""
    name: str
    seed: int
    cart0: int = 2
    dim: int = 3
    drift: tuple = (0.0, 0.0, 0.0)
    jitter: tuple = (1e-3, 1e-3, 1e-3)
    material: float = None         # the value of column MAT_COL the filter keeps; None: every row
    block: bool = False            # the last tenth of the rows (at least one) is a rigid block moving as one beside still sand


KINDS = {k.name: k for k in (
    Kind("jitter", 1),
    Kind("drift", 2, drift=(1.0e-2, -2.0e-2, 3.0e-2), jitter=(1e-5, 2e-5, 3e-5)),            # mean / std about 1e3
    Kind("block_all", 3, block=True),
    Kind("block_sand", 3, block=True, material=0.0),
    Kind("block_rigid", 3, block=True, material=1.0),
    Kind("scales", 4, jitter=(1e-6, 1e-2, 1e1)),
    Kind("dim1", 5, dim=1),
    Kind("dim2", 6, dim=2),
    Kind("first_column", 7, cart0=0),
    Kind("last_column", 8, cart0=D - 3),
    Kind("last_column_dim1", 9, cart0=D - 1, dim=1),
)}


@functools.lru_cache(maxsize=None)
def recording(kind_name, t, n):
    """float32 [t, n, D], read-only.  Columns outside the positions hold an id, the material and noise (so that a wrong column
    shows); the positions start in [0.3, 0.6) and move by drift + jitter * N(0, 1) per frame."""
    k = KINDS[kind_name]
    rng = _rng(k.seed, t, n)
    rec = rng.random((t, n, D)) + 2.0                       # what a wrong column would read
    rec[:, :, 0] = np.arange(n)
    rec[:, :, MAT_COL] = 0.0
    vel = np.asarray(k.drift[:k.dim]) + np.asarray(k.jitter[:k.dim]) * rng.standard_normal((t - 1, n, k.dim))
    if k.block:
        rigid = max(n // 10, 1)
        rec[:, n - rigid:, MAT_COL] = 1.0
        vel[:, :n - rigid] = 1e-6 * rng.standard_normal((t - 1, n - rigid, k.dim))      # settled sand
        vel[:, n - rigid:] = np.asarray([1e-2, -5e-3, 2e-3][:k.dim])                     # the block: one velocity for all its rows
    p0 = 0.3 + 0.3 * rng.random((1, n, k.dim))
    rec[:, :, k.cart0:k.cart0 + k.dim] = np.concatenate((p0, p0 + np.cumsum(vel, axis=0)))
    out = rec.astype(F32)
    out.setflags(write=False)
    return out


def selected_rows(kind_name, rec):
    k = KINDS[kind_name]
    return np.ones(rec.shape[1], bool) if k.material is None else rec[0, :, MAT_COL] == F32(k.material)


def samples(rec, cart0, dim, rows=None):
    """(velocities [., dim], accelerations [., dim]) in float64, as the recipe stacks them; rows: a mask over the nodes."""
    data = np.asarray(rec, np.float64)[:, :, cart0:cart0 + dim]
    if rows is not None:
        data = data[:, rows]
    vel = np.diff(data, n=1, axis=0)
    acc = np.diff(vel, n=1, axis=0)
    return vel.reshape(-1, dim), acc.reshape(-1, dim)


def recipe(recs, cart0, dim, rows=None):
    """generate_metadata.py:24-45 over a list of recordings (rows: one mask per recording, or None)."""
    parts = [samples(r, cart0, dim, None if rows is None else rows[i]) for i, r in enumerate(recs)]
    vel = np.concatenate([p[0] for p in parts], axis=0)
    acc = np.concatenate([p[1] for p in parts], axis=0)
    # *_var: np.var, the number np.std takes the root of
    return dict(vel_mean=np.mean(vel, axis=0), vel_std=np.std(vel, axis=0), acc_mean=np.mean(acc, axis=0), acc_std=np.std(acc, axis=0),
                vel_var=np.var(vel, axis=0), acc_var=np.var(acc, axis=0))


def fsum_of(x):
    """(count, mean, M2, mean |x|) per column of x [., dim] with exactly rounded sums."""
    n = x.shape[0]
    mean = np.asarray([math.fsum(x[:, a].tolist()) / n for a in range(x.shape[1])]) if n else np.zeros(x.shape[1])
    m2 = np.asarray([math.fsum(((x[:, a] - mean[a]) ** 2).tolist()) for a in range(x.shape[1])])
    mabs = np.asarray([math.fsum(np.abs(x[:, a]).tolist()) / n for a in range(x.shape[1])]) if n else np.zeros(x.shape[1])
    return n, mean, m2, mabs


def fsum_moments(recs, cart0, dim, rows=None):
    """The exactly summed form over a list of recordings: per quantity (count, mean, M2, mean |x|), the standard deviations, and
    the positions' range over the counted rows."""
    parts = [samples(r, cart0, dim, None if rows is None else rows[i]) for i, r in enumerate(recs)]
    vel = fsum_of(np.concatenate([p[0] for p in parts], axis=0))
    acc = fsum_of(np.concatenate([p[1] for p in parts], axis=0))
    pos = [np.asarray(r)[:, :, cart0:cart0 + dim][:, slice(None) if rows is None else rows[i]].reshape(-1, dim) for i, r in enumerate(recs)]
    pos = np.concatenate(pos, axis=0)
    rng_ = np.stack((pos.min(axis=0), pos.max(axis=0)), axis=1) if pos.shape[0] else None
    return dict(vel=vel, acc=acc, vel_std=np.sqrt(vel[2] / max(vel[0], 1)), acc_std=np.sqrt(acc[2] / max(acc[0], 1)), position_range=rng_)


@functools.lru_cache(maxsize=None)
def reference(kind_name, t, n):
    """fsum_moments of one recording of a kind, over the rows its filter keeps."""
    k = KINDS[kind_name]
    rec = recording(kind_name, t, n)
    rows = None if k.material is None else [selected_rows(kind_name, rec)]
    return fsum_moments([rec], k.cart0, k.dim, rows)


def one_pass_m2(x):
    """The scheme the kernel must NOT use: sum of squares minus n * mean^2, in float64."""
    n = x.shape[0]
    mean = x.sum(axis=0) / n
    return (x * x).sum(axis=0) - n * mean * mean


def chan(a, b):
    """(n, mean, M2) of two samples' union (Chan, Golub, LeVeque), float64."""
    (na, ma, m2a), (nb, mb, m2b) = a, b
    n = na + nb
    d = mb - ma
    return n, ma + d * (nb / n), m2a + m2b + d * d * (na * nb / n)


def summation_bound(n, mabs):
    """Worst case of a recursive float64 sum of n terms, divided by n: n * u * mean|x|, doubled for the division and the terms'
    own rounding -- the error numpy's mean may have, whichever order it sums in."""
    return 2.0 * n * U * mabs


# ------------------------------------------------------------------------------------------ the census past the cap
CLUMP_R = 0.015
CLUMP_MARGIN = 1e-6


@functools.lru_cache(maxsize=None)
def clump(n=600, rows=200, seed=77):
    """float32 [n, 3]: a cloud of n - rows points and `rows` distinct points inside a ball of diameter 0.9 r (each sees all the
    others of the clump: counts > 160), redrawn until no pair of the whole set lies within CLUMP_MARGIN (relative, in d2) of
    r * r -- the predicate then has one answer whatever the rounding."""
    for attempt in range(64):
        rng = _rng(seed, attempt)
        p = 0.3 + 0.12 * rng.random((n, 3))
        d = rng.standard_normal((rows, 3))
        d *= (0.45 * CLUMP_R * rng.random((rows, 1)) ** (1.0 / 3.0)) / np.linalg.norm(d, axis=1, keepdims=True)
        p[100:100 + rows] = p[7] + d
        p = p.astype(F32)
        if clump_margin(p) > CLUMP_MARGIN and np.unique(p, axis=0).shape[0] == n:
            p.setflags(write=False)
            return p
    raise AssertionError("no clump with the margin")


def sq_dists(q, p):
    """float64 squared distances accumulated x -> y -> z, separate multiply and add: the header's arithmetic."""
    q, p = np.asarray(q, np.float64), np.asarray(p, np.float64)
    d2 = np.zeros((q.shape[0], p.shape[0]))
    for j in range(3):
        t = q[:, j:j + 1] - p[None, :, j]
        d2 = d2 + t * t
    return d2


def clump_margin(p, r=CLUMP_R):
    return float(np.abs(sq_dists(p, p) / (r * r) - 1.0).min())


def brute_counts(p, r):
    return (sq_dists(p, p) <= float(r) * float(r)).sum(axis=1)


def clump_recording(frames=4):
    """[frames, n, D] whose frame t is the clump pulled apart by the factor 1 + t about its centre (frame 0: the clump itself, later
    frames ever sparser), positions in columns 2..4."""
    p = clump().astype(np.float64)
    c = p[100:300].mean(axis=0)
    rec = np.zeros((frames, p.shape[0], D), F32)
    for t in range(frames):
        rec[t, :, 2:5] = (c + (p - c) * (1.0 + t)).astype(F32)
    rec[0, :, 2:5] = clump()
    return rec
