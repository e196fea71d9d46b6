"""Seeded inputs for the graph front end (csrc/graph.hip, csrc/blocks_dev.h, the table builder of csrc/hedge.hip) on ties and
degenerate geometry -- a plain helper module shared by test_graph_cases.py (CPU) and test_gpu_graph_edges.py (GPU).

Pure numpy (PCG64): a seed gives the same case on every machine.  Every generator returns what it built together with a dict of
the properties the case exists for, computed on what was actually built; the tests assert those properties (``GeoCase.check`` /
``DegreeCase.check``) before they touch the GPU, so no case can pass without entering its regime.

The thresholds named here are the kernels' own: NB_CAP (96 in-radius candidates: neighbor_fast_kernel hands the query to
neighbor_kernel), SEG_CAP (in-degree 96: segment_sort_kernel's long path), kCellOrderCap (1024 rows in a cell: cell_order_kernel
raises order_skip), 32-edge blocks and 128-edge groups (edge_blocks_plan / edge_blocks_fill).
"""
import functools
from dataclasses import dataclass, field

import numpy as np

F32 = np.float32
NB_CAP = 96
SEG_CAP = 96
CELL_ORDER_CAP = 1024
BLOCK, GROUP = 32, 128
R = 0.015          # the scenes' connectivity radius
S7 = 2.0 ** -7     # lattice spacing of the tie lattice: r / s = 1.92, so the shells at s, s*sqrt(2), s*sqrt(3) are inside, 2s is not


# ------------------------------------------------------------------------------------------ measuring a geometry case
def _sq_dists(q, p):
    """float64 squared distances accumulated x -> y -> z, separate multiply and add: the contract's arithmetic."""
    q = np.asarray(q, np.float64)
    p = np.asarray(p, np.float64)
    d2 = np.zeros((q.shape[0], p.shape[0]))
    for j in range(3):
        t = q[:, j:j + 1] - p[None, :, j]
        d2 = d2 + t * t
    return d2


def radius_regime(pos, r, cap, n_per=None):
    """What the radius search meets on `pos` (graphs of `n_per` rows apart): per query the number of in-radius candidates
    (itself included), whether the cap cuts a group of equal distances in two (the kept set is then decided by index alone),
    whether two of its first cap + 1 candidates are equally far, and how many pairs sit at d2 == r*r exactly."""
    pos = np.asarray(pos)
    n = pos.shape[0]
    n_per = n if not n_per else int(n_per)
    r2 = float(r) * float(r)
    count = np.zeros(n, np.int64)
    tie_at_cap = np.zeros(n, bool)
    tie_in_kept = np.zeros(n, bool)
    zero_rank_of_self = np.zeros(n, np.int64)
    at_radius = 0
    for g0 in range(0, n, n_per):
        p = pos[g0:g0 + n_per]
        for a in range(0, p.shape[0], 512):
            d2 = _sq_dists(p[a:a + 512], p)
            inside = d2 <= r2
            at_radius += int((d2 == r2).sum())
            count[g0 + a:g0 + a + d2.shape[0]] = inside.sum(axis=1)
            srt = np.sort(np.where(inside, d2, np.inf), axis=1)[:, :cap + 1]
            fin = np.isfinite(srt)
            eq = (srt[:, 1:] == srt[:, :-1]) & fin[:, 1:]
            tie_in_kept[g0 + a:g0 + a + d2.shape[0]] = eq.any(axis=1)
            if srt.shape[1] > cap:
                tie_at_cap[g0 + a:g0 + a + d2.shape[0]] = eq[:, cap - 1]
            rows = np.arange(d2.shape[0])
            zero_rank_of_self[g0 + a:g0 + a + d2.shape[0]] = ((d2 == 0.0) & (np.arange(p.shape[0])[None, :] < (a + rows)[:, None])).sum(axis=1)
    return dict(count=count, tie_at_cap=tie_at_cap, tie_in_kept=tie_in_kept, at_radius=at_radius,
                self_not_first=int((zero_rank_of_self > 0).sum()), self_cut=int((zero_rank_of_self >= cap).sum()))


def engine_grid(pos, r, n_per=None):
    """The cell grid the engine lays over `pos` -- grid_params of csrc/graph.hip restated: cell edge r * (1 + 2^-10), doubled in
    volume until the grid of ONE graph fits max(2n, 32768) / n_graphs cells.  Returns (dims, coarsening rounds, rows in the
    fullest cell)."""
    pos = np.asarray(pos, np.float64)
    n = pos.shape[0]
    n_per = n if not n_per else int(n_per)
    n_graphs = (n + n_per - 1) // n_per
    max_cells = max(min(max(2 * n, 32768), 1 << 22) // n_graphs, 1)
    lo, ext = pos.min(axis=0), pos.max(axis=0) - pos.min(axis=0)
    h, rounds = float(r) * (1.0 + 1.0 / 1024.0), 0
    while True:
        dims = np.minimum(np.floor(ext / h) + 1.0, 2.0e9)
        if dims.prod() <= max_cells:
            break
        h *= 1.2599210498948732
        rounds += 1
    dims = dims.astype(np.int64)
    cell = np.clip(np.floor((pos - lo) * (1.0 / h)).astype(np.int64), 0, dims - 1)
    key = ((np.arange(n) // n_per) * dims.prod() + (cell[:, 2] * dims[1] + cell[:, 1]) * dims[0] + cell[:, 0])
    return dims, rounds, int(np.bincount(key).max())


@dataclass
class GeoCase:
    name: str
    pos: np.ndarray                 # float32 [n, 3]
    r: float
    cap: int
    n_per: int = None               # rows per graph of a batch (None: one graph)
    expect: dict = field(default_factory=dict)   # property name -> predicate on its value
    props: dict = field(default_factory=dict)
    cells_ok: bool = True           # the oracle's own cell list (edge r * 1.001, never coarsened) is affordable on this extent

    def measure(self):
        reg = radius_regime(self.pos, self.r, self.cap, self.n_per)
        c = reg["count"]
        dims, rounds, fullest = engine_grid(self.pos, self.r, self.n_per)
        p64 = self.pos.astype(np.float64)
        self.props = dict(
            n=int(self.pos.shape[0]), min_in_radius=int(c.min()), max_in_radius=int(c.max()),
            cap_binds=int((c > self.cap).sum()), tie_at_cap=int(reg["tie_at_cap"].sum()), tie_in_kept=int(reg["tie_in_kept"].sum()),
            tie_free=not reg["tie_in_kept"].any(), at_radius=reg["at_radius"], self_not_first=reg["self_not_first"], self_cut=reg["self_cut"],
            fast_path=int((c <= NB_CAP).sum()), general_path=int((c > NB_CAP).sum()), over_160=int((c > 160).sum()),
            duplicates=int(self.pos.shape[0] - np.unique(self.pos, axis=0).shape[0]),
            dims=tuple(int(d) for d in dims), coarsening_rounds=rounds, fullest_cell=fullest,
            extent=tuple(float(e) for e in p64.max(axis=0) - p64.min(axis=0)), lo=float(p64.min()), hi=float(p64.max()))
        return self

    def check(self):
        """The case is in the regime it was built for."""
        assert self.pos.dtype == F32 and self.pos.ndim == 2 and self.pos.shape[1] == 3 and np.isfinite(self.pos).all(), self.name
        assert self.expect, self.name
        for key, pred in self.expect.items():
            assert pred(self.props[key]), (self.name, key, self.props[key])


def _case(name, pos, r=R, cap=20, n_per=None, cells_ok=True, **expect):
    return GeoCase(name, np.ascontiguousarray(pos, dtype=F32), float(r), int(cap), n_per, expect, cells_ok=cells_ok).measure()


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _pos(v):
    return lambda x: x > v


def _is(v):
    return lambda x: x == v


# ------------------------------------------------------------------------------------------ geometry generators
def lattice(m, spacing=S7, origin=0.25, seed=11):
    """m^3 lattice, rows in shuffled order (so the index that breaks a tie is unrelated to the position)."""
    k = np.arange(m, dtype=np.float64)
    g = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * spacing + origin
    p = g.astype(F32)
    assert np.array_equal(p.astype(np.float64), g)   # every coordinate is a float32: the lattice is exact
    return p[_rng(seed).permutation(p.shape[0])]


def cloud(n, side, seed, lo=0.3):
    return (lo + side * _rng(seed).random((n, 3))).astype(F32)


def side_for(n, mean_in_radius, r=R):
    return float((n * 4.0 / 3.0 * np.pi * r ** 3 / mean_in_radius) ** (1.0 / 3.0))


def with_cluster(base, rows, point):
    p = np.array(base, dtype=F32, copy=True)
    p[rows] = np.asarray(point, F32)
    return p


def _a1(m):
    interior = (m - 2) ** 3
    return _case(f"a1_lattice{m}", lattice(m), tie_free=_is(False), cap_binds=lambda v: v >= interior, tie_at_cap=lambda v: v >= interior,
                 min_in_radius=_is(8), max_in_radius=_is(27), n=_is(m ** 3))


def _a2(r, want):
    k = np.arange(-4, 5, dtype=np.float64)
    g = (np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * 2.0 ** -6).astype(F32)
    g = g[_rng(21).permutation(g.shape[0])]
    name = "a2_exactly_r" if want == 7 else "a2_just_below_r"
    return _case(name, g, r=r, max_in_radius=_is(want), at_radius=(_pos(0) if want == 7 else _is(0)), lo=lambda v: v < 0)


def _a3(size):
    base = cloud(1200, 0.1, 31)
    rows = np.arange(400, 400 + size)
    p = with_cluster(base, rows, base[17])
    if size > NB_CAP:   # ranking by index alone in the general kernel; the self edge is cut for all but the first 20 rows of the cluster
        return _case(f"a3_cluster{size}", p, general_path=lambda v: v >= size, fast_path=_pos(0), self_cut=lambda v: v >= size - 20,
                     duplicates=lambda v: v >= size - 1, tie_at_cap=lambda v: v >= size)
    return _case(f"a3_cluster{size}", p, general_path=_is(0), self_cut=lambda v: v >= size - 20, duplicates=lambda v: v >= size - 1,
                 tie_at_cap=lambda v: v >= size)


def _a4_point():
    return _case("a4_one_point", np.tile(np.asarray([[0.4, 0.5, 0.6]], F32), (1500, 1)), dims=_is((1, 1, 1)), fullest_cell=_is(1500),
                 general_path=_is(1500), self_cut=_is(1480), extent=_is((0.0, 0.0, 0.0)))


def _a4_line():
    p = np.full((600, 3), 0.5, F32)
    p[:, 0] = (0.2 + 0.6 * _rng(41).random(600)).astype(F32)
    return _case("a4_line", p, dims=lambda d: d[0] > 1 and d[1] == 1 and d[2] == 1, cap_binds=_pos(0), max_in_radius=lambda v: v <= NB_CAP)


def _a4_plane():
    p = np.full((2000, 3), 0.5, F32)
    p[:, :2] = (0.3 + 0.25 * _rng(42).random((2000, 2))).astype(F32)
    return _case("a4_plane", p, dims=lambda d: d[0] > 1 and d[1] > 1 and d[2] == 1, cap_binds=_pos(0))


def _a5_neg():
    return _case("a5_lattice12_at_minus3", lattice(12, origin=-3.0), tie_free=_is(False), tie_at_cap=lambda v: v >= 1000,
                 lo=_is(-3.0), hi=lambda v: v < -2.8)


def _a5_far_lattice():
    # 1000 + 0.25 + k / 128 is a float32 (spacing 2^-14 there): the lattice and all its ties survive the translation
    return _case("a5_lattice12_at_1000", lattice(12, origin=1000.25), tie_free=_is(False), tie_at_cap=lambda v: v >= 1000, lo=_is(1000.25))


def _a5_far_cloud():
    """A random cloud translated to +1000 and rounded to float32 there (spacing 6.1e-5: squared distances are small integers in
    that unit, so equal distances appear), with a clump 5e-4 wide that the rounding folds onto shared grid points."""
    rng = _rng(51)
    p = 1000.0 + 0.3 + side_for(3000, 30.0) * rng.random((3000, 3))
    p[1000:1200] = p[7] + 5e-4 * rng.random((200, 3))
    return _case("a5_cloud_at_1000", p.astype(F32), tie_free=_is(False), duplicates=_pos(0), general_path=lambda v: v >= 200, fast_path=_pos(0),
                 lo=lambda v: v > 1000)


def _a6(gap, name):
    rng = _rng(61)
    a = 0.3 + side_for(300, 25.0) * rng.random((300, 3))
    b = a[:, ::-1] + np.asarray([gap, 0.0, 0.0])
    p = np.concatenate((a, b))
    return _case(name, p[rng.permutation(600)], cells_ok=False, coarsening_rounds=_pos(20), cap_binds=_pos(0),
                 extent=lambda e: e[0] > 0.9 * gap, fullest_cell=lambda v: v <= 300)


def _a6_outlier():
    rng = _rng(62)
    p = np.concatenate((0.3 + side_for(300, 25.0) * rng.random((300, 3)), [[1.0e6, -1.0e6, 1.0e6]]))
    return _case("a6_outlier", p, cells_ok=False, coarsening_rounds=_pos(20), min_in_radius=_is(1), cap_binds=_pos(0),
                 extent=lambda e: min(e) > 9.0e5)


A7_CAPS = (1, 2, 42, 43, 64, 65, 95, 96, 97, 128, 160)


def _a7(cap, mean=96.0, name="a7_straddle"):
    """Mean in-radius count 96 in the bulk, fewer near the faces of the box: queries on both sides of the fast / general hand-off.
    neighbor_kernel changes its LDS request at caps 42 / 43 (64 KiB) and its workgroup size at 64 / 65; 160 is its limit."""
    p = cloud(3000, side_for(3000, mean), 71)
    extra = dict(over_160=_pos(0), cap_binds=_pos(0)) if mean > 96.0 else dict(fast_path=_pos(0), over_160=_is(0))
    if cap <= 97:
        extra["cap_binds"] = _pos(0)
    return _case(f"{name}_cap{cap}", p, cap=cap, general_path=_pos(0), **extra)


def _a8_small(n_per, graphs):
    """Thousands of graphs of 1, 2 or 7 rows on a 2^-9 grid (ties and duplicates inside a graph), all inside one small box: graphs
    overlap in space, and every graph gets a handful of cells."""
    rng = _rng(80 + n_per)
    centre = np.round((0.3 + 0.05 * rng.random((graphs, 1, 3))) * 512.0) / 512.0
    p = centre + rng.integers(-3, 4, size=(graphs, n_per, 3)) / 512.0
    c = _case(f"a8_{graphs}_graphs_of_{n_per}", p.reshape(-1, 3), n_per=n_per, coarsening_rounds=_pos(0),
              dims=lambda d: 1 < d[0] * d[1] * d[2] <= 16, max_in_radius=lambda v: v <= n_per,
              **({} if n_per == 1 else dict(tie_in_kept=_pos(0), duplicates=_pos(0))))
    # another graph's row within the radius of some row: a cross-graph edge would be possible if the batch offset were ignored
    whole = radius_regime(c.pos[:2000], c.r, c.cap)["count"]
    assert whole.max() > n_per, c.name
    return c


def _a8_lattice_batch(graphs=3):
    one = lattice(12)
    return _case(f"a8_lattice12_x{graphs}", np.tile(one, (graphs, 1)), n_per=one.shape[0], tie_free=_is(False), tie_at_cap=lambda v: v >= 1000 * graphs,
                 duplicates=_is(one.shape[0] * (graphs - 1)))


GEOMETRY = {
    "a1_lattice12": lambda: _a1(12),
    "a1_lattice17": lambda: _a1(17),
    "a2_exactly_r": lambda: _a2(2.0 ** -6, 7),
    "a2_just_below_r": lambda: _a2(float(np.nextafter(2.0 ** -6, 0.0)), 1),
    "a3_cluster150": lambda: _a3(150),
    "a3_cluster60": lambda: _a3(60),
    "a4_one_point": _a4_point,
    "a4_line": _a4_line,
    "a4_plane": _a4_plane,
    "a5_lattice12_at_minus3": _a5_neg,
    "a5_lattice12_at_1000": _a5_far_lattice,
    "a5_cloud_at_1000": _a5_far_cloud,
    "a6_gap_1e6": lambda: _a6(1.0e6, "a6_gap_1e6"),
    "a6_gap_1e30": lambda: _a6(1.0e30, "a6_gap_1e30"),
    "a6_outlier": _a6_outlier,
    "a8_3000_graphs_of_1": lambda: _a8_small(1, 3000),
    "a8_3000_graphs_of_2": lambda: _a8_small(2, 3000),
    "a8_3000_graphs_of_7": lambda: _a8_small(7, 3000),
    "a8_lattice12_x3": _a8_lattice_batch,
}
GEOMETRY.update({f"a7_straddle_cap{c}": (lambda c=c: _a7(c)) for c in A7_CAPS})
GEOMETRY["a7_over160_cap160"] = lambda: _a7(160, 200.0, "a7_over160")
GEOMETRY["a7_over160_cap128"] = lambda: _a7(128, 200.0, "a7_over160")


@functools.lru_cache(maxsize=None)
def geometry(name):
    return GEOMETRY[name]()


# ------------------------------------------------------------------------------------------ rollout scenes (Part B)
def scene_with_last_frame(last, cluster_rows=(), seed=0, k=6, rigid_frac=0.1, vel_scale=5e-4):
    """A make_scene-style state [k, n, 8] (rows [id, material, x, y, z, cx, cy, cz], the last `rigid_frac` of the rows rigid) whose
    LAST frame is `last` exactly; earlier frames step back along a random velocity, except for `cluster_rows`, which sit on the same
    point in every frame (coincident rows then have identical features as well)."""
    last = np.asarray(last, F32)
    n = last.shape[0]
    rng = _rng(seed)
    v = vel_scale * rng.standard_normal((n, 3))
    v[list(cluster_rows)] = 0.0
    obs = np.zeros((k, n, 8), F32)
    for t in range(k):
        obs[t, :, 2:5] = (last.astype(np.float64) - (k - 1 - t) * v).astype(F32)
    obs[:, :, 0] = np.arange(n, dtype=F32)
    n_rigid = int(round(n * rigid_frac))
    if n_rigid:
        obs[:, n - n_rigid:, 1] = 1.0
    assert np.array_equal(obs[-1, :, 2:5], last)
    return obs


@dataclass
class SceneCase:
    name: str
    obs: np.ndarray
    geo: GeoCase
    cluster_rows: tuple


def _scene(name, last, cluster_rows=(), seed=0, **expect):
    geo = _case(name, last, **expect)
    return SceneCase(name, scene_with_last_frame(geo.pos, cluster_rows, seed), geo, tuple(cluster_rows))


def _scene_cluster(n, lo, hi, seed, name, **expect):
    base = cloud(n, side_for(n, 20.0), seed)
    rows = np.arange(lo, hi)
    return _scene(name, with_cluster(base, rows, base[lo]), rows, seed + 1, **expect)


SCENES = {
    # 9^3 tie lattice: 343 interior rows whose 20th neighbour is one of 8 equally far
    "lattice9": lambda: _scene("scene_lattice9", lattice(9, seed=91), (), 92, tie_free=_is(False), tie_at_cap=lambda v: v >= 343,
                               general_path=_is(0)),
    # 700 rows, rows 100 .. 299 on one point: 20 rows of in-degree > 200 (long segments with their feature writes, many groups
    # per destination), a third of the queries above 96 candidates
    "cluster200": lambda: _scene_cluster(700, 100, 300, 93, "scene_cluster200", general_path=lambda v: v >= 200, fast_path=_pos(0),
                                         self_cut=lambda v: v >= 180, fullest_cell=lambda v: v <= CELL_ORDER_CAP),
    # 1500 rows, rows 200 .. 1299 on one point: a cell of more than 1024 rows (cell_order_kernel raises order_skip)
    "cluster1100": lambda: _scene_cluster(1500, 200, 1300, 95, "scene_cluster1100", fullest_cell=_pos(CELL_ORDER_CAP), general_path=lambda v: v >= 1100),
}


@functools.lru_cache(maxsize=None)
def scene_case(name):
    return SCENES[name]()


# ------------------------------------------------------------------------------------------ degree structures (Part C)
@dataclass
class DegreeCase:
    name: str
    n: int
    edge_index: np.ndarray          # int64 [2, E], columns in random order
    expect: dict
    props: dict = field(default_factory=dict)

    def measure(self):
        ei, n = self.edge_index, self.n
        e = ei.shape[1]
        indeg = np.bincount(ei[1], minlength=n) if e else np.zeros(n, np.int64)
        in_ptr = np.r_[0, np.cumsum(indeg)]
        hubs = np.flatnonzero(indeg >= GROUP)
        _, counts = np.unique(ei.T, axis=0, return_counts=True) if e else (None, np.zeros(1, np.int64))
        self.props = dict(
            n=n, e=e, indeg=indeg, in_ptr=in_ptr, degrees=set(indeg.tolist()), hubs=hubs.tolist(),
            hub_start=[int(in_ptr[v]) for v in hubs], hub_len=[int(indeg[v]) for v in hubs],
            e_mod_group=e % GROUP, self_loops=int((ei[0] == ei[1]).sum()), max_multiplicity=int(counts.max()),
            isolated_tail=int(n - 1 - np.flatnonzero(indeg)[-1]) if e else n,
            permuted=bool(e < 2 or not np.array_equal(np.argsort(ei[1], kind="stable"), np.arange(e))))
        return self

    def check(self):
        assert self.edge_index.dtype == np.int64 and self.edge_index.shape[0] == 2, self.name
        if self.edge_index.size:
            assert 0 <= self.edge_index.min() and self.edge_index.max() < self.n, self.name
        assert self.expect, self.name
        for key, pred in self.expect.items():
            assert pred(self.props[key]), (self.name, key, self.props[key])


def graph_from_indegrees(name, indeg, seed, self_loop_nodes=(), dup_nodes=(), **expect):
    """edge_index whose destination-sorted list has node v's segment at offset sum(indeg[:v]) with indeg[v] rows: sources are
    random, the nodes in `self_loop_nodes` receive from themselves only, those in `dup_nodes` receive one edge many times over, and
    the columns are shuffled (the destination sort has something to undo)."""
    indeg = np.asarray(indeg, np.int64)
    n = indeg.shape[0]
    rng = _rng(seed)
    dst = np.repeat(np.arange(n, dtype=np.int64), indeg)
    src = rng.integers(0, n, size=dst.shape[0]).astype(np.int64)
    for v in self_loop_nodes:
        src[dst == v] = v
    for v in dup_nodes:
        src[dst == v] = (v * 7 + 3) % n
    ei = np.stack((src, dst))
    ei = np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])]) if ei.shape[1] > 1 else ei
    return DegreeCase(name, n, ei, expect).measure()


def _pad_to(indeg, offset_mod_group, filler=5):
    """Append small segments until the next segment would start at `offset_mod_group` past a group boundary."""
    out = list(indeg)
    while sum(out) % GROUP != offset_mod_group:
        out.append(min(filler, (offset_mod_group - sum(out)) % GROUP))
    return out


def _degrees_every_threshold():
    rng = _rng(101)
    want = [31, 32, 33, 95, 96, 97, 127, 128, 129]
    indeg = []
    for d in want:
        indeg += rng.integers(0, 9, size=5).tolist() + [d]
    indeg += rng.integers(0, 9, size=20).tolist()
    return graph_from_indegrees("c_degrees_31_to_129", indeg, 102, self_loop_nodes=[5], dup_nodes=[11],
                                degrees=lambda s: set(want) <= s, self_loops=_pos(0), max_multiplicity=_pos(1), permuted=_is(True))


def _hub(offset, k=3, name=None, tail=40):
    """A hub of exactly 128 k rows whose segment starts `offset` rows past a group boundary, small segments around it."""
    rng = _rng(110 + offset)
    indeg = _pad_to(rng.integers(1, 9, size=30).tolist(), offset)
    hub = len(indeg)
    indeg += [GROUP * k] + rng.integers(0, 9, size=tail).tolist()
    return graph_from_indegrees(name or f"c_hub{GROUP * k}_at_group_plus_{offset}", indeg, 111 + offset,
                                hubs=_is([hub]), hub_start=lambda s: s[0] % GROUP == offset and s[0] >= GROUP, hub_len=_is([GROUP * k]),
                                permuted=_is(True))


def _hub_node0(n=511):
    """Node 0 is the hub: its segment opens the list.  n + 1 is a multiple of 64, so that the destination list starts right behind the
    structure's cursor array (the word in front of dst[0] is then a defined zero, not padding)."""
    rng = _rng(120)
    indeg = [300] + rng.integers(0, 6, size=n - 1).tolist()
    return graph_from_indegrees("c_hub_is_node0", indeg, 121, hubs=_is([0]), hub_start=_is([0]), n=lambda v: (v + 1) % 64 == 0, permuted=_is(True))


def _hub_last(n=400):
    rng = _rng(122)
    indeg = rng.integers(0, 6, size=n - 1).tolist() + [300]
    return graph_from_indegrees("c_hub_is_last_node", indeg, 123, hubs=_is([n - 1]), isolated_tail=_is(0), permuted=_is(True))


def _hub_then_isolated():
    rng = _rng(124)
    indeg = rng.integers(1, 6, size=50).tolist() + [333] + [0] * 200
    return graph_from_indegrees("c_hub_then_isolated", indeg, 125, hubs=_is([50]), isolated_tail=_is(200), permuted=_is(True))


def _e_mod(rem):
    rng = _rng(130 + rem)
    indeg = rng.integers(0, 12, size=300).tolist()
    indeg = _pad_to(indeg, rem, filler=7)
    return graph_from_indegrees(f"c_e_is_128k_plus_{rem}", indeg, 131 + rem, e_mod_group=_is(rem), e=_pos(10 * GROUP), permuted=_is(True))


def _no_edges():
    return DegreeCase("c_no_edges", 70, np.zeros((2, 0), np.int64), dict(e=_is(0), n=_pos(0))).measure()


def _one_edge():
    return DegreeCase("c_one_edge", 70, np.asarray([[3], [41]], np.int64), dict(e=_is(1))).measure()


def _all_into_one():
    indeg = [0] * 90
    indeg[37] = 1000
    return graph_from_indegrees("c_all_into_one_node", indeg, 140, hubs=_is([37]), degrees=_is({0, 1000}))


def _hub_graph_style():
    """Self loops and exact duplicates next to hubs, in the style of _hub_graph of test_gpu_train_regimes.py."""
    rng = _rng(150)
    n, e = 400, 6000
    ei = rng.integers(0, 390, size=(2, e)).astype(np.int64)
    ei[1, :700] = 17
    ei[1, 700:1000] = 233
    ei[:, 2000:2064] = ei[:, 2100:2164]
    ei[:, 2064:2072] = ei[:, 2100:2101]
    ei[0, 2200:2300] = ei[1, 2200:2300]
    ei = np.ascontiguousarray(ei[:, rng.permutation(e)])
    return DegreeCase("c_hubs_loops_duplicates", n, ei, dict(hubs=_is([17, 233]), self_loops=lambda v: v >= 100,
                                                               max_multiplicity=lambda v: v >= 10, isolated_tail=_pos(0), permuted=_is(True))).measure()


DEGREES = {
    "c_degrees_31_to_129": _degrees_every_threshold,
    "c_hub384_at_group_plus_0": lambda: _hub(0),
    "c_hub384_at_group_plus_1": lambda: _hub(1),
    "c_hub_is_node0": _hub_node0,
    "c_hub_is_last_node": _hub_last,
    "c_hub_then_isolated": _hub_then_isolated,
    "c_e_is_128k_plus_0": lambda: _e_mod(0),
    "c_e_is_128k_plus_1": lambda: _e_mod(1),
    "c_no_edges": _no_edges,
    "c_one_edge": _one_edge,
    "c_all_into_one_node": _all_into_one,
    "c_hubs_loops_duplicates": _hub_graph_style,
}


@functools.lru_cache(maxsize=None)
def degree_case(name):
    return DEGREES[name]()


# ------------------------------------------------------------------------------------------ the 32-edge block tables, restated
def block_tables(dst_sorted, n_nodes):
    """What edge_blocks_plan / edge_blocks_fill (csrc/blocks_dev.h) document for ONE graph, from the destination-sorted list:
    blocks of 32 edges padded to a multiple of 4 (one group = 128 edges); per block (first edge, count, first-of-group /
    last-of-group flags) and the bit masks cont (row continues the segment of the row in front, inside its group) and last (row
    ends its piece: the segment ends, or the group does); per group head = the destination whose segment continues from the
    group in front, else -1; stitch[v] = the first group of v's run of head partials, else -1."""
    dst = np.asarray(dst_sorted, np.int64)
    e = dst.shape[0]
    nblk = ((e + BLOCK - 1) // BLOCK + 3) & ~3
    b = np.arange(nblk)
    start = np.minimum(b * BLOCK, e)
    cnt = np.minimum(BLOCK, e - start)
    blk = np.stack((start, cnt | (((b % 4 == 0) * 1 | (b % 4 == 3) * 2) << 8)), axis=1)
    p = np.arange(e)
    same_as_prev = np.r_[False, dst[1:] == dst[:-1]][:e]
    cont_bit = same_as_prev & (p % GROUP != 0)
    last_bit = np.r_[~same_as_prev[1:], True][:e] | (p % GROUP == GROUP - 1)
    bits = np.zeros((2, nblk * BLOCK), np.int64)
    bits[0, :e], bits[1, :e] = cont_bit, last_bit
    seg = (bits.reshape(2, nblk, BLOCK) << np.arange(BLOCK)).sum(axis=2).T      # [nblk, (cont, last)]
    g_start = start[::4]
    head = np.full(nblk // 4, -1, np.int64)
    is_head = (cnt[::4] > 0) & (g_start > 0)
    is_head[is_head] = same_as_prev[g_start[is_head]]
    head[is_head] = dst[g_start[is_head]]
    stitch = np.full(n_nodes, -1, np.int64)
    for g in range(nblk // 4 - 1, -1, -1):
        if head[g] >= 0:
            stitch[head[g]] = g     # descending: the first group of the run is written last
    return dict(n_blocks=nblk, blk=blk, seg=seg, head=head, stitch=stitch)
