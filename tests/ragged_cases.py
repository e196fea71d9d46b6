"""Seeded inputs for the ragged builds (gm_radius_graph_build_ragged, gm_train_batch_build_ragged / _edges_ragged): batches of
graphs of DIFFERENT sizes stored back to back -- a plain helper module shared by test_ragged_cases.py (CPU), test_abi_ragged.py
(CPU) and test_gpu_ragged.py (GPU).

Pure numpy (PCG64), on the generators of graph_cases.py and the recordings of train_batch_cases.py.  All graphs of a graph case
lie in the same box, so rows of different graphs are within the radius of each other: an edge across graphs is possible wherever
the build mistakes the graph of a row.  The thresholds named here are the kernels': NB_QPB (16 queries per workgroup of
neighbor_fast_kernel), the 256 rows per workgroup of cell_assign_kernel, NB_CAP (96 candidates: the general kernel, 128 queries
per workgroup up to cap 64 and 64 above), GM_RAGGED_MAX_GRAPHS (64 graphs per build)."""
import functools
from dataclasses import dataclass, field

import numpy as np

import graph_cases as gc
import train_batch_cases as tc

F32 = np.float32
R = gc.R
NB_QPB = 16
ASSIGN_BLOCK = 256
GM_RAGGED_MAX_GRAPHS = 64
MAX_ROWS = 3 * 12 ** 3                 # the largest case is graph_cases' 3 x 12^3 tie lattice; every other one has at most 4099 rows


def offsets(sizes):
    return np.r_[0, np.cumsum(np.asarray(sizes, np.int64))]


def graph_of_rows(sizes):
    return np.repeat(np.arange(len(sizes)), sizes)


# ------------------------------------------------------------------------------------------ two formulations of the result
def brute_force(pos, sizes, r, cap):
    """The ragged contract stated on the WHOLE cloud: d2 <= r * r AND same graph, ranked by (d2, index), cut at the cap."""
    pos = np.asarray(pos)
    graph = graph_of_rows(sizes)
    s, rcv = [], []
    for a in range(0, pos.shape[0], 512):
        d2 = gc._sq_dists(pos[a:a + 512], pos)
        ok = (d2 <= float(r) * float(r)) & (graph[a:a + 512, None] == graph[None, :])
        for row in range(d2.shape[0]):
            idx = np.nonzero(ok[row])[0]
            idx = idx[np.lexsort((idx, d2[row, idx]))][:cap]
            s.append(np.full(idx.shape[0], a + row, np.int64))
            rcv.append(idx.astype(np.int64))
    return np.concatenate(s), np.concatenate(rcv)


def per_graph(connectivity, pos, sizes, r, cap):
    """`connectivity(pos_g, r, cap)` on each graph's rows, with the graph's row offset on its indices, concatenated."""
    s, rcv = [], []
    for o, n in zip(offsets(sizes)[:-1], sizes):
        sg, rg = connectivity(pos[o:o + n], r, cap)
        s.append(np.asarray(sg, np.int64) + o)
        rcv.append(np.asarray(rg, np.int64) + o)
    return np.concatenate(s), np.concatenate(rcv)


def ragged_grid(pos, r, n_graphs):
    """The grid of a ragged build -- graph_cases.engine_grid's restatement of grid_params with the number of graphs given: ONE
    geometry over the whole cloud, coarsened until it fits max(2n, 32768) / n_graphs cells.  Returns (dims, coarsening rounds)."""
    pos = np.asarray(pos, np.float64)
    max_cells = max(min(max(2 * pos.shape[0], 32768), 1 << 22) // n_graphs, 1)
    ext = pos.max(axis=0) - pos.min(axis=0)
    h, rounds = float(r) * (1.0 + 1.0 / 1024.0), 0
    while True:
        dims = np.minimum(np.floor(ext / h) + 1.0, 2.0e9)
        if dims.prod() <= max_cells:
            return dims.astype(np.int64), rounds
        h *= 1.2599210498948732
        rounds += 1


# ------------------------------------------------------------------------------------------ graph cases
@dataclass
class RaggedCase:
    name: str
    pos: np.ndarray                 # float32 [n, 3]
    sizes: tuple
    cap: int
    r: float = R
    expect: dict = field(default_factory=dict)    # property name -> predicate on its value
    props: dict = field(default_factory=dict)

    def measure(self):
        off = offsets(self.sizes)
        whole = gc.radius_regime(self.pos, self.r, self.cap)["count"]                 # without the graph split
        parts = [gc.radius_regime(self.pos[o:o + n], self.r, self.cap) for o, n in zip(off[:-1], self.sizes)]
        own = np.concatenate([p["count"] for p in parts])                           # with it
        n = self.pos.shape[0]
        dims, rounds = ragged_grid(self.pos, self.r, len(self.sizes))
        self.props = dict(
            n=n, n_graphs=len(self.sizes), sizes=tuple(int(v) for v in self.sizes),
            boundaries_mod_16=tuple(int(o % NB_QPB) for o in off[1:-1]), boundaries_mod_256=tuple(int(o % ASSIGN_BLOCK) for o in off[1:-1]),
            blocks_256=int(-(-n // ASSIGN_BLOCK)),
            leak_rows=int((whole > own).sum()),                                      # rows with an in-radius row of ANOTHER graph
            leak_rows_per_graph=tuple(int((whole[o:o + m] > own[o:o + m]).sum()) for o, m in zip(off[:-1], self.sizes)),
            cap_binds_per_graph=tuple(int((p["count"] > self.cap).sum()) for p in parts),
            general_per_graph=tuple(int((p["count"] > gc.NB_CAP).sum()) for p in parts),
            fast_rows=int((own <= gc.NB_CAP).sum()),
            tie_free=not any(p["tie_in_kept"].any() for p in parts),
            tie_at_cap=int(sum(p["tie_at_cap"].sum() for p in parts)),
            coarsening_rounds=rounds, dims=tuple(int(d) for d in dims))
        return self

    def check(self):
        assert self.pos.dtype == F32 and self.pos.shape == (sum(self.sizes), 3) and np.isfinite(self.pos).all(), self.name
        assert self.pos.shape[0] <= MAX_ROWS and 1 <= len(self.sizes) <= GM_RAGGED_MAX_GRAPHS and min(self.sizes) >= 1, self.name
        assert self.expect, self.name
        for key, pred in self.expect.items():
            assert pred(self.props[key]), (self.name, key, self.props[key])


def _case(name, parts, cap=20, **expect):
    pos = np.ascontiguousarray(np.concatenate(parts), dtype=F32)
    return RaggedCase(name, pos, tuple(int(p.shape[0]) for p in parts), int(cap), expect=expect).measure()


def _cloud25(n, seed):
    """About 25 rows in radius where the size allows (a graph of fewer rows is wholly inside one radius)."""
    return gc.cloud(n, gc.side_for(n, 25.0), seed)


def _edges_of_blocks():
    sizes = (1, 15, 17, 255, 257, 1, 16)
    # offsets 1, 16, 33, 288, 545, 546: on the 16-query edge at 16 and 288 (= 18 * 16) and off it elsewhere; the first workgroup
    # of cell_assign_kernel holds graphs 0 .. 3 and the head of graph 4, the 256-row edges at 256 and 512 fall INSIDE graphs 3 and 4
    return _case("edges_of_blocks", [_cloud25(n, 300 + g) for g, n in enumerate(sizes)],
                 sizes=gc._is(sizes), boundaries_mod_16=gc._is((1, 0, 1, 0, 1, 2)), boundaries_mod_256=gc._is((1, 16, 33, 32, 33, 34)),
                 blocks_256=gc._is(3), cap_binds_per_graph=lambda v: v[3] > 0 and v[4] > 0, leak_rows=gc._pos(200), tie_free=gc._is(True))


def _copies():
    base = _cloud25(97, 310)
    return _case("copies", [base, base, base, base[:64]], sizes=gc._is((97, 97, 97, 64)), leak_rows=gc._is(97 * 3 + 64),
                 cap_binds_per_graph=lambda v: v[0] > 0 and v[0] == v[1] == v[2], tie_free=gc._is(True))


def _full_table():
    sizes = gc._rng(320).integers(1, 41, size=GM_RAGGED_MAX_GRAPHS)
    return _case("full_table", [gc.cloud(int(n), gc.side_for(40, 25.0), 321 + g) for g, n in enumerate(sizes)],
                 n_graphs=gc._is(GM_RAGGED_MAX_GRAPHS), sizes=lambda v: min(v) >= 1 and max(v) <= 40 and len(set(v)) > 10,
                 leak_rows=gc._pos(500), tie_free=gc._is(True))


def _general_path(cap):
    g0, g1, g2 = _cloud25(300, 330), _cloud25(40, 331), _cloud25(500, 332)
    point = g0[17]
    g0 = gc.with_cluster(g0, np.arange(100, 250), point)
    g2 = gc.with_cluster(g2, np.arange(200, 350), point)        # the same point: 300 coincident rows, 150 in each of two graphs
    return _case(f"general_path_cap{cap}", [g0, g1, g2], cap=cap, sizes=gc._is((300, 40, 500)),
                 general_per_graph=lambda v: v[0] >= 150 and v[1] == 0 and v[2] >= 150, fast_rows=gc._pos(0),
                 leak_rows_per_graph=lambda v: v[0] >= 150 and v[2] >= 150, tie_at_cap=gc._pos(299), tie_free=gc._is(False))


def _equal():
    c = gc.geometry("a8_lattice12_x3")
    return _case("equal", [c.pos[g * c.n_per:(g + 1) * c.n_per] for g in range(3)], sizes=gc._is((1728,) * 3), tie_free=gc._is(False),
                 tie_at_cap=lambda v: v >= 3000, leak_rows=gc._is(3 * 1728))


def _big_and_tiny():
    big = _cloud25(4096, 340)
    return _case("big_and_tiny", [big, big[[5, 900, 4000]] + F32(1e-3)], sizes=gc._is((4096, 3)), leak_rows=gc._pos(50),
                 cap_binds_per_graph=lambda v: v[0] > 1000 and v[1] == 0, tie_free=gc._is(True))


def _far_apart():
    a = _cloud25(300, 350)
    b = _cloud25(300, 351).astype(np.float64)
    b[:, 0] += 1.0e6                                               # x rounds to float32's grid there (spacing 1/16): a sheet
    return _case("far_apart", [a, b.astype(F32)], sizes=gc._is((300, 300)), coarsening_rounds=lambda v: v >= 20,
                 cap_binds_per_graph=lambda v: v[0] > 0 and v[1] > 0)


GRAPHS = {
    "edges_of_blocks": _edges_of_blocks,
    "copies": _copies,
    "full_table": _full_table,
    "general_path_cap20": lambda: _general_path(20),
    "general_path_cap128": lambda: _general_path(128),
    "equal": _equal,
    "big_and_tiny": _big_and_tiny,
    "far_apart": _far_apart,
}


@functools.lru_cache(maxsize=None)
def graph_case(name):
    return GRAPHS[name]()


# ------------------------------------------------------------------------------------------ training-batch cases
class BatchCase:
    """Samples of different sizes: sample b is frame `t` on of a recording of its own with `n` rows (train_batch_cases.Case's
    make_scene recordings; two samples of equal n and seed share the recording)."""

    def __init__(self, name, samples, k=6, control=True, max_nb=20):
        self.name, self.k, self.control, self.max_nb = name, k, control, max_nb
        self.parts = [tc.Case(f"{name}_{b}", n, k, [(0, t)], control=control, max_nb=max_nb, seed=seed) for b, (n, t, seed) in enumerate(samples)]
        self.sizes = tuple(n for n, _, _ in samples)
        self.first_frames = tuple(t for _, t, _ in samples)
        self.B = len(samples)

    def recordings(self):
        """[B] float32 [T_b, N_b, 5]: the recording sample b is cut from (T_b = first frame + k + 1)."""
        return [p.recordings()[0] for p in self.parts]

    def windows(self):
        return [p.windows()[0] for p in self.parts]

    def graph_kw(self, max_nb=None):
        return self.parts[0].graph_kw(max_nb)


BATCHES = {c.name: c for c in (
    BatchCase("mixed6", [(64, 0, 21), (97, 2, 22), (97, 1, 23), (300, 0, 24)], max_nb=12),
    BatchCase("mixed_k2_noctl", [(130, 0, 25), (33, 0, 26)], k=2, control=False),
    BatchCase("mixed_cap5", [(300, 0, 27), (64, 0, 28)], max_nb=5),
    BatchCase("same97", [(97, 0, 29), (97, 2, 29), (97, 1, 30)]),
)}
LOADER_N = (64, 97, 300)              # the loader tests: recordings of these sizes, batch_size 3

# gm_graph_workspace_bytes(n_nodes, max_neighbours) and gm_train_batch_workspace_bytes(fdesc of k = 6 with control columns, batch,
# nodes_per_graph, max_neighbours) as the library returned them BEFORE the ragged entry points existed (read from that build on the
# CPU: the queries need no device).  The ragged builds add nothing to these layouts.
GRAPH_WS_BYTES = {(1, 1): 264448, (97, 20): 274432, (1177, 20): 390912, (4099, 20): 706816, (16384, 20): 2033152,
                  (20000, 128): 11121408, (100000, 160): 68402432}
TRAIN_BATCH_WS_BYTES = {(1, 64, 20): 271616, (3, 97, 20): 299008, (2, 300, 5): 300288, (4, 1025, 12): 625408, (64, 64, 20): 755456,
                        (2, 5000, 20): 1464064}
