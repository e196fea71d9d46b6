"""Cases of the ragged rollout (gm_rollout_step_ragged, gm_rollout_ragged, gm_rollout_recorded_ragged, gm_rollout_errors_ragged,
RolloutEngine(sizes=...), evaluate_rollout(ragged=True)): batches of recorded scenes of DIFFERENT sizes stored back to back along
the node axis -- a plain helper module shared by test_ragged_rollout_cases.py (CPU: every case is in the regime it was built
for), test_abi_ragged_rollout.py (CPU) and test_gpu_ragged_rollout.py (GPU).

What the GPU tests hold the batch to is the same scene rolled ALONE: there is no tolerance anywhere, every comparison is bit for
bit.  The thresholds named here are the kernels': NB_QPB (16 queries per workgroup of neighbor_fast_kernel), the 256 rows per
workgroup of cell_assign_kernel, the 32-edge blocks and 4-block groups (128 edges) of the processor kernels' block tables, over
which the scatter-add carries a running sum: a destination with more than 128 incoming edges has a segment longer than a group,
whose later pieces are head partials on the stitch list."""
import functools

import numpy as np

from gnn_manip_amd import scene
from oracle import epd_oracle as orc
import eval_cases as ec
import ragged_cases as rgc
import train_step_cases as tsc
import width_cases as wc

F32 = np.float32
R = ec.R
L = wc.LAYOUTS["default"]
STEPS = 3
T_FRAMES = L.k + STEPS                     # frames of a recording: the first window and one frame per step
GROUP_EDGES = 128                          # 4 blocks of 32 edges
CLUMP = 140                                # rows of a clump: all inside one radius, more than GROUP_EDGES of them

# the models the forward is run with: name -> (hidden, num_layers, m_steps, set_edge_kernel, set_precision)
SMALL = tsc.SMALL
MODELS = {"h64": (SMALL[3], SMALL[4], SMALL[5], None, None),
          "h128_hm": (128, 2, 2, "hm", None), "h128_sys": (128, 2, 2, "sys", None), "h128_sys_all": (128, 2, 2, "sys_all", None),
          "h128_f16": (128, 2, 2, None, "f16")}
SYS_NODE_MIN_NODES = 32 * 256 * 6          # hedge.h kSysNodeMinNodes: every graph of every case lies below it


def model(name):
    """(dims, float32 parameters with a damped decoder, edge kernel, precision)."""
    hidden, nl, ms, kernel, precision = MODELS[name]
    dims, params = ec.model_params(L, hidden, nl, ms)
    return dims, params, kernel, precision


class Scene:
    """One recorded scene [T_FRAMES, n, D] in the default layout: make_scene's frames with the dataset's control columns
    (coffee_dataset.py:91-97).  clump = (rows, point): those rows sit within a thousandth of `point` in frame 0 and move a fifth
    of the way make_scene moved them, so they stay inside one radius of each other over the few steps of a test."""

    def __init__(self, n, seed, rigid_frac=0.1, clump=None):
        base = scene.make_scene(n, seed=seed, k=T_FRAMES, rigid_frac=rigid_frac, side=0.05)
        if clump is not None:
            rows, point = clump
            p0 = np.asarray(point, np.float64) + 1e-3 * wc._rng(seed + 1).standard_normal((len(rows), 3))
            moved = 0.2 * (base[:, rows, 2:5].astype(np.float64) - base[0, rows, 2:5].astype(np.float64))
            base[:, rows, 2:5] = (p0[None] + moved).astype(F32)
        sim = np.ascontiguousarray(base[:, :, :L.D])
        rigid = sim[0, :, L.mat] == 1
        sim[:-1, :, L.ctrl:L.ctrl + 3] = np.where(rigid[None, :, None], sim[1:, :, 2:5] - sim[:-1, :, 2:5], F32(0))
        sim[-1, :, L.ctrl:L.ctrl + 3] = 0
        self.n, self.sim, self.rigid = n, sim, rigid
        self.sim.setflags(write=False)

    def window(self):
        return np.array(self.sim[:L.k])

    def frames(self, steps=STEPS):
        return np.array(self.sim[L.k - 1:L.k - 1 + steps])

    def trajectory(self, seed, steps=STEPS):
        return wc.drift_trajectory(self.window(), L, steps, seed)


class Case:
    def __init__(self, name, scenes, max_nb=20, expect=None):
        self.name, self.scenes, self.max_nb = name, scenes, max_nb
        self.sizes = tuple(s.n for s in scenes)
        self.offsets = rgc.offsets(self.sizes)
        self.expect = expect or {}

    def window(self):
        return np.ascontiguousarray(np.concatenate([s.window() for s in self.scenes], axis=1))

    def frames(self, steps=STEPS):
        return np.ascontiguousarray(np.concatenate([s.frames(steps) for s in self.scenes], axis=1))

    def recording(self):
        return np.ascontiguousarray(np.concatenate([s.sim for s in self.scenes], axis=1))

    def trajectories(self, steps=STEPS):
        """Per scene [steps, n_rigid_g, 3] (a scene without rigid rows: an empty array)."""
        return [s.trajectory(950 + g, steps) for g, s in enumerate(self.scenes)]

    def trajectory(self, steps=STEPS):
        """[steps, n_rigid, 3] of the batch: ranks are global, scene g's rigid rows behind those of the scenes before it."""
        return np.ascontiguousarray(np.concatenate(self.trajectories(steps), axis=1))

    def rows(self, g):
        return slice(int(self.offsets[g]), int(self.offsets[g + 1]))

    @functools.lru_cache(maxsize=None)
    def measure(self):
        """The regime on the oracle's graphs of the first window: per scene the edge count and the in-degrees of its rows."""
        edges, indeg = [], []
        for s in self.scenes:
            _, rcv = orc.get_connectivity(s.sim[L.k - 1][:, L.cart_idx], R, self.max_nb)
            edges.append(int(rcv.shape[0]))
            indeg.append(np.bincount(rcv, minlength=s.n))                 # messages are summed at edge_index[1]
        off = self.offsets
        return dict(sizes=self.sizes, n_graphs=len(self.sizes), edges=tuple(edges), indeg=indeg,
                    edges_mod_group=tuple(e % GROUP_EDGES for e in edges),
                    boundaries_mod_16=tuple(int(o % rgc.NB_QPB) for o in off[1:-1]),
                    boundaries_mod_256=tuple(int(o % rgc.ASSIGN_BLOCK) for o in off[1:-1]),
                    rigid=tuple(int(s.rigid.sum()) for s in self.scenes))

    def check(self):
        props = self.measure()
        assert self.expect, self.name
        assert max(self.sizes) < SYS_NODE_MIN_NODES and 1 <= len(self.sizes) <= rgc.GM_RAGGED_MAX_GRAPHS
        for key, pred in self.expect.items():
            assert pred(props[key]), (self.name, key, props[key])


def _is(v):
    return lambda x: x == v


def _mixed():
    # offsets 256 (ON the 16-query and the 256-row edge) and 353 (off both); the middle scene has no rigid row
    return Case("mixed", [Scene(256, 960), Scene(97, 961, rigid_frac=0.0), Scene(300, 962)], expect=dict(
        sizes=lambda v: len(set(v)) == 3, boundaries_mod_16=_is((0, 1)), boundaries_mod_256=_is((0, 97)),
        edges_mod_group=lambda v: all(v), rigid=lambda v: v[0] > 0 and v[1] == 0 and v[2] > 0))


def _single_row():
    # the radius graph keeps every row's edge to itself (KDTree.query_radius returns the query): a scene of one row has that edge
    # and no other -- no edge to another row, one block of one edge
    return Case("single_row", [Scene(130, 963), Scene(1, 964), Scene(77, 965)], expect=dict(
        sizes=_is((130, 1, 77)), edges=lambda v: v[1] == 1, rigid=lambda v: v[1] == 0, edges_mod_group=lambda v: all(v)))


def _clump():
    # the last CLUMP rows of scene 0 and the first CLUMP rows of scene 1 each lie inside one radius, at max_neighbours = 160: every
    # one of those rows receives more than 128 edges, so segments longer than a group end scene 0's edge list and begin scene 1's
    point = (0.32, 0.33, 0.31)
    n = 200
    return Case("clump", [Scene(n, 966, clump=(np.arange(n - CLUMP, n), point)), Scene(n, 967, clump=(np.arange(CLUMP), point))],
                max_nb=160, expect=dict(
        indeg=lambda v: v[0][n - CLUMP:].min() > GROUP_EDGES and v[1][:CLUMP].min() > GROUP_EDGES, edges_mod_group=lambda v: all(v)))


def _equal():
    return Case("equal", [Scene(150, 968 + g) for g in range(3)], expect=dict(sizes=_is((150,) * 3), edges_mod_group=lambda v: all(v)))


def _one():
    return Case("one", [Scene(301, 971)], expect=dict(n_graphs=_is(1), edges_mod_group=lambda v: all(v)))


CASES = {"mixed": _mixed, "single_row": _single_row, "clump": _clump, "equal": _equal, "one": _one}
# the model variants every case is run with; the clump adds the systolic kernels, whose tables hold the head partials
CASE_MODELS = {"mixed": tuple(MODELS), "single_row": ("h64", "h128_sys"), "clump": ("h64", "h128_hm", "h128_sys", "h128_sys_all"),
               "equal": ("h64", "h128_sys"), "one": ("h64", "h128_sys")}
FORWARD = [(c, m) for c in CASES for m in CASE_MODELS[c]]


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


# ------------------------------------------------------------------------------------------ evaluate_rollout
def eval_sims():
    """Recordings of two sizes, two of each, interleaved: the default call makes two groups, ragged=True one."""
    return [Scene(97, 980), Scene(130, 981), Scene(97, 982), Scene(130, 983)]


# ------------------------------------------------------------------------------------------ refusals
def refusals(sizes):
    """name -> (offsets, nodes_per_graph, workspace bytes short): what every _ragged rollout entry point refuses."""
    good = [int(v) for v in rgc.offsets(sizes)]
    n = good[-1]
    return {"nodes_per_graph": (good, sizes[0], 0),
            "offsets_start": ([1] + good[1:], 0, 0),
            "empty_graph": (good[:2] + [good[1]] + good[2:], 0, 0),
            "too_many_graphs": (list(range(rgc.GM_RAGGED_MAX_GRAPHS + 1)) + [n], 0, 0),
            "workspace": (good, 0, 1)}


# ------------------------------------------------------------------------------------------ the loss of a ragged batch
LOSS_SIZES = (300, 97, 33)                  # workgroups of the loss kernels: two, one and one, none of them full
LOSS_STEPS = 2
LOSS_RTOL = 1e-12                           # float64 sums of at most 1e3 float32 terms in another order: 1e3 x 2^-53 = 1.1e-13


# The shapes at which ONE set of loss kernels, shared by the single call and the batch, can go wrong.  "tail": graph 1 is past one
# pass of the capped grid with a ragged tail (33025 = 128 * 256 + 257: the second pass has one full workgroup and one with a
# single row) beside a one-row graph, whose other 127 workgroups of the launch row leave without writing, and a graph of exactly
# one full workgroup.  "cap": GM_RAGGED_MAX_GRAPHS graphs -- the table and the frame pointers at their cap, the search for a row's
# graph through all its depths; with a material column the graphs LOSS_CAP_EMPTY count no row.
LOSS_SHAPES = {"tail": (1, 33025, 256), "cap": tuple((1, 2, 3, 5)[g % 4] for g in range(rgc.GM_RAGGED_MAX_GRAPHS))}
LOSS_SHAPE_MASKS = ("none", "rigid_material")
LOSS_CAP_EMPTY = (0, 17, 42, 63)            # one graph of every size, the first and the last graph among them


def loss_shape(name, k, frame_dim, mask):
    """loss_batch at LOSS_SHAPES[name]; "cap" under a mask with a material column: the graphs LOSS_CAP_EMPTY count no row."""
    import train_rollout_cases as trc
    empty = LOSS_CAP_EMPTY if name == "cap" and trc.LOSS_MASKS[mask][1] else ()
    return loss_batch(k, frame_dim, mask, sizes=LOSS_SHAPES[name], empty=empty)


def loss_rtol(steps, counted):
    """Every term |pred - frame| is non-negative, so a float64 sum of T = steps * rows counted terms in another order differs by
    at most T * 2^-53 relative; the divisions behind the sums are the restatement's own."""
    return float(steps) * np.asarray(counted, np.float64) * 2.0 ** -53


def loss_batch(k, frame_dim, mask, sizes=LOSS_SIZES, steps=LOSS_STEPS, empty=()):
    """train_rollout_cases.loss_case per graph (its own seed), and the batch assembled from them: dict(parts=[case per graph],
    windows [steps,k,N,D], final [k,N,D], frames=[per graph], rank int32 [N] with GLOBAL ranks or None, material_col, pos_scale).
    empty: graphs built under the "empty" mask instead (every material flag 1: nothing counts), for a mask with a material column."""
    import train_rollout_cases as trc
    parts = [trc.loss_case(n, steps, k, frame_dim, "empty" if g in empty else mask, seed=40 + g) for g, n in enumerate(sizes)]
    for g in empty:
        assert trc.LOSS_MASKS[mask][:2] == (True, True), mask
        parts[g]["pos_scale"] = trc.LOSS_MASKS[mask][2]                  # the single call on the graph alone takes the batch's scale
    rank = None
    if parts[0]["rank"] is not None:
        ranks, base = [], 0
        for p in parts:
            ranks.append(np.where(p["rank"] >= 0, p["rank"] + base, -1).astype(np.int32))
            base += int((p["rank"] >= 0).sum())
        rank = np.concatenate(ranks)
    return dict(parts=parts, windows=np.ascontiguousarray(np.concatenate([p["windows"] for p in parts], axis=2)),
                final=np.ascontiguousarray(np.concatenate([p["final"] for p in parts], axis=1)), frames=[p["frames"] for p in parts],
                rank=rank, material_col=parts[0]["material_col"], pos_scale=parts[0]["pos_scale"], sizes=tuple(sizes))


def rollout_l1_restated_ragged(windows, final, frames_list, sizes, cart, rank=None, material_col=-1, pos_scale=None):
    """train_rollout_cases.rollout_l1_restated per graph of a batch: (losses float64 [G], rows counted [G], d_records [steps,N,D],
    d_final [k,N,D]) as gm_rollout_l1_loss_ragged defines them -- graph g's loss and gradient scale come from its own rows and
    its own count; whether a rigid row counts depends on the sign of its (global) rank alone."""
    import train_rollout_cases as trc
    off = rgc.offsets(sizes)
    losses, counts, d_rec, d_fin = [], [], [], []
    for g, frames in enumerate(frames_list):
        rows = slice(int(off[g]), int(off[g + 1]))
        loss, count, dr, df = trc.rollout_l1_restated(windows[:, :, rows], final[:, rows], frames, cart,
                                                      None if rank is None else rank[rows], material_col, pos_scale)
        losses.append(loss), counts.append(count), d_rec.append(dr), d_fin.append(df)
    return np.asarray(losses, np.float64), np.asarray(counts, np.int64), np.concatenate(d_rec, axis=1), np.concatenate(d_fin, axis=1)


def batch_loss(losses):
    """What a ragged mini-batch leaves behind its loss: (the graphs' losses added in graph order, how many are not finite)."""
    total = float(losses[0])
    for v in losses[1:]:
        total += float(v)
    return total, int(sum(not np.isfinite(v) for v in losses))


# ------------------------------------------------------------------------------------------ the sweep and the training mini-batch
SWEEP_CASE, SWEEP_STEPS = "single_row", 2    # 130 + 1 + 77 rows: the restated float64 sweeps stay quick
W_FINAL_SEED, W_RECORD_SEED = 16, 19
