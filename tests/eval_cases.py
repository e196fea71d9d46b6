"""Cases and numpy restatements of the evaluation path: the recorded drive (gm_state_recorded, gm_rollout_recorded --
compute_rollout's ground-truth mode, rollout_utils.py:38-61 with args.cma_traj None) and the error sums behind the model
comparison (gm_rollout_errors, evaluate_rollout).  tests/test_eval_cases.py holds the restatements to independent formulations
on the CPU, tests/test_gpu_eval.py holds the HIP kernels to the restatements.

The recorded drive copies float32 values: a device result has nothing to differ by, every comparison with it is bit for bit.
The sums are float64 sums of non-negative float64 terms, each term the same IEEE expression here and on the device: only the
order of the additions differs, at most 1e3 terms per sum x 2^-53 = 1.1e-13 relative; the bar is 1e-12."""
import numpy as np

from conftest import STATS
from gnn_manip_amd import scene
from oracle import epd_oracle as orc
import width_cases as wc

F32, F64 = np.float32, np.float64
R = wc.R
K_NB = 20
GM_RECORDED_CONTROL, GM_RECORDED_POSE = 1, 4
SUM_RTOL = 1e-12

# ------------------------------------------------------------------------------------------ the row kernels
SIZES = (1, 63, 64, 65, 257, 1000)          # the wave (64) and workgroup (256) edges of a 256-thread launch
KS = (2, 6)
RIGID = ("none", "one", "all")
ROW_LAYOUTS = {2: wc.LAYOUTS["k2"], 6: wc.LAYOUTS["default"]}
ROW_CASES = [(n, k, rigid, mapped) for n in SIZES for k in KS for rigid in RIGID for mapped in (False, True)]


def row_case_id(c):
    return f"n{c[0]}-k{c[1]}-rigid_{c[2]}-{'row_map' if c[3] else 'identity'}"


def rigid_rank(n, rigid):
    """int32 [n]: the rank of each rigid row among the rigid rows, -1 elsewhere (gm_rigid_rank's output)."""
    rank = np.full(n, -1, np.int32)
    if rigid == "one":
        rank[n // 2] = 0
    elif rigid == "all":
        rank[:] = np.arange(n)
    return rank


def row_inputs(n, k, mapped):
    """(window [k, n, D], frame [n, D], row_map int32 [n] or None): seeded values, every element distinct in practice."""
    L = ROW_LAYOUTS[k]
    rng = np.random.default_rng(1000 * k + n + (500 if mapped else 0))
    obs = rng.standard_normal((k, n, L.D)).astype(F32)
    frame = rng.standard_normal((n, L.D)).astype(F32)
    row_map = rng.permutation(n).astype(np.int32) if mapped else None
    return obs, frame, row_map


def state_recorded(obs, L, rank, frame, row_map, what):
    """gm_state_recorded: on the rigid rows of the last frame the control columns (what = GM_RECORDED_CONTROL) or xyz
    (GM_RECORDED_POSE) take those of `frame`, state row j reading the frame's row row_map[j]."""
    out = np.array(obs, F32, copy=True)
    rows = np.nonzero(np.asarray(rank) >= 0)[0]
    src = rows if row_map is None else np.asarray(row_map)[rows]
    cols = L.ctrl_idx if what == GM_RECORDED_CONTROL else L.cart_idx
    last = out[-1]
    last[np.ix_(rows, cols)] = np.asarray(frame, F32)[np.ix_(src, cols)]
    return out


# ------------------------------------------------------------------------------------------ the recorded loop
def recorded_loop(predict, obs0, frames, L, rigid, steps):
    """compute_rollout's ground-truth loop (rollout_utils.py:38-61): predict(window) -> (next xyz [N, 3], normalised acceleration
    [N, 3]).  Returns (final window, records [steps, N, D], predictions [steps, N, 3]).  Step i reads frames[i] twice: its control
    columns before the step (:45), its xyz after it (:60) -- the pose lags the window by one step."""
    cur = np.array(obs0, F32, copy=True)
    ci = L.cart_idx
    recs, preds = [], []
    for i in range(steps):
        gt = np.asarray(frames[i], F32)
        if L.ctrl >= 0:
            new = cur[-1][rigid]
            new[:, L.ctrl_idx] = gt[rigid][:, L.ctrl_idx]
            cur[-1][rigid] = new
        recs.append(cur[-1].copy())
        nxt, acc = predict(cur)
        preds.append(np.asarray(acc, F32))
        new_rigid = cur[-1][rigid].copy()
        cur[:-1] = cur[1:].copy()
        cur[-1][:, ci] = nxt                      # every row, rigid ones included (:51-54)
        new_rigid[:, ci] = gt[rigid][:, ci]
        cur[-1][rigid] = new_rigid
    return cur, np.stack(recs), np.stack(preds)


def oracle_predict(params, L, num_layers, m_steps, stats=STATS, bounds=None, r=R):
    """The float32 oracle's step: features, radius graph, forward, integration."""
    from conftest import BOUNDS
    bounds = BOUNDS if bounds is None else bounds

    def predict(cur):
        nodes, ea, s, rcv, _ = orc.process(cur, None, stats, bounds, r, L.cart_idx, [L.mat], L.ctrl_idx)
        acc = orc.epd_forward(params, nodes, ea, np.stack((s, rcv)), num_layers, m_steps)
        return orc.get_position_from_prediction(stats, L.cart_idx, acc, cur), acc
    return predict


# ------------------------------------------------------------------------------------------ recordings
class Recording:
    """A synthetic recorded simulation in the layout `name` ('default' or 'no_control'): sim [T, n, D] float32."""

    def __init__(self, name, n, T, seed, rigid_frac=0.1, side=0.05):
        self.name, self.L, self.n, self.T = name, wc.LAYOUTS[name], n, T
        L = self.L
        assert (L.cart, L.mat) == (2, 1) and L.ctrl in (-1, 5)          # make_scene's own columns
        base = scene.make_scene(n, seed=seed, k=T, rigid_frac=rigid_frac, side=side)
        sim = np.ascontiguousarray(base[:, :, :L.D])
        if L.ctrl >= 0:                                                   # coffee_dataset.py:91-97: the way to the next frame, rigid rows only
            rigid = sim[0, :, L.mat] == 1
            sim[:-1, :, L.ctrl:L.ctrl + 3] = np.where(rigid[None, :, None], sim[1:, :, 2:5] - sim[:-1, :, 2:5], F32(0))
        self.sim = sim
        self.sim.setflags(write=False)

    @property
    def rigid(self):
        return self.sim[0, :, self.L.mat] == 1

    @property
    def coffee(self):
        return self.sim[0, :, self.L.mat] == 0

    def window(self):
        return np.array(self.sim[:self.L.k])

    def frames(self, steps):
        k = self.L.k
        return np.array(self.sim[k - 1:k - 1 + steps])


FUSED_N, FUSED_STEPS = 301, 4                # one launch of two workgroups, neither full
FUSED_MODELS = {"systolic": (128, 2, 2), "streamed": (64, 2, 2)}      # (hidden, num_layers, m_steps)
FUSED_CASES = [("default", "systolic"), ("default", "streamed"), ("no_control", "systolic")]
RENUMBER_STEPS, RENUMBER_EVERY = 5, 2
RENUMBER_BAR = 2e-6                          # of the frame's largest coordinate: the bar of the renumbering tests of gm_rollout


def fused_recording(name, c=0):
    """Mixed scene: a tenth of the rows rigid, the rest granular; c: the simulation of a batch."""
    return Recording(name, FUSED_N, wc.LAYOUTS[name].k + RENUMBER_STEPS + 1, 900 + c)


def model_params(L, hidden, num_layers, m_steps, seed=870):
    """Random weights with a damped decoder: the rollout stays a scene."""
    dims = (L.node_dim, 4, 3, hidden, num_layers, m_steps)
    params = orc.init_params(*dims, seed)
    params[f"decoder.{2 * num_layers}.weight"] = params[f"decoder.{2 * num_layers}.weight"] * F32(1e-2)
    return dims, params


def frames_are_tie_free(rec, steps):
    """The radius graph of every frame a loop of `steps` steps can see is free of distance ties (a tie falls back on the row
    index, which renumbering changes)."""
    k = rec.L.k
    return all(orc.connectivity_is_tie_free(rec.sim[t][:, rec.L.cart_idx], R, K_NB) for t in range(k - 1, k - 1 + steps))


# ------------------------------------------------------------------------------------------ the error sums
ERR_ROWS = (1, 63, 64, 65, 257, 1000)
ERR_GRAPHS = (1, 3)
ERR_STEPS = (1, 5)
ERR_CASES = [(rows, g, steps) for rows in ERR_ROWS for g in ERR_GRAPHS for steps in ERR_STEPS]
ERR_L = wc.LAYOUTS["default"]


def error_inputs(rows, graphs, steps, coffee=True, seed=0):
    """(record_last [steps, N, D], record_pred [steps, N, 3], sim [steps + 3, N, D], first_frame = 1): seeded positions in the
    unit box, records a small way off them; material 0 / 1 / 2 on seeded rows (coffee=False: 1 / 2 only)."""
    L, n, T = ERR_L, rows * graphs, steps + 3
    rng = np.random.default_rng(7000 + 10 * rows + 3 * graphs + steps + seed)
    sim = rng.standard_normal((T, n, L.D)).astype(F32)
    p0 = 0.2 + 0.6 * rng.random((n, 3))
    for t in range(T):
        sim[t, :, L.cart_idx] = (p0 + 1e-3 * t + 2e-4 * rng.standard_normal((n, 3))).astype(F32).T
    mat = rng.integers(0, 3, n).astype(F32)
    if not coffee:
        mat[mat == 0] = 2.0
    sim[:, :, L.mat] = mat
    rec = sim[1:1 + steps].copy()
    rec[:, :, L.cart_idx] += (1e-3 * rng.standard_normal((steps, n, 3))).astype(F32)
    pred = rng.standard_normal((steps, n, 3)).astype(F32)
    return rec, pred, sim, 1


def acceleration_target(sim, f, L, stats=STATS):
    """float64 [N, 3]: ((p[f+1] - 2 p[f] + p[f-1]) - acc_mean) / acc_std, statistics as the float32 the descriptor carries."""
    p = lambda t: np.asarray(sim[t], F32)[:, L.cart_idx].astype(F64)
    am = np.asarray(stats["acceleration_mean"], F32).astype(F64)
    sd = np.asarray(stats["acceleration_std"], F32).astype(F64)
    return (((p(f + 1) - 2.0 * p(f)) + p(f - 1)) - am) / sd


def error_sums(rec, pred, sim, first, steps, n_per, L, stats=STATS):
    """gm_rollout_errors in float64 numpy: [steps, G, 4]."""
    n = rec.shape[1]
    G = n // n_per
    out = np.zeros((steps, G, 4), F64)
    for i in range(steps):
        gt = np.asarray(sim[first + i], F32)
        d = np.asarray(rec[i], F32)[:, L.cart_idx].astype(F64) - gt[:, L.cart_idx].astype(F64)
        e = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        coffee = gt[:, L.mat] == 0
        ea = np.zeros(n, F64)
        if pred is not None:
            da = np.asarray(pred[i], F32).astype(F64) - acceleration_target(sim, first + i, L, stats)
            ea = (da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2]
        for g in range(G):
            rows = slice(g * n_per, (g + 1) * n_per)
            c = coffee[rows]
            out[i, g] = (e[rows].sum(), e[rows][c].sum(), ea[rows][c].sum(), c.sum())
    return out


def rmse_from_sums(sums, n_rows):
    """(rmse_position, rmse_position_coffee, rmse_acceleration) of one simulation from its [steps, 4] sums -- the engine's own,
    unpinned definition: sqrt(sum over steps and rows of |delta|^2 / (steps * rows))."""
    sums = np.asarray(sums, F64)
    steps = sums.shape[0]
    tot = sums.sum(axis=0)
    cnt = sums[0, 3]
    div = lambda v, rows: float(np.sqrt(v / (steps * rows))) if steps * rows > 0 else float("nan")
    return div(tot[0], n_rows), div(tot[1], cnt), div(tot[2], cnt)
