"""Cases and references that hold the fp16 mode (``set_precision("f16")``) to float64 on the routes a ROLLOUT takes -- a plain helper
module (no test) of test_f16_rollout_cases.py (CPU: every case is in the regime it was built for, and the references tell right
from wrong) and test_gpu_f16_rollout.py (GPU).  The restatement of the mode is precision_cases' (``pc.epd_forward``), the
integrator, the radius graph and the Sinkhorn loss are the oracle's (oracle/epd_oracle.py); nothing of either is copied here.

  sorted     gm_epd_forward on edge attributes in the csr's order (the only route to the systolic edge encoder): layernorm_cases'
             sorted scene and precision_cases' tick-boundary graphs stable-sorted by destination (the library's sort keeps the edges
             of a destination in the order they came in, so such an input is in the csr's order already)
  step       one rollout step from a GIVEN window (the device's own, teacher-forced): the oracle's step with a forward that records
             the features it was given, then rule B of precision_cases on those features
  compound   a whole rollout: the oracle's loop with the exact float64 forward and with the restatement as its forward; d = the
             largest deviation of a sand row's end position from the float64 rollout's, over the largest displacement of a sand row
  ranking    six candidate trajectories of one scene, the float64 Sinkhorn loss of where the sand ends up, and the pairs of
             candidates that the restatement's own noise leaves decided
  raw rows   the encoders' input rounding as the kernels do it (``round_rows``), where it differs from rounding the unscaled value

"Exact float64 forward" is ``pc.exact(pc.epd_forward, ...)`` in the rollouts (numpy) and oracle/torch_epd.py in rule B
(``pc.b_reference``); test_precision_cases.py holds the two to 1e-6 of each other.  oracle.epd_forward itself is float32.  The oracle's
integrator and state are float32 in every rollout here, as on the device: what is compared is the forward's arithmetic.

The encoders' operand rounding (csrc/hmlp.hip: narrow_rows_to_image, pack_hm_kernel; csrc/hedge.hip: sys_enc_kernel,
pack_h3_kernel).  A raw feature row is multiplied by a power of two s that brings its largest magnitude into [2^6, 2^7), s at most
`cap`, and THEN rounded to fp16 (an all-zero row takes the cap); Linear l's weights are rounded as t_l W_l, t_l the power of two the
pack kernels derive from the weights' norms.  fp16 has 11 significant bits down to 2^-14 and a fixed spacing of 2^-24 below, so
this is the rounding of the unscaled value (``pc.r16``) only while neither the unscaled nor the scaled value is below 2^-14:
  * a row of magnitude below 2^-14 loses bits rounded as it stands (all of them from 2^-25 down) and none at the kernels' scale;
    the same holds for first-Linear weights of that magnitude (raw features times 1e3 under weights divided by 1e3)
  * an entry more than 2^20 below its row's maximum is subnormal at the kernels' scale and keeps about 31 - k bits at 2^-k of the
    maximum; under a maximum of order 1 it is far below 2^-14 as it stands, where r16 keeps fewer still.
``encoder_scales`` restates t_l and the cap (no row scale may push a bias, in the accumulators' units U_l s b, beyond 4096) in
float64.  They are powers of two taken from float32 sums, which a summation order could move by a factor 2 at a boundary: a t_l
off by 2 changes the rounding of weights within a factor 2 of 2^-14 only, and every case here keeps its non-zero rows a factor 2
or more below the cap (test_f16_rollout_cases.py), so the cap decides no bit of any case.  Where the cap holds a row of tiny
magnitude down, the kernels' rounding is the coarser one; no case is built for that.

Pure numpy (PCG64): a seed gives the same case on every machine."""
import functools

import numpy as np

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from gnn_manip_amd import scene
from oracle import epd_oracle as orc
import layernorm_cases as lc
import precision_cases as pc
import width_cases as wc

F32, F64 = np.float32, np.float64
L = wc.LAYOUTS["default"]
R, K_NB = 0.015, 20
NL, MS = 2, 2
TARGET_RMS, RAW_RMS = 16.0, 32.0           # csrc/hmlp.h: kHmTargetRms, kHmRawInputRms


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


# ------------------------------------------------------------------------------------------ raw rows at the kernels' scale
def _pow2_floor(x):
    return float(np.ldexp(1.0, np.frexp(x)[1] - 1))


def _pow2_near(x):
    f, ex = np.frexp(x)
    return float(np.ldexp(1.0, ex if f >= 0.70710678 else ex - 1))


def encoder_scales(p, prefix, nl):
    """([t_l], cap) of an encoder MLP as the pack kernels choose them.  m: the estimated rms of the activations (raw rows enter at
    RAW_RMS; a layer maps m to gain m, gain^2 = |W|_F^2 / outputs / 2), U_l: the power of two nearest TARGET_RMS / m_l, t_l = U_l /
    U_(l-1) -- the scale Linear l's weights are rounded at -- held where max |W_l| t_l stays in [2^-4, 2^13]; the cap is the smallest
    over the layers of the power of two at or below 4096 / (U_l max |b_l|).  The Linear in front of the LayerNorm counts centred."""
    m, U, cap, ts = RAW_RMS, 1.0, 1.0e18, []
    for l in range(nl + 1):
        w, b = p[f"{prefix}.{2 * l}.weight"], p[f"{prefix}.{2 * l}.bias"]
        if l == nl:
            w, b = pc.centred(w, b)
        w, b = np.asarray(w, F64), np.asarray(b, F64)
        m = float(np.sqrt((w * w).sum() / w.shape[0] * 0.5) * m)
        t = _pow2_near(TARGET_RMS / m) / U
        wm = float(np.abs(w).max())
        if wm * t > 8192.0:
            t = _pow2_floor(8192.0 / wm)
        if wm * t < 0.0625:
            t = 2.0 * _pow2_floor(0.0625 / wm)
        U *= t
        ts.append(t)
        if np.abs(b).max() > 0:
            cap = min(cap, _pow2_floor(4096.0 / (U * float(np.abs(b).max()))))
    return ts, cap


def row_cap(p, prefix, nl):
    return encoder_scales(p, prefix, nl)[1]


def row_scale(x, cap=np.inf):
    """[rows, 1]: the power of two of each row -- largest magnitude into [2^6, 2^7), `cap` at the most; an all-zero row: the cap."""
    mx = np.abs(np.asarray(x, F32).astype(F64)).max(axis=1, keepdims=True)
    ex = np.frexp(np.where(mx > 0, mx, 1.0))[1]
    return np.where(mx > 0, np.minimum(np.ldexp(1.0, np.minimum(7 - ex, 100)), cap), min(cap, 2.0 ** 100))


def round_rows(x, cap=np.inf):
    """The rows of x rounded to fp16 at the kernels' scale, scaled back; float64."""
    s = row_scale(x, cap)
    return pc.r16(np.asarray(x, F32).astype(F64) * s) / s


def raw_rounding(p, nl=NL):
    """The keywords that make ``pc.epd_forward`` / ``pc.graph_independent`` round the encoders' operands as the kernels do: the raw
    rows at their own scale, the weights at the scale they are packed at."""
    def of(prefix):
        ts, cap = encoder_scales(p, prefix, nl)
        return dict(round_first=functools.partial(round_rows, cap=cap), weight_scale=ts)
    return dict(enc_node=of("encoder.phi_node"), enc_edge=of("encoder.phi_edge"))


# the wrong variant of "done when" 3: everything rounded but the edge encoder (its inputs and its weights)
EDGE_ENCODER_UNROUNDED = dict(enc_edge=dict(round_w=False, round_x=False))

RAW_HIDDEN = (128, 100)
RAW_CASES = ("scene", "scene_x1e-4", "scene_x1e3", "wide")
WIDE_ROWS = 64
WIDE_DEPTHS = (8, 16, 22, 26)              # rows 4 i + j, i < 14: entries at 2^-WIDE_DEPTHS[j] of the row's maximum
WIDE_SINGLE = tuple(range(56, 60))         # one non-zero entry
WIDE_ZERO = tuple(range(60, 64))           # all zero


def raw_rows_by_depth(depth):
    return [4 * i + WIDE_DEPTHS.index(depth) for i in range(14)]


def _wide_block(dim, seed):
    """[64, dim]: column 0 holds the row's maximum (magnitude 1 .. 2), the other columns values of magnitude 0.5 .. 1 times
    2^-depth; then the rows with a single entry (in a column that moves with the row) and the zero rows."""
    rng = _rng(seed)
    x = rng.uniform(0.5, 1.0, (WIDE_ROWS, dim)) * rng.choice((-1.0, 1.0), (WIDE_ROWS, dim))
    x[:, 0] = rng.uniform(1.0, 2.0, WIDE_ROWS) * rng.choice((-1.0, 1.0), WIDE_ROWS)
    for depth in WIDE_DEPTHS:
        x[raw_rows_by_depth(depth), 1:] *= 2.0 ** -depth
    for r in WIDE_SINGLE:
        x[r] = 0.0
        x[r, 1 + r % (dim - 1)] = (-1.0) ** r * (0.37 + 0.1 * (r - WIDE_SINGLE[0]))
    x[list(WIDE_ZERO)] = 0.0
    return x.astype(F32)


@functools.lru_cache(maxsize=None)
def raw_case(hidden, name):
    """(parameters, nodes, edge_attr, edge_index) of a raw-row case at `hidden`: layernorm_cases' scene and plain weights as they
    are, with the features times 1e-4 / 1e3 and the first Linears divided by it (lc.feature_scaled), and "wide": the block above
    as both feature arrays (64 nodes, 64 edges in destination order) under the plain weights."""
    p = lc.case_params(hidden, NL, "plain-all-eps1e-05")
    nodes, ea, ei = lc.scene()
    if name == "wide":
        nodes, ea = _wide_block(pc.NODE_DIM, 71), _wide_block(pc.EDGE_DIM, 72)
        ei = _rng(73).integers(0, WIDE_ROWS, (2, WIDE_ROWS)).astype(np.int64)
        ei = ei[:, np.argsort(ei[1], kind="stable")]
    elif name != "scene":
        p, nodes, ea = lc.feature_scaled(p, nodes, ea, float(name[len("scene_x"):]))
    _frozen(nodes, ea, ei, *p.values())
    return p, nodes, ea, ei


RAW_OUTPUTS = ("encoder_h", "encoder_e")


def raw_restate(hidden, name, natural=False, **kw):
    """{output: array} of the encoder block on a raw-row case: the rows rounded at the kernels' scale, or (natural) as they stand."""
    p, nodes, ea, _ = raw_case(hidden, name)
    how = {} if natural else raw_rounding(p)
    h, e = pc.graph_independent(p, "encoder", nodes, ea, NL, how.get("enc_node"), how.get("enc_edge"), **kw)
    return {"encoder_h": h, "encoder_e": e}


@functools.lru_cache(maxsize=None)
def raw_reference(hidden, name):
    """(restatement at the kernels' scale with float64 accumulation, g) -- check A's: the bar is 3 g, g[output] the rel_rms between
    the float32- and the float64-accumulating restatement of THIS case."""
    r64, r32 = raw_restate(hidden, name), raw_restate(hidden, name, acc=F32)
    _frozen(*r64.values())
    return r64, {k: pc.rel_rms(r32[k], r64[k]) for k in r64}


def sorted_case(hidden, name):
    """A raw-row case with its edges in the csr's order (the scene's: lc.scene_sorted's permutation; "wide" is built sorted)."""
    p, nodes, ea, ei = raw_case(hidden, name)
    perm = np.lexsort((ei[0], ei[1]))
    return p, nodes, np.ascontiguousarray(ea[perm]), np.ascontiguousarray(ei[:, perm])


@functools.lru_cache(maxsize=None)
def raw_forward_reference(name):
    """Rule B of a raw-row case's whole forward at hidden 128: (float64 forward, err of the restatement at the kernels' scale, err
    of the restatement that rounds the rows as they stand)."""
    p, nodes, ea, ei = raw_case(128, name)
    ref, err = pc.b_reference(p, nodes, ea, ei, NL, lc.M_STEPS, **raw_rounding(p))
    ref.setflags(write=False)
    return ref, err, pc.max_err(pc.epd_forward(p, nodes, ea, ei, NL, lc.M_STEPS), ref, pc.B_FLOOR)


# ------------------------------------------------------------------------------------------ sorted attributes (part 1)
SORTED_KERNELS = ("sys", "sys_all")
SORTED_GRAPHS = ("scene", "e1", "e33", "e129", "e513", "hub")


@functools.lru_cache(maxsize=None)
def sorted_graph(name):
    """(parameters, dims, nodes, edge_attr, edge_index) with the edges in the csr's order."""
    if name == "scene":
        return (pc.sys_params(), pc.SYS_DIMS) + tuple(lc.scene_sorted())
    nodes, ea, ei = pc.sys_case(name)
    perm = np.argsort(ei[1], kind="stable")
    return (pc.sys_params(), pc.SYS_DIMS) + _frozen(nodes, np.ascontiguousarray(ea[perm]), np.ascontiguousarray(ei[:, perm]))


@functools.lru_cache(maxsize=None)
def sorted_reference(name, variant=False):
    """Rule B's (float64 forward, err of the restatement) -- precision_cases' own for the tick-boundary graphs: a prediction does not
    depend on the order of the edges.  variant: err of EDGE_ENCODER_UNROUNDED in place of the restatement's."""
    if name != "scene" and not variant:
        return pc.sys_reference(name)
    p, dims, nodes, ea, ei = sorted_graph(name)
    ref, err = pc.b_reference(p, nodes, ea, ei, dims[4], dims[5], **(EDGE_ENCODER_UNROUNDED if variant else {}))
    ref.setflags(write=False)
    return ref, err


# ------------------------------------------------------------------------------------------ scenes and models of the rollouts
# name -> (n, seed, side): 10 to 14 neighbours within R, the last tenth of the rows rigid.  The seeds are the best of 1300 (n300) and
# 3000 (n700) by the condition below: an 8-step rollout of a random scene usually has a pair nearer to the radius than the mode's
# noise moves it (at 700 nodes one seed in 3000 meets the condition)
SCENES = {"n300": (300, 842, 0.062), "n700": (700, 1857, 0.086)}
# In every frame a graph is built on, no edge is nearer to changing (graph_margins) than this many times the largest deviation of the
# restatement's own rollout in that frame
MARGIN = 1.0
STEPS = 4                                  # teacher-forced steps (part 2)
HORIZON = 8                                # compounding (part 3)
# name -> (hidden, set_edge_kernel)
STEP_MODELS = {"h128_hm": (128, "hm"), "h128_sys": (128, "sys"), "h128_sys_all": (128, "sys_all"), "h128_auto": (128, None),
               "h64_hm": (64, "hm"), "h256_hm": (256, "hm")}
COMPOUND_MODELS = ("h128_hm", "h128_sys", "h128_sys_all", "h128_auto")


def dims(hidden):
    return (pc.NODE_DIM, pc.EDGE_DIM, pc.OUT_DIM, hidden, NL, MS)


@functools.lru_cache(maxsize=None)
def params(hidden):
    """oracle.init_params, the decoder NOT damped: a prediction is of order 1, a step's acceleration of the order of its deviation
    (2.4e-4), and what the candidates of the ranking do to the sand stays above the mode's noise."""
    p = orc.init_params(*dims(hidden), 7100 + hidden)
    _frozen(*p.values())
    return p


@functools.lru_cache(maxsize=None)
def rollout_scene(name, steps=HORIZON):
    """(window [6, n, 8], trajectory [steps, n_rigid, 3])."""
    n, seed, side = SCENES[name]
    obs = scene.make_scene(n, seed=seed, k=L.k, side=side)
    return _frozen(obs, scene.rigid_drift_trajectory(obs, steps, seed=seed + 100, step_size=3e-4))


def sand_rows(obs):
    return obs[-1][:, MAT[0]] != 1


def oracle_step(p, window, target, forward):
    """One step of the oracle's rollout from `window` under the scripted pose `target` [n_rigid, 3]: (the state after it, the
    features and edges the forward was given)."""
    seen = {}

    def forward_fn(nodes, ea, ei):
        seen.update(nodes=nodes, ea=ea, ei=ei)
        return forward(nodes, ea, ei)

    after = orc.rollout(p, window, np.asarray(target)[None], 1, STATS, BOUNDS, R, CART, MAT, CTRL, NL, MS, K_NB, forward_fn=forward_fn)
    return after, seen


def exact_forward(p):
    return lambda nodes, ea, ei: pc.exact(pc.epd_forward, p, nodes, ea, ei, NL, MS)


def restated_forward(p, **kw):
    return lambda nodes, ea, ei: pc.epd_forward(p, nodes, ea, ei, NL, MS, **kw)


def step_reference(p, window, target, **kw):
    """Part 2's reference of one step from the device's own window: (float64 prediction on the step's features, err of the
    restatement on them -- rule B --, edge count, the features).  **kw: a variant of the restatement."""
    _, seen = oracle_step(p, window, target, lambda nodes, ea, ei: np.zeros((nodes.shape[0], pc.OUT_DIM), F32))
    ref, err = pc.b_reference(p, seen["nodes"], seen["ea"], seen["ei"], NL, MS, **kw)
    return ref, err, seen["ei"].shape[1], seen


def rollout_with(p, obs, traj, steps, forward):
    """The oracle's rollout step by step: (final state, [(positions the step's graph was built on, its edge_index)] per step)."""
    obs, frames = np.array(obs), []
    for s in range(steps):
        pos = obs[-1][:, CART].copy()      # the pre-step overwrite touches control columns only
        obs, seen = oracle_step(p, obs, traj[s], forward)
        frames.append((pos, seen["ei"]))
    return obs, frames


@functools.lru_cache(maxsize=None)
def compound_reference(scene_name, hidden=128, steps=HORIZON):
    """((end state, frames) of the float64 rollout, the same of the restatement's own rollout)."""
    obs, traj = rollout_scene(scene_name)
    p = params(hidden)
    r64 = rollout_with(p, obs, traj, steps, exact_forward(p))
    rr = rollout_with(p, obs, traj, steps, restated_forward(p))
    _frozen(r64[0], rr[0])
    return r64, rr


def end_deviation(end, end64, obs0):
    """max |x_end - x_end64| over the sand rows' coordinates, over the largest |x_end64 - x_0| of a sand row's coordinate."""
    sand = sand_rows(obs0)
    x, x64, x0 = (np.asarray(a, F64)[-1][sand][:, CART] for a in (end, end64, obs0))
    return float(np.abs(x - x64).max() / np.abs(x64 - x0).max())


def graph_margins(pos):
    """How far the radius graph of `pos` is from another edge set, float64 on the float32 positions: (the smallest | |x_i - x_j| - R |
    over the pairs, the smallest gap between the K_NB-th and the next neighbour's distance over the nodes with more than K_NB
    within R -- inf where the cap binds nowhere)."""
    x = np.asarray(pos, F64)
    d = np.sqrt(((x[:, None, :] - x[None, :, :]) ** 2).sum(-1))
    ds = np.sort(d, axis=1)                    # column 0: the node itself, which the graph counts among its K_NB
    capped = (d <= R).sum(axis=1) > K_NB
    rank = float((ds[capped, K_NB] - ds[capped, K_NB - 1]).min()) if capped.any() else float("inf")
    return float(np.abs(d - R).min()), rank


def edge_set(ei):
    return set(zip(ei[0].tolist(), ei[1].tolist()))


# ------------------------------------------------------------------------------------------ the ranking (part 4)
RANK_SCENE = "n300"
RANK_B, RANK_H = 6, 4
RANK_STEP_SIZES = tuple(float(2e-4 * 10 ** (c / 5)) for c in range(RANK_B))     # 2e-4 .. 2e-3: a decade
RANK_BLUR = 0.01
RANK_SHIFT = (0.003, -0.002, 0.002)        # the desired cloud: the sand's start moved by a few millimetres
RANK_KERNELS = ("sys_all", "hm")


@functools.lru_cache(maxsize=None)
def rank_case():
    """(window, trajectories [B, H, n_rigid, 3], desired cloud [n_sand, 3])."""
    obs, _ = rollout_scene(RANK_SCENE)
    trajs = np.stack([scene.rigid_drift_trajectory(obs, RANK_H, seed=300 + c, step_size=RANK_STEP_SIZES[c]) for c in range(RANK_B)])
    desired = (obs[-1][sand_rows(obs)][:, CART] + np.asarray(RANK_SHIFT, F32)).astype(F32)
    return (obs,) + _frozen(trajs, desired)


def rank_loss(end_state):
    """The float64 Sinkhorn loss of a final state's sand against the desired cloud."""
    obs, _, desired = rank_case()
    return orc.sinkhorn_divergence(np.asarray(end_state, F64)[-1][sand_rows(obs)][:, CART], desired.astype(F64), blur=RANK_BLUR)


@functools.lru_cache(maxsize=None)
def rank_reference():
    """(L64 [B], nu [B], decided pairs): the losses of the float64 rollouts, nu_c = |L(restatement's rollout of c) - L64_c|, and the
    pairs (i, j), i < j, with |L64_i - L64_j| > 4 (nu_i + nu_j)."""
    obs, trajs, _ = rank_case()
    p = params(128)
    l64 = np.array([rank_loss(rollout_with(p, obs, trajs[c], RANK_H, exact_forward(p))[0]) for c in range(RANK_B)])
    lr = np.array([rank_loss(rollout_with(p, obs, trajs[c], RANK_H, restated_forward(p))[0]) for c in range(RANK_B)])
    nu = np.abs(lr - l64)
    decided = [(i, j) for i in range(RANK_B) for j in range(i + 1, RANK_B) if abs(l64[i] - l64[j]) > 4 * (nu[i] + nu[j])]
    _frozen(l64, nu)
    return l64, nu, decided


def rank_table(name, losses):
    """The per-pair table of a set of losses against the reference: the lines, and the decided pairs it orders the other way."""
    l64, nu, decided = rank_reference()
    lines, wrong = [], []
    for i in range(RANK_B):
        for j in range(i + 1, RANK_B):
            same = (losses[i] < losses[j]) == (l64[i] < l64[j])
            is_decided = (i, j) in decided
            lines.append(f"[ranking] {name} pair ({i}, {j}): L64 gap {l64[i] - l64[j]:+.3e}, 4 (nu_i + nu_j) {4 * (nu[i] + nu[j]):.3e}, "
                         f"{'decided' if is_decided else 'open'}; its gap {losses[i] - losses[j]:+.3e} {'agrees' if same else 'DIFFERS'}")
            if is_decided and not same:
                wrong.append((i, j))
    return lines, wrong
