"""Cases and the numpy restatement of the fp16 single-product inference mode (``set_precision("f16")``) -- a plain helper module shared
by test_precision_cases.py (CPU) and test_gpu_precision.py (GPU).

The mode's contract (include/gnn_manip_hip.h, "Numeric domain of the fp16 mode"): every Linear multiplies its weights and its inputs
rounded to fp16 (round to nearest even) and accumulates the exact products in float32; biases, LayerNorm, residuals, the scatter-add
and the latents stay float32.  The kernels hold their operands at power-of-two scales and round them there.  A power of two
commutes with the rounding as long as the value is an fp16 normal (>= 2^-14) at both scales, so on operands of ordinary magnitude
this is "round each Linear's weight matrix and input to fp16, multiply exactly" -- what ``mlp`` below does by default.  Where an
operand is below 2^-14 at one of the two scales it is not: raw feature rows or first-Linear weights of magnitude 1e-4, entries 2^20
below their row's maximum.  ``round_first`` and ``weight_scale`` then say at which scale the kernels round
(f16_rollout_cases.raw_rounding restates the scales; on standard-normal rows and the weights of ``init_params`` the two
restatements are 1e-6 apart at the most, test_f16_rollout_cases.py).  Two details of the kernels are visible at the mode's precision:
  * the Linear in front of a LayerNorm is packed centred over its outputs (W - mean_rows(W), b - mean(b), float32, the pack
    kernels' summation order -- after the coarse part of the mean, which is zero unless the mean exceeds the entries' spread, has
    been taken off unrounded: csrc/mlp.h, coarse_mean), and it is the CENTRED matrix that is rounded;
  * the LayerNorm behind it takes the mean square of those outputs as their variance and subtracts no mean (csrc/hmlp.hip:
    ln_merge) -- exact for the centred float32 weights, off by the mean of the rounding errors (about 3e-5 of the outputs' rms) for
    the rounded ones.
The concatenations of the processor MLPs ([h_i, h_j, e], [h, agg]) are rounded per block, which is the same thing.

Accumulation is float64, or float32 on request: the distance between the two (``rel_rms``) is the scale of what an evaluation
order may change, and the bar of the tight GPU checks is taken from it, per case.  Variants with only the weights / only the
inputs rounded, and the exact float64 forward, say how far the contract is from its neighbours.

Pure numpy (PCG64): a seed gives the same case on every machine."""
import functools

import numpy as np

from oracle import epd_oracle as orc

F32, F64 = np.float32, np.float64
NODE_DIM, EDGE_DIM, OUT_DIM = 25, 4, 3
EPS = 1e-5


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def r16(a):
    """Round to nearest even to fp16, as v_cvt_pk_f16_f32 does on the float32 value the kernels hold; returned in float64."""
    with np.errstate(over="ignore"):   # |x| >= 65520 rounds to +-inf, as in the kernels
        return np.asarray(a).astype(F32).astype(np.float16).astype(F64)


def coarse_mean(x):
    """csrc/mlp.h: per column of x, the multiple of g nearest to the mean, g the power of two with 2 s < g <= 4 s, s the largest
    deviation from the mean; s = 0: the mean itself.  float32, zero for entries whose mean is below their spread."""
    x = np.asarray(x, F32).astype(F64)
    m = np.zeros(x.shape[1:], F64)
    for row in x:
        m = m + row
    m = m / x.shape[0]
    s = np.abs((x - m).astype(F32)).max(axis=0)
    g = np.ldexp(1.0, np.frexp(np.where(s > 0, s, 1).astype(F32))[1] + 1)
    return np.where(s > 0, np.rint(m / g) * g, m).astype(F32)


def centred(w, b):
    """(W - mean_rows(W), b - mean(b)) as pack_hm_kernel / pack_h3_kernel form them: the coarse mean taken off (float64 subtraction,
    rounded to float32 once), then the float32 mean of what is left, summed output after output."""
    w, b = np.asarray(w, F32), np.asarray(b, F32)
    w = (w.astype(F64) - coarse_mean(w).astype(F64)).astype(F32)
    b = (b.astype(F64) - coarse_mean(b[:, None]).astype(F64)).astype(F32)
    cm = np.zeros(w.shape[1], F32)
    for o in range(w.shape[0]):
        cm = cm + w[o]
    cm = cm / F32(w.shape[0])
    bm = F32(0)
    for o in range(b.shape[0]):
        bm = F32(bm + b[o])
    bm = F32(bm / F32(b.shape[0]))
    return w - cm, b - bm


def mlp(p, prefix, blocks, num_layers, norm, acc=F64, round_w=True, round_x=True, ln_eps=EPS, round_first=None, weight_scale=None):
    """One MLP of the model on the concatenation of `blocks`: Linear ReLU [Linear ReLU] x (L - 1) Linear [LayerNorm].
    round_w / round_x: round the weights / the inputs of every Linear to fp16 (both: the mode; neither: the float32 path's
    function in float64).  acc: the dtype the products are accumulated -- and everything behind them computed -- in.  ln_eps: the eps
    of the LayerNorm (the callers below pass it on in **kw).  round_first: the rounding of the first Linear's input where it is not
    r16 on the value as it stands (f16_rollout_cases.round_rows: the encoders round a raw feature row at its own scale).
    weight_scale: per Linear, the power of two its weights are multiplied by before they are rounded (f16_rollout_cases.encoder_scales;
    default: rounded as they stand -- the same thing unless entries are below 2^-14 at one of the two scales)."""
    x = np.concatenate([np.asarray(b, F64) for b in blocks], axis=1)
    for l in range(num_layers + 1):
        w, b = p[f"{prefix}.{2 * l}.weight"], p[f"{prefix}.{2 * l}.bias"]
        if norm and l == num_layers:
            w, b = centred(w, b)
        t = 1.0 if weight_scale is None else float(weight_scale[l])
        w = r16(np.asarray(w, F32) * F32(t)) / t if round_w else np.asarray(w, F64)
        xin = (round_first(x) if l == 0 and round_first is not None else r16(x)) if round_x else x
        z = xin.astype(acc) @ w.astype(acc).T + np.asarray(b, acc)
        x = np.maximum(z, 0) if l < num_layers else z
        x = x.astype(F64) if acc is F64 else x.astype(F32).astype(F64)
    if norm:
        g, bt = p[f"{prefix}.{2 * num_layers + 1}.weight"], p[f"{prefix}.{2 * num_layers + 1}.bias"]
        z = x.astype(acc)
        k = 1.0 / np.sqrt((z * z).mean(axis=1, keepdims=True, dtype=acc) + acc(ln_eps))
        x = ((z * k) * np.asarray(g, acc) + np.asarray(bt, acc)).astype(F64)
    return x


def graph_independent(p, prefix, nodes, edge_attr, num_layers, enc_node=None, enc_edge=None, **kw):
    """enc_node / enc_edge: keywords of `mlp` that hold for that one MLP alone, over those of **kw."""
    return (mlp(p, f"{prefix}.phi_node", [nodes], num_layers, True, **{**kw, **(enc_node or {})}),
            mlp(p, f"{prefix}.phi_edge", [edge_attr], num_layers, True, **{**kw, **(enc_edge or {})}))


def interaction_network(p, prefix, h, e, edge_index, num_layers, **kw):
    """(h', e') of the block, no residual: j = edge_index[0], i = edge_index[1]; agg_i = sum of e' over the edges into i."""
    j, i = np.asarray(edge_index[0]), np.asarray(edge_index[1])
    e_new = mlp(p, f"{prefix}.phi_edge", [h[i], h[j], e], num_layers, True, **kw)
    agg = np.zeros_like(np.asarray(h, F64))
    np.add.at(agg, i, e_new)
    h_new = mlp(p, f"{prefix}.phi_node", [h, agg], num_layers, True, **kw)
    return h_new, e_new


def epd_forward(p, nodes, edge_attr, edge_index, num_layers, m_steps, enc_node=None, enc_edge=None, **kw):
    h, e = graph_independent(p, "encoder", nodes, edge_attr, num_layers, enc_node, enc_edge, **kw)
    for k in range(m_steps):
        hn, en = interaction_network(p, f"processor.{k}", h, e, edge_index, num_layers, **kw)
        h, e = h + hn, e + en
    return mlp(p, "decoder", [h], num_layers, False, **kw)


def exact(fn, *args):
    """`fn` with nothing rounded, float64: what the float32 mode computes to 1e-6."""
    return fn(*args, round_w=False, round_x=False)


def rel_rms(a, ref):
    """rms of a - ref over all elements, divided by the rms of ref."""
    a, ref = np.asarray(a, F64), np.asarray(ref, F64)
    return float(np.sqrt(np.mean((a - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def max_err(a, ref, floor=0.0):
    """max |a - ref| / max(max |ref|, floor)."""
    a, ref = np.asarray(a, F64), np.asarray(ref, F64)
    return float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), floor))


# ------------------------------------------------------------------------------------------ A: one MLP deep
A_N, A_E = 300, 1000
A_CASES = [(hidden, nl) for hidden in (64, 128, 256, 100) for nl in (2, 3)]


def a_seed(hidden, nl):
    return 9000 + 10 * hidden + nl


@functools.lru_cache(maxsize=None)
def a_params(hidden, nl):
    return orc.init_params(NODE_DIM, EDGE_DIM, OUT_DIM, hidden, nl, 1, a_seed(hidden, nl))


@functools.lru_cache(maxsize=None)
def a_inputs(hidden, nl):
    """(nodes [N, 25], edge_attr [E, 4], h [N, hidden], e [E, hidden], edge_index [2, E]): seeded standard normal rows, random
    edges."""
    rng = _rng(a_seed(hidden, nl) + 1)
    nodes = rng.standard_normal((A_N, NODE_DIM)).astype(F32)
    ea = rng.standard_normal((A_E, EDGE_DIM)).astype(F32)
    h = rng.standard_normal((A_N, hidden)).astype(F32)
    e = rng.standard_normal((A_E, hidden)).astype(F32)
    ei = rng.integers(0, A_N, (2, A_E)).astype(np.int64)
    return nodes, ea, h, e, ei


A_OUTPUTS = ("encoder_h", "encoder_e", "block_e")


def a_restate(hidden, nl, **kw):
    """{output name: array}: both outputs of the encoder block and e' of the processor block, one MLP deep each."""
    p = a_params(hidden, nl)
    nodes, ea, h, e, ei = a_inputs(hidden, nl)
    eh, ee = graph_independent(p, "encoder", nodes, ea, nl, **kw)
    be = mlp(p, "processor.0.phi_edge", [h[ei[1]], h[ei[0]], e], nl, True, **kw)
    return {"encoder_h": eh, "encoder_e": ee, "block_e": be}


@functools.lru_cache(maxsize=None)
def a_reference(hidden, nl):
    """(restatement with float64 accumulation, g): g[name] = rel_rms between the float32- and the float64-accumulating
    restatement -- the scale of what a summation order changes.  The bar of check A is 3 g."""
    r64 = a_restate(hidden, nl)
    r32 = a_restate(hidden, nl, acc=F32)
    for v in r64.values():
        v.setflags(write=False)
    return r64, {k: rel_rms(r32[k], r64[k]) for k in r64}


# ------------------------------------------------------------------------------------------ B: whole forward
B_FLOOR = 1e-3
SYS_DIMS = (NODE_DIM, EDGE_DIM, OUT_DIM, 128, 2, 3)
# (name, n nodes, edges, hub in-degree): the shapes of tests/test_gpu_edge_ticks.py
SYS_GRAPHS = [("e1", 40, 1, 0), ("e33", 40, 33, 0), ("e129", 40, 129, 0), ("e513", 40, 4 * 128 + 1, 0),
              ("257_groups", 2000, 128 * 256 + 1, 0), ("hub", 600, 4000, 200)]
# (name, hidden, num_layers, m_steps, n nodes, edges): the streamed kernels; the last lies just past launch_node_h's switch to the
# four-block form (4 blocks of 32 rows per workgroup x 256 workgroups = 32768 nodes at hidden 128)
HM_CASES = [("h64_l3", 64, 3, 2, 300, 1000), ("h256_l2", 256, 2, 2, 300, 1000), ("h128_l3", 128, 3, 2, 300, 1000),
            ("four_block", 128, 3, 2, 33000, 100000)]


def random_graph(n, e, seed, hub=0):
    """n nodes, e random edges; hub > 0: the first `hub` edges all arrive at node n // 2."""
    rng = _rng(seed)
    nodes = rng.standard_normal((n, NODE_DIM)).astype(F32)
    ea = rng.standard_normal((e, EDGE_DIM)).astype(F32)
    ei = rng.integers(0, n, (2, e)).astype(np.int64)
    ei[1, :hub] = n // 2
    return nodes, ea, ei


@functools.lru_cache(maxsize=None)
def sys_params():
    return orc.init_params(*SYS_DIMS, 128)


@functools.lru_cache(maxsize=None)
def sys_case(name):
    _, n, e, hub = next(c for c in SYS_GRAPHS if c[0] == name)
    return random_graph(n, e, 7000 + n + e, hub)


@functools.lru_cache(maxsize=None)
def hm_params(name):
    _, hidden, nl, ms, _, _ = next(c for c in HM_CASES if c[0] == name)
    return orc.init_params(NODE_DIM, EDGE_DIM, OUT_DIM, hidden, nl, ms, 8000 + hidden + nl)


@functools.lru_cache(maxsize=None)
def hm_case(name):
    _, _, _, _, n, e = next(c for c in HM_CASES if c[0] == name)
    return random_graph(n, e, 8500 + n)


def b_reference(params, nodes, ea, ei, nl, ms, ln_eps=EPS, **kw):
    """(float64 forward of oracle/torch_epd.py, err of the restatement against it): the envelope of check B is err / 4 .. 4 err.
    **kw: keywords of `epd_forward` (a variant of the restatement)."""
    import torch
    from oracle import torch_epd
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    with torch.no_grad():
        ref = torch_epd.epd_forward(p, torch.tensor(nodes, dtype=torch.float64), torch.tensor(ea, dtype=torch.float64),
                                    torch.tensor(ei, dtype=torch.int64), nl, ms, ln_eps).numpy()
    rest = epd_forward(params, nodes, ea, ei, nl, ms, ln_eps=ln_eps, **kw)
    return ref, max_err(rest, ref, B_FLOOR)


@functools.lru_cache(maxsize=None)
def sys_reference(name):
    """b_reference of a systolic case: computed once, shared by the tests that need it, never written to."""
    ref, err = b_reference(sys_params(), *sys_case(name), SYS_DIMS[4], SYS_DIMS[5])
    ref.setflags(write=False)
    return ref, err


@functools.lru_cache(maxsize=None)
def hm_reference(name):
    _, _, nl, ms, _, _ = next(c for c in HM_CASES if c[0] == name)
    ref, err = b_reference(hm_params(name), *hm_case(name), nl, ms)
    ref.setflags(write=False)
    return ref, err
