"""Cases in which a LayerNorm's eps and the centring of the Linear in front of it decide the answer -- a plain helper module (no
test) of tests/test_layernorm_cases.py (CPU: the references against torch, the regimes' own figures, the table's power) and
tests/test_gpu_layernorm.py (every LayerNorm implementation of the library against float64 on these cases).

The scene is the small one of train_step_cases (N = 300, 5362 edges), the model (25, 4, 3, hidden, num_layers, 2).  Every
regime is oracle.init_params with float32 edits of the Linear in front of a LayerNorm (Sequential index 2 * num_layers), applied to
one group of MLPs (TARGETS) at a time and to all of them:

  regime      edit                          variance entering the edited LayerNorms / eps (float64, hidden 128, num_layers 2, target
                                            "all": min .. median .. max over the rows of all the edited MLPs)
  plain       none                          eps 1e-5: 4.5e2 .. 1.9e3 .. 3.8e5  (eps is a correction of 1e-3 at the most; leaving
                                            it out moves the prediction by 4.6e-4 of its maximum)
                                            eps 1e-2: 0.45 .. 1.0 .. 2.4e2;  eps 1.0: 3.5e-3 .. 3.6e-3 .. 7.3e-2
  shrunk(k)   (W3, b3) * 2^-k               the plain ratio times 2^-2k:
                                            k = 7:  2.4e-2 .. 3.1e-2 .. 1.3: the variance is about eps on the processors' node MLPs
                                                    (6.4e-1 .. 7.3 .. 23) and 3 to 13 percent of it on the encoders and the edge
                                                    MLPs; either way the output is a function of eps
                                            k = 10: 3.1e-4 .. 3.4e-4 .. 5.6e-3  (at most 0.42, processor node MLPs): eps dominates
                                            k = 14: 1.2e-6 .. 1.4e-6 .. 2.3e-5: the output is z / sqrt(eps)
                                            k = 14 at eps = 1e-12: 17 .. 69 .. 1.4e4 -- exactly the plain weights at eps = 2^28 * 1e-12
                                                    = 2.7e-4 (a power of two commutes with every rounding): scale invariance at tiny
                                                    magnitudes, where v_rsq_f32 sees arguments near 1e-11
  offset(c)   b3 += c, W3 += c / fan_in     as plain (a column-constant shift, which a LayerNorm removes); the mean to remove is about
                                            c (1 + sum of the activations / fan_in): 8 or 256 against a standard deviation of
                                            0.07 .. 2
  flat(c)     W3 = 0, b3 = c                exactly 0: the output is the LayerNorm's bias (plus the residual)

(test_layernorm_cases.py prints these figures for every case and bounds them.)

The forward bar of the GPU test is max(1e-5, 4 e32) of max |ref64|, e32 the error of torch float32 against torch float64 on the same
case.  Hidden 128, num_layers 2: e32 = 1.2e-7 .. 1.0e-6 on every plain, shrunk and flat case (bar 1e-5).  On offset(8) e32 =
1.2e-6 .. 1.0e-5; the e32 term passes 1e-5 on offset8-enc_node (e32 9.0e-6, bar 3.6e-5) and offset8-all (1.0e-5, bar 4.0e-5).  On
offset(256) it decides every case: e32 = 3.0e-5 (enc_edge, bar 1.2e-4), 2.8e-4 (enc_node, 1.1e-3), 6.8e-5 (proc_edge, 2.7e-4),
5.7e-5 (proc_node, 2.3e-4), 2.7e-4 (all, 1.1e-3).  float32 loses c / sigma ulps where it subtracts the mean of c + z; the library
takes the coarse part of the mean off the weights, unrounded, when it packs them (csrc/mlp.h: coarse_mean) -- with the float32
mean alone, the restatement of the packed form (precision_cases.mlp, nothing rounded) missed the bar on offset256-enc_edge (1.6e-4
against 1.2e-4), offset256-proc_edge (4.7e-4 against 2.7e-4) and offset8-proc_edge (1.03e-5 against 1e-5), and the training
forward at hidden 256 on offset8-all (4.4e-5 against 3.0e-5) and offset256-all (1.3e-3 against 9.0e-4); with the coarse mean off
the restatement is within 3e-7 of float64 on every case.
"""
import collections
import functools

import numpy as np

from oracle import epd_oracle as orc
import train_step_cases as sc

F32, F64 = np.float32, np.float64
M_STEPS = 2
SCENE_SEED = 11
EPS_VALUES = (1e-12, 1e-5, 1e-2, 1.0)


def dims(hidden, nl):
    return (25, 4, 3, hidden, nl, M_STEPS)


# the groups of MLPs a regime is applied to (prefixes in state_dict naming)
TARGETS = collections.OrderedDict([
    ("enc_edge", ("encoder.phi_edge",)),
    ("enc_node", ("encoder.phi_node",)),
    ("proc_edge", tuple(f"processor.{k}.phi_edge" for k in range(M_STEPS))),
    ("proc_node", tuple(f"processor.{k}.phi_node" for k in range(M_STEPS))),
])
TARGETS["all"] = tuple(p for group in list(TARGETS.values()) for p in group)

Case = collections.namedtuple("Case", "name regime arg target eps")


def _case(regime, arg, target, eps):
    tag = regime if arg is None else f"{regime}{arg:g}"
    return Case(f"{tag}-{target}-eps{eps:g}", regime, arg, target, eps)


def _table():
    cases = [_case("plain", None, "all", 1e-5)]
    for regime, args in (("shrunk", (7, 10, 14)), ("offset", (8, 256)), ("flat", (0, 1.5))):
        for arg in args:
            cases += [_case(regime, arg, target, 1e-5) for target in TARGETS]
    cases += [_case("shrunk", 14, target, 1e-12) for target in TARGETS]
    cases += [_case("plain", None, "all", 1e-2), _case("plain", None, "all", 1.0)]
    return cases


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
# the cases with every MLP edited (and the plain weights at every eps): what the training and block tests run
ALL_MLPS = [c for c in CASES if c.target == "all"]


@functools.lru_cache(maxsize=None)
def scene():
    """(nodes [300, 25], edge_attr [E, 4], edge_index [2, E]), read-only."""
    g = sc.scene_graph(SCENE_SEED)
    for a in g:
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def scene_sorted():
    """The scene with its edges in destination order (then source order): the order the library's destination sort gives them, so
    that edge_attr may be handed to gm_epd_forward as already sorted -- what a rollout step does with the features it computes."""
    nodes, ea, ei = scene()
    perm = np.lexsort((ei[0], ei[1]))
    return _frozen(nodes, np.ascontiguousarray(ea[perm]), np.ascontiguousarray(ei[:, perm]))


@functools.lru_cache(maxsize=None)
def base_params(hidden, nl):
    return orc.init_params(*dims(hidden, nl), 5000 + hidden + nl)


def edit(params, nl, regime, arg, prefixes):
    """A copy of `params` with the regime's edit on the Linear in front of the LayerNorm of every MLP in `prefixes`: float32 in,
    float32 out, every operation rounded to float32 -- the reference runs on exactly these arrays."""
    p = {k: v.copy() for k, v in params.items()}
    for prefix in prefixes:
        wk, bk = f"{prefix}.{2 * nl}.weight", f"{prefix}.{2 * nl}.bias"
        w, b = p[wk], p[bk]
        if regime == "shrunk":
            s = F32(2.0 ** -arg)
            w, b = w * s, b * s
        elif regime == "offset":
            w, b = w + F32(arg / w.shape[1]), b + F32(arg)
        elif regime == "flat":
            w, b = np.zeros_like(w), np.full_like(b, F32(arg))
        else:
            assert regime == "plain", regime
        assert w.dtype == F32 and b.dtype == F32
        p[wk], p[bk] = w, b
    return p


@functools.lru_cache(maxsize=None)
def case_params(hidden, nl, name):
    c = BY_NAME[name]
    p = edit(base_params(hidden, nl), nl, c.regime, c.arg, TARGETS[c.target])
    for v in p.values():
        v.setflags(write=False)
    return p


def rel_err(a, ref):
    """max |a - ref| / max |ref|."""
    a, ref = np.asarray(a, F64), np.asarray(ref, F64)
    return float(np.abs(a - ref).max() / max(float(np.abs(ref).max()), 1e-300))


def forward_bar(e32):
    """The project's 1e-5 forward bar, widened the way tests/yardstick.py widens the gradients': the library is not held to more
    than the same computation in float32 delivers."""
    return max(1e-5, 4.0 * e32)


# ------------------------------------------------------------------------------------------ torch references (float64 and float32)
def _torch_params(p, dtype):
    import torch
    return {k: torch.tensor(v, dtype=dtype) for k, v in p.items()}


def torch_forward(p, nodes, ea, ei, nl, ms, eps, dtype):
    import torch
    from oracle import torch_epd
    with torch.no_grad():
        return torch_epd.epd_forward(_torch_params(p, dtype), torch.tensor(nodes, dtype=dtype), torch.tensor(ea, dtype=dtype),
                                     torch.tensor(ei, dtype=torch.int64), nl, ms, eps).numpy()


def torch_encoder(p, nodes, ea, nl, eps, dtype):
    """(h, e) of the GraphIndependent block."""
    import torch
    from oracle import torch_epd
    tp = _torch_params(p, dtype)
    with torch.no_grad():
        return (torch_epd.mlp(tp, "encoder.phi_node", torch.tensor(nodes, dtype=dtype), nl, True, eps).numpy(),
                torch_epd.mlp(tp, "encoder.phi_edge", torch.tensor(ea, dtype=dtype), nl, True, eps).numpy())


def torch_block(p, prefix, h, e, ei, nl, eps, dtype):
    """(h', e') of an InteractionNetwork block, no residual."""
    import torch
    from oracle import torch_epd
    tp = _torch_params(p, dtype)
    h, e, ei = torch.tensor(h, dtype=dtype), torch.tensor(e, dtype=dtype), torch.tensor(ei, dtype=torch.int64)
    with torch.no_grad():
        e_new = torch_epd.mlp(tp, f"{prefix}.phi_edge", torch.cat((h[ei[1]], h[ei[0]], e), dim=1), nl, True, eps)
        agg = torch.zeros_like(h).index_add_(0, ei[1], e_new)
        h_new = torch_epd.mlp(tp, f"{prefix}.phi_node", torch.cat((h, agg), dim=1), nl, True, eps)
    return h_new.numpy(), e_new.numpy()


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def forward_reference(hidden, nl, name):
    """(ref64, ref32, e32) of a case's whole forward: oracle/torch_epd.py in float64 and float32 on the case's parameters and eps."""
    import torch
    c = BY_NAME[name]
    p = case_params(hidden, nl, name)
    r64 = torch_forward(p, *scene(), nl, M_STEPS, c.eps, torch.float64)
    r32 = torch_forward(p, *scene(), nl, M_STEPS, c.eps, torch.float32)
    _frozen(r64, r32)
    return r64, r32, rel_err(r32, r64)


def feature_scaled(p, nodes, ea, c):
    """Raw features times c and the encoders' first Linears divided by c (float32): the same function, other raw magnitudes."""
    c32 = F32(c)
    q = dict(p)
    for k in ("encoder.phi_node.0.weight", "encoder.phi_edge.0.weight"):
        q[k] = (p[k] / c32).astype(F32)
    return q, (nodes * c32).astype(F32), (ea * c32).astype(F32)


@functools.lru_cache(maxsize=None)
def encoder_reference(hidden, nl, name, feature_scale=1.0):
    """((h64, e64), (h32, e32)) of the stand-alone encoder on the scene's raw features times feature_scale."""
    import torch
    c = BY_NAME[name]
    p, nodes, ea = feature_scaled(case_params(hidden, nl, name), scene()[0], scene()[1], feature_scale)
    r64 = torch_encoder(p, nodes, ea, nl, c.eps, torch.float64)
    r32 = torch_encoder(p, nodes, ea, nl, c.eps, torch.float32)
    _frozen(*r64, *r32)
    return r64, r32


@functools.lru_cache(maxsize=None)
def block_inputs(hidden):
    """(h [N, hidden], e [E, hidden]) of the stand-alone processor block: seeded standard normal latents on the scene's edges."""
    rng = np.random.Generator(np.random.PCG64(6000 + hidden))
    n, ne = scene()[0].shape[0], scene()[1].shape[0]
    return _frozen(rng.standard_normal((n, hidden)).astype(F32), rng.standard_normal((ne, hidden)).astype(F32))


@functools.lru_cache(maxsize=None)
def block_reference(hidden, nl, name):
    """((h64, e64), (h32, e32)) of processor.0 on block_inputs."""
    import torch
    c = BY_NAME[name]
    p = case_params(hidden, nl, name)
    h, e = block_inputs(hidden)
    r64 = torch_block(p, "processor.0", h, e, scene()[2], nl, c.eps, torch.float64)
    r32 = torch_block(p, "processor.0", h, e, scene()[2], nl, c.eps, torch.float32)
    _frozen(*r64, *r32)
    return r64, r32


def target(out_dim=3, seed=77):
    return sc.step_target(scene()[0], out_dim, seed)


def gradient_reference(hidden, nl, name):
    """(out64, loss64, grads64, grads32) of one L1 step: oracle/torch_epd.loss_and_grads with the case's eps, in both precisions."""
    import torch
    from oracle import torch_epd
    c = BY_NAME[name]
    p = case_params(hidden, nl, name)
    out, loss, g64 = torch_epd.loss_and_grads(p, *scene(), target(), nl, M_STEPS, ln_eps=c.eps)
    _, _, g32 = torch_epd.loss_and_grads(p, *scene(), target(), nl, M_STEPS, torch.float32, ln_eps=c.eps)
    return out, loss, g64, g32


# ------------------------------------------------------------------------------------------ float64 restatement, with taps and mistakes
MISTAKES = ("eps_omitted", "eps_times_t", "eps_unpadded", "divided_by_hp", "mean_kept")
ACC_SCALE = 2.0   # the t of "eps_times_t": the kernels hold their accumulators at a power-of-two scale t (the chain's scale,
#                   times a per-row power of two in the encoders); t = 2 is the smallest such scale that is not 1


def padded_width(hidden):
    return next(w for w in (64, 128, 256) if hidden <= w)


def restated_layer_norm(z, gamma, beta, eps, mistake=None):
    """LayerNorm of the rows of z in float64, as torch defines it -- or with one of MISTAKES built in, each stated on the unscaled
    z (Hv = z.shape[1] real features, Hp = padded_width(Hv), Q = the centred sum of squares):
      eps_omitted    1 / sqrt(Q / Hv)                       (a row of variance 0 is left at its bias)
      eps_times_t    accumulators a = t z: a / sqrt(eps t + mean a^2) = z / sqrt(eps / t + Q / Hv)
      eps_unpadded   the LayerNorm over Hp with gamma sqrt(Hv / Hp) but eps in place of eps Hv / Hp: z / sqrt(Q / Hv + eps Hp / Hv)
      divided_by_hp  z / sqrt(Q / Hp + eps)
      mean_kept      no mean subtracted: z / sqrt(mean z^2 + eps)"""
    z = np.asarray(z, F64)
    hv = z.shape[1]
    hp = padded_width(hv)
    zc = z if mistake == "mean_kept" else z - z.mean(axis=1, keepdims=True)
    q = (zc * zc).sum(axis=1, keepdims=True)
    var = q / (hp if mistake == "divided_by_hp" else hv)
    e = {"eps_omitted": 0.0, "eps_times_t": eps / ACC_SCALE, "eps_unpadded": eps * hp / hv}.get(mistake, eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = 1.0 / np.sqrt(var + e)
    k = np.where(np.isfinite(k), k, 0.0)
    return zc * k * np.asarray(gamma, F64) + np.asarray(beta, F64)


class EpsPerMlp:
    """An eps for restated_forward that differs between MLPs: `default`, or `by_prefix[prefix]` where there is one."""

    def __init__(self, default, by_prefix):
        self.default, self.by_prefix = default, dict(by_prefix)

    def of(self, prefix):
        return self.by_prefix.get(prefix, self.default)


def restated_mlp(p, prefix, x, nl, norm, eps, mistake=None, taps=None):
    if isinstance(eps, EpsPerMlp):
        eps = eps.of(prefix)
    x = np.asarray(x, F64)
    for l in range(nl + 1):
        x = x @ np.asarray(p[f"{prefix}.{2 * l}.weight"], F64).T + np.asarray(p[f"{prefix}.{2 * l}.bias"], F64)
        if l < nl:
            x = np.maximum(x, 0.0)
    if norm:
        if taps is not None:
            taps.setdefault(prefix, []).append(x.var(axis=1))
        x = restated_layer_norm(x, p[f"{prefix}.{2 * nl + 1}.weight"], p[f"{prefix}.{2 * nl + 1}.bias"], eps, mistake)
    return x


def restated_forward(p, nodes, ea, ei, nl, ms, eps, mistake=None, taps=None):
    """The model's forward in float64 numpy.  taps: a dict that receives, per MLP prefix, the variance of every row entering its
    LayerNorm.  mistake: one of MISTAKES, built into every LayerNorm."""
    j, i = np.asarray(ei[0]), np.asarray(ei[1])
    h = restated_mlp(p, "encoder.phi_node", nodes, nl, True, eps, mistake, taps)
    e = restated_mlp(p, "encoder.phi_edge", ea, nl, True, eps, mistake, taps)
    for k in range(ms):
        e_new = restated_mlp(p, f"processor.{k}.phi_edge", np.concatenate((h[i], h[j], e), axis=1), nl, True, eps, mistake, taps)
        agg = np.zeros_like(h)
        np.add.at(agg, i, e_new)
        h_new = restated_mlp(p, f"processor.{k}.phi_node", np.concatenate((h, agg), axis=1), nl, True, eps, mistake, taps)
        h, e = h + h_new, e + e_new
    return restated_mlp(p, "decoder", h, nl, False, eps)


def variance_over_eps(hidden, nl, name):
    """(min, median, max) over the rows of the case's edited MLPs (all of them for the plain weights) of the variance entering the
    LayerNorm, divided by the case's eps -- float64."""
    c = BY_NAME[name]
    taps = {}
    restated_forward(case_params(hidden, nl, name), *scene(), nl, M_STEPS, c.eps, taps=taps)
    v = np.concatenate([a for prefix in TARGETS[c.target] for a in taps[prefix]]) / c.eps
    return float(v.min()), float(np.median(v)), float(v.max())
