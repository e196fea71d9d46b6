"""CPU: the case table of layernorm_cases.py is what it claims to be -- its references are torch's LayerNorm, its regimes put eps and
the centring where they decide the output, and each plausible wrong treatment of eps or of the mean moves at least one case by more
than ten times the bar tests/test_gpu_layernorm.py applies."""
import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
import layernorm_cases as lc
import precision_cases as pc

H, NL = 128, 2
NAMES = [c.name for c in lc.CASES]


def _z_rows(hidden, nl, name):
    """The rows entering the node encoder's LayerNorm (float64), the gain and the bias of that LayerNorm."""
    p = lc.case_params(hidden, nl, name)
    z = lc.restated_mlp(p, "encoder.phi_node", lc.scene()[0], nl, False, None)
    return z, p[f"encoder.phi_node.{2 * nl + 1}.weight"], p[f"encoder.phi_node.{2 * nl + 1}.bias"]


@pytest.mark.parametrize("name", [c.name for c in lc.CASES if c.target in ("enc_node", "all")])
def test_restated_layer_norm_is_torchs(name):
    """restated_layer_norm against torch.nn.functional.layer_norm and torch.nn.LayerNorm(eps=...) in float64 on the rows every regime
    feeds the node encoder's LayerNorm: float64 rounding, which on offset(c) is c / sigma ulps (sigma >= 0.06: under 1e-11 at c = 256)."""
    c = lc.BY_NAME[name]
    z, g, b = _z_rows(H, NL, name)
    got = lc.restated_layer_norm(z, g, b, c.eps)
    tz, tg, tb = (torch.tensor(np.asarray(a), dtype=torch.float64) for a in (z, g, b))
    fn = torch.nn.functional.layer_norm(tz, (z.shape[1],), tg, tb, c.eps).numpy()
    mod = torch.nn.LayerNorm(z.shape[1], eps=c.eps).double()
    with torch.no_grad():
        mod.weight.copy_(tg)
        mod.bias.copy_(tb)
        via_module = mod(tz).numpy()
    assert np.array_equal(fn, via_module)
    assert lc.rel_err(got, fn) <= 1e-11, (name, lc.rel_err(got, fn))
    # the float32 numpy oracle with the same eps: float32 rounding of the same function (c / sigma ulps of float32 on offset(c))
    o32 = orc.layer_norm(z.astype(np.float32), g, b, ln_eps=c.eps)
    bound = 1e-6 * (1.0 + (c.arg if c.regime == "offset" else 0.0) / 0.06)
    assert lc.rel_err(o32, fn) <= bound, (name, lc.rel_err(o32, fn), bound)


@pytest.mark.parametrize("name", [c.name for c in lc.ALL_MLPS])
def test_references_agree_with_each_other(name):
    """The eps-taking references on a whole forward: the float64 restatement against oracle/torch_epd.py in float64 (rounding); the
    float32 numpy oracle and precision_cases' restatement of the packed form (centred weights, no mean in the LayerNorm, nothing
    rounded) against it within the bar the library is held to."""
    c = lc.BY_NAME[name]
    p = lc.case_params(H, NL, name)
    r64, _, e32 = lc.forward_reference(H, NL, name)
    rest = lc.restated_forward(p, *lc.scene(), NL, lc.M_STEPS, c.eps)
    o32 = orc.epd_forward(p, *lc.scene(), NL, lc.M_STEPS, ln_eps=c.eps)
    packed = pc.epd_forward(p, *lc.scene(), NL, lc.M_STEPS, round_w=False, round_x=False, ln_eps=c.eps)
    bar = lc.forward_bar(e32)
    print(f"\n[layernorm] {name}: restatement {lc.rel_err(rest, r64):.2e}, numpy float32 oracle {lc.rel_err(o32, r64):.2e}, packed form "
          f"{lc.rel_err(packed, r64):.2e}; e32 {e32:.2e}, bar {bar:.2e}")
    assert lc.rel_err(rest, r64) <= 1e-9, name
    assert lc.rel_err(o32, r64) <= bar, name
    assert lc.rel_err(packed, r64) <= bar, name


@pytest.mark.parametrize("name", [c.name for c in lc.CASES if c.regime == "offset"])
def test_packed_form_removes_a_large_mean(name):
    """The restatement of the inference kernels' form (W3, b3 centred as the pack kernels centre them, variance = mean square) on
    offset(c), one MLP at a time and all together: within the bar.  With the pack's means in float32 it was not (layernorm_cases'
    docstring has the figures)."""
    c = lc.BY_NAME[name]
    r64, _, e32 = lc.forward_reference(H, NL, name)
    packed = pc.epd_forward(lc.case_params(H, NL, name), *lc.scene(), NL, lc.M_STEPS, round_w=False, round_x=False, ln_eps=c.eps)
    err, bar = lc.rel_err(packed, r64), lc.forward_bar(e32)
    print(f"\n[layernorm] {name}: packed form {err:.2e}, e32 {e32:.2e}, bar {bar:.2e}")
    assert err <= min(bar, 1e-6), (name, err)   # and far inside it: what float32 centres is no larger than the weights' spread


# (regime, arg, eps) -> bounds (lo, hi) of variance / eps over the rows of the edited MLPs, any target: a factor of about 2 around
# what the float64 reference shows on this scene at hidden 128 (layernorm_cases' table)
RATIO_BOUNDS = {
    ("plain", None, 1e-5): (2e2, 8e5), ("plain", None, 1e-2): (0.2, 5e2), ("plain", None, 1.0): (1.5e-3, 0.15),
    ("shrunk", 7, 1e-5): (1e-2, 50.0), ("shrunk", 10, 1e-5): (1.5e-4, 0.9), ("shrunk", 14, 1e-5): (6e-7, 4e-3),
    ("shrunk", 14, 1e-12): (8.0, 3e4),
    ("offset", 8, 1e-5): (2e2, 8e5), ("offset", 256, 1e-5): (2e2, 8e5),
    ("flat", 0, 1e-5): (0.0, 0.0), ("flat", 1.5, 1e-5): (0.0, 0.0),
}


@pytest.mark.parametrize("name", NAMES)
def test_regimes_are_what_they_claim(name):
    c = lc.BY_NAME[name]
    lo, med, hi = lc.variance_over_eps(H, NL, name)
    blo, bhi = RATIO_BOUNDS[(c.regime, c.arg, c.eps)]
    print(f"\n[layernorm] {name}: variance / eps over the edited rows: min {lo:.2e} median {med:.2e} max {hi:.2e} (bounds {blo:g} .. {bhi:g})")
    assert blo <= lo and hi <= bhi, (name, lo, hi)
    if c.regime == "shrunk" and c.eps == 1e-5 and c.target != "proc_node":
        # about eps (k = 7), far below it (k = 10), negligible (k = 14): the medians
        assert med <= {7: 0.2, 10: 3e-3, 14: 1.2e-5}[c.arg] and (c.arg != 7 or med >= 0.02)
    if c.regime in ("plain", "offset") and c.eps == 1e-5:
        assert med >= 5e2   # eps is a small correction: what the suite had before


@pytest.mark.parametrize("mistake", lc.MISTAKES)
def test_the_cases_catch_the_mistake(mistake):
    """Each wrong treatment, built into every LayerNorm of the float64 restatement, moves the prediction of at least one case by more
    than ten times that case's GPU bar.  The two mistakes of the padded width exist only at a hidden size between the kernels'
    widths: hidden 100."""
    hidden = 100 if mistake in ("eps_unpadded", "divided_by_hp") else H
    caught = []
    for c in lc.ALL_MLPS:
        p = lc.case_params(hidden, NL, c.name)
        r64, _, e32 = lc.forward_reference(hidden, NL, c.name)
        bad = lc.restated_forward(p, *lc.scene(), NL, lc.M_STEPS, c.eps, mistake=mistake)
        moved, bar = lc.rel_err(bad, r64), lc.forward_bar(e32)
        print(f"\n[layernorm] {mistake} at hidden {hidden}, {c.name}: moves the prediction by {moved:.2e} of its maximum, bar {bar:.2e}")
        if moved > 10 * bar:
            caught.append((c.name, moved / bar))
    assert caught, mistake
    if mistake != "divided_by_hp":   # (that one moves every case, the plain weights included)
        assert any(not name.startswith("plain-all-eps1e-05") for name, _ in caught)


@pytest.mark.parametrize("c", [8, 256])
@pytest.mark.parametrize("target", list(lc.TARGETS))
def test_offset_is_invisible_in_float64(c, target):
    """offset(c) leaves the float64 output where the same parameters with the shift taken off again in float64 put it: what is left is
    the float64 rounding of the shift itself.  A row's z carries c (1 + sum a / fan_in), at most 3 c here, on a standard deviation
    sigma >= 0.06: 3 c / sigma ulps of float64 per LayerNorm, times 1e3 for the sums over fan_in and the passage through the
    network: 3e3 * (c / 0.06) * 2^-53 -- 1.4e-9 at c = 256.  (Against the UNEDITED float32 weights the difference is the float32
    rounding of the edit, W3 + c / fan_in rounded to float32: a property of the regime, not of a LayerNorm.)"""
    name = f"offset{c:g}-{target}-eps1e-05"
    p = lc.case_params(H, NL, name)
    q = {k: np.asarray(v, np.float64) for k, v in p.items()}
    for prefix in lc.TARGETS[target]:
        w = q[f"{prefix}.{2 * NL}.weight"]
        q[f"{prefix}.{2 * NL}.weight"] = w - np.float64(np.float32(c / w.shape[1]))
        q[f"{prefix}.{2 * NL}.bias"] = q[f"{prefix}.{2 * NL}.bias"] - np.float64(c)
    shifted = lc.restated_forward(p, *lc.scene(), NL, lc.M_STEPS, 1e-5)
    unshifted = lc.restated_forward(q, *lc.scene(), NL, lc.M_STEPS, 1e-5)
    tol = 3e3 * (c / 0.06) * 2.0 ** -53
    print(f"\n[layernorm] {name}: float64 output moves by {lc.rel_err(shifted, unshifted):.2e} (tolerance {tol:.2e})")
    assert lc.rel_err(shifted, unshifted) <= tol
    # and the unshifted parameters are the plain ones to the float32 rounding of the edit: half an ulp of c / fan_in on W3
    plain = lc.base_params(H, NL)
    for prefix in lc.TARGETS[target]:
        w = q[f"{prefix}.{2 * NL}.weight"]
        assert np.abs(w - plain[f"{prefix}.{2 * NL}.weight"]).max() <= np.spacing(np.float32(c / w.shape[1] + 0.1))
        assert np.abs(q[f"{prefix}.{2 * NL}.bias"] - plain[f"{prefix}.{2 * NL}.bias"]).max() <= np.spacing(np.float32(c + 0.1))


@pytest.mark.parametrize("target", list(lc.TARGETS))
def test_shrunk_weights_at_a_tiny_eps_are_the_plain_ones(target):
    """shrunk(14) at eps = 1e-12 is the unshrunk model at eps = 2^28 * 1e-12 in the edited LayerNorms: a power of two commutes with
    every rounding, so in float64 the two differ by the rounding of eps 2^28 alone -- held to 1e-12.  And eps is small against the
    variance again (1 / 17 of it at the most), so the output is close to the plain weights' at 1e-5: within 3 percent."""
    name = f"shrunk14-{target}-eps1e-12"
    shrunk = lc.restated_forward(lc.case_params(H, NL, name), *lc.scene(), NL, lc.M_STEPS, 1e-12)
    eps_of = {prefix: 1e-12 * 2.0 ** 28 for prefix in lc.TARGETS[target]}
    plain = lc.restated_forward(lc.base_params(H, NL), *lc.scene(), NL, lc.M_STEPS, lc.EpsPerMlp(1e-12, eps_of))
    print(f"\n[layernorm] {name}: against the plain weights at eps 2^28 * 1e-12: {lc.rel_err(shrunk, plain):.2e}")
    assert lc.rel_err(shrunk, plain) <= 1e-12
    at_default = lc.forward_reference(H, NL, "plain-all-eps1e-05")[0]
    near = lc.rel_err(shrunk, at_default)
    print(f"[layernorm] {name}: against the plain weights at eps 1e-5: {near:.2e}")
    assert near <= 0.03


def test_table_covers_what_the_issue_names():
    assert len(lc.CASES) == len(set(NAMES)) == 1 + 7 * 5 + 5 + 2
    assert {c.eps for c in lc.CASES} == set(lc.EPS_VALUES)
    assert {(c.regime, c.arg) for c in lc.CASES if c.eps == 1e-5} == {("plain", None), ("shrunk", 7), ("shrunk", 10), ("shrunk", 14),
                                                                      ("offset", 8), ("offset", 256), ("flat", 0), ("flat", 1.5)}
    assert {(c.regime, c.arg) for c in lc.CASES if c.eps == 1e-12} == {("shrunk", 14)}
    assert {(c.regime, c.arg) for c in lc.CASES if c.eps in (1e-2, 1.0)} == {("plain", None)}
    n, e = lc.scene()[0].shape[0], lc.scene()[1].shape[0]
    assert n == 300 and 4000 <= e <= 6000 and n > 2 * 128 and e > 32 * 32   # several 32-row blocks, more than one 128-row tile
    for c in lc.CASES:   # float32 parameters, and only the named Linears differ from init_params
        p, base = lc.case_params(H, NL, c.name), lc.base_params(H, NL)
        changed = {k for k in p if not np.array_equal(p[k], base[k])}
        allowed = {f"{prefix}.{2 * NL}.{t}" for prefix in lc.TARGETS[c.target] for t in ("weight", "bias")}
        assert all(v.dtype == np.float32 for v in p.values()) and changed <= allowed
        assert (c.regime == "plain") == (not changed)


def test_model_desc_refuses_layer_norms_that_disagree_on_eps():
    """The library has one ln_eps per model: a model whose LayerNorms disagree is a ValueError that names both values, wherever the
    odd one sits; one common value, default or not, is the descriptor's."""
    from gnn_manip_amd import EncProcDecGNN
    m = EncProcDecGNN(*lc.dims(64, 2))
    assert m.model_desc()[6] == 1e-5
    for mod in m.modules():
        if isinstance(mod, torch.nn.LayerNorm):
            mod.eps = 1e-3
    assert m.model_desc()[6] == 1e-3
    for odd in (m.encoder.phi_node, m.processor[0].phi_edge, m.processor[1].phi_node):
        odd[-1].eps = 0.5
        with pytest.raises(ValueError, match="0.001 and 0.5"):
            m.model_desc()
        odd[-1].eps = 1e-3
    m.encoder.phi_edge[-1].eps = 0.25
    with pytest.raises(ValueError, match="0.25 and 0.001"):
        m.model_desc()
