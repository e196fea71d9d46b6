"""Numeric domain, precision and NaN handling of the TRAINING kernels (csrc/train.hip, csrc/train_model.hip; include/gnn_manip_hip.h,
"Numeric domain of the training entry points"), on the cases of tests/train_domain_cases.py (checked on the CPU by
tests/test_train_domain_cases.py).  The training twin of tests/test_gpu_domain.py.

  1. Exact homogeneity.  The chains split every operand into three bf16 parts with the full float exponent range and accumulate in
     fp32: a rescaling by a power of two changes exponents only, so the results of the rescaled run are those of the base run
     times the power of two BIT FOR BIT (torch.equal on the device results; no reference, no tolerance).  An fp16 intermediate, a
     per-array scale or an absolute threshold anywhere on the path breaks it.
  2. Float32 accuracy where the gradient is continuous: on models whose every ReLU is away from zero by a margin, each gradient
     within tol_case = 4 x plain float32 PyTorch's own worst error of that case (at most 5e-6 of a tensor's maximum; no 2e-4
     floor, no flip allowance), the prediction within max(2.5 x float32's error, 2.5e-6).
  3. Non-finite values stay visible: the rows that are NaN in the float32 restatement are NaN here, every other row is bit-equal
     to the healthy run, the loss is NaN and every parameter gradient that is non-finite in the restatement is non-finite here.

Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from oracle import torch_epd
import train_domain_cases as tc
from gpu_support import compare_parameter_gradients as _compare_gradients, dev, load_model as _model, to_dev as _t

pytestmark = pytest.mark.gpu


def _step(params, dims, nodes, ea, ei, w, dev):
    """One training step through EncProcDecGNN with the loss (out * w).sum(): (prediction, {name: gradient}) on the device, the
    input gradients as d_nodes / d_edge_attr."""
    m = _model(params, dims, dev)
    x, a = _t(nodes, dev).requires_grad_(True), _t(ea, dev).requires_grad_(True)
    out = m.forward(x, a, _t(ei, dev))
    assert out.grad_fn is not None
    (out * _t(w, dev)).sum().backward()
    g = {k: p.grad for k, p in m.named_parameters()}
    assert all(v is not None for v in g.values())
    g["d_nodes"], g["d_edge_attr"] = x.grad, a.grad
    return out.detach(), g


_BASE = {}


def _base(hidden, dev):
    """The unscaled step of homogeneity_case(hidden), run once per module."""
    if hidden not in _BASE:
        dims, params, nodes, ea, ei, w = tc.homogeneity_case(hidden)
        out, g = _step(params, dims, nodes, ea, ei, w, dev)
        assert torch.isfinite(out).all() and all(torch.isfinite(v).all() and float(v.abs().max()) > 0 for v in g.values())
        _BASE[hidden] = (out, g)
    return _BASE[hidden]


def _assert_scaled(what, out, g, base_out, base_g, log2):
    """The prediction is the base run's and every gradient the base run's times 2^log2[name] (default 0), bit for bit."""
    assert torch.equal(out, base_out), (what, "prediction", float((out - base_out).abs().max()))
    for k, b in base_g.items():
        want = b * (2.0 ** log2.get(k, 0))
        assert torch.isfinite(want).all()
        assert torch.equal(g[k], want), (what, k, float(((g[k] - want).abs() / want.abs().max()).max()))


# ------------------------------------------------------------------------------------------ 1. exact homogeneity
@pytest.mark.parametrize("hidden", tc.HOMOGENEITY_HIDDEN)
def test_gradient_scale_is_exact(dev, hidden):
    """The backward is linear in grad_out: with w * 2^k, k = -20 / +20, every parameter gradient and both input gradients are the
    base run's times 2^k, bit for bit -- gradients of 1e-9 and of 1e+5 go through the same splits with no scale search."""
    dims, params, nodes, ea, ei, w = tc.homogeneity_case(hidden)
    base_out, base_g = _base(hidden, dev)
    for k in tc.GRAD_SCALE_LOG2:
        out, g = _step(params, dims, nodes, ea, ei, tc.pow2(w, k), dev)
        _assert_scaled(f"w * 2^{k}", out, g, base_out, base_g, {name: k for name in base_g})


@pytest.mark.parametrize("hidden", [64, 128, 256])
@pytest.mark.parametrize("log2s", tc.WEIGHT_SCALE_LOG2)
def test_weight_rescaling_between_linears_is_exact(dev, hidden, log2s):
    """The training twin of test_gpu_domain.test_weight_rescaling_between_linears_is_immaterial: (W_l, b_l) * s with W_(l+1) / s,
    s = 2^log2s, for five MLPs and both pairs of Linears.  The hidden activations in between -- and the tape's a_l -- are s times
    larger or smaller; the training forward's prediction is bit-equal to the unscaled model's, dW_l and db_l are the base
    gradients / s, dW_(l+1) the base gradient * s, everything else (input gradients included) bit-equal."""
    dims, params, nodes, ea, ei, w = tc.homogeneity_case(hidden)
    base_out, base_g = _base(hidden, dev)
    for mlp in tc.MLPS:
        for l in range(dims[4]):
            out, g = _step(tc.rescale_linear_pair(params, mlp, l, log2s), dims, nodes, ea, ei, w, dev)
            _assert_scaled(f"{mlp} pair {l} s = 2^{log2s}", out, g, base_out, base_g,
                           {f"{mlp}.{2 * l}.weight": -log2s, f"{mlp}.{2 * l}.bias": -log2s, f"{mlp}.{2 * l + 2}.weight": log2s})


@pytest.mark.parametrize("hidden", tc.HOMOGENEITY_HIDDEN)
@pytest.mark.parametrize("k", tc.FEATURE_SCALE_LOG2)
def test_feature_magnitude_is_exact(dev, hidden, k):
    """Raw features times c = 2^k (1e-6 .. 8e3) with both encoders' first weights / c: the prediction is bit-equal, the two
    first-weight gradients are the base times c, d_nodes and d_edge_attr the base / c, everything else bit-equal."""
    dims, params, nodes, ea, ei, w = tc.homogeneity_case(hidden)
    base_out, base_g = _base(hidden, dev)
    p, nodes_c, ea_c = tc.rescale_features(params, nodes, ea, k)
    out, g = _step(p, dims, nodes_c, ea_c, ei, w, dev)
    _assert_scaled(f"features * 2^{k}", out, g, base_out, base_g,
                   {"encoder.phi_node.0.weight": k, "encoder.phi_edge.0.weight": k, "d_nodes": -k, "d_edge_attr": -k})


@pytest.mark.parametrize("hidden", [64, 128, 256])
def test_rows_of_very_different_gradient_magnitude_in_one_tile(dev, hidden):
    """The standalone GraphIndependent under autograd with inputs that require grad: dx / dedge_attr are row-local (LayerNorm and
    the Linears act per row).  Row i of the incoming dh / de times 2^(r_i), r_i in -40 .. +20 inside every 128-row tile and one
    row exactly zero: row i of dx / dedge_attr is the unscaled run's row times 2^(r_i), bit for bit, and the zero row exactly
    zero -- 60 binades inside one array with no scale search."""
    dims, params, nodes, ea, ei, _ = tc.homogeneity_case(hidden)
    m = _model(params, dims, dev)
    rng = np.random.default_rng(hidden)
    dh = _t(rng.standard_normal((nodes.shape[0], hidden)).astype(np.float32), dev)
    de = _t(rng.standard_normal((ea.shape[0], hidden)).astype(np.float32), dev)
    fh, fe = _t(tc.row_factors(nodes.shape[0], hidden), dev), _t(tc.row_factors(ea.shape[0], hidden + 1), dev)

    def run(dh, de):
        x, a = _t(nodes, dev).requires_grad_(True), _t(ea, dev).requires_grad_(True)
        h, e, _ = m.encoder(x, a, _t(ei, dev))
        assert h.grad_fn is not None and e.grad_fn is not None
        torch.autograd.backward([h, e], [dh, de])
        return x.grad, a.grad

    dx0, da0 = run(dh, de)
    dx1, da1 = run(dh * fh, de * fe)
    assert torch.isfinite(dx0).all() and torch.isfinite(da0).all() and float(dx0.abs().min(dim=1).values.max()) > 0
    for what, got, base, f in (("dx", dx1, dx0, fh), ("dedge_attr", da1, da0, fe)):
        want = base * f
        bad = (got != want).any(dim=1)
        assert not bool(bad.any()), (what, int(bad.sum()), torch.log2(f[bad]).flatten()[:8].tolist())
        assert not bool(got[tc.ROW_ZERO].any()) and bool(got[tc.ROW_ZERO + 1].any())


# ------------------------------------------------------------------------------------------ 2. float32 accuracy
@pytest.mark.parametrize("name", list(tc.CALIBRATED))
def test_gradients_are_float32_accurate_where_they_are_continuous(dev, name):
    """Calibrated biases keep every pre-activation at least 1e-3 rms from zero (checked on the CPU), so no ReLU's sign depends on
    rounding and the 2e-4 floor of test_gpu_train.py has nothing to cover: every parameter gradient and both input gradients
    within tol_case = 4 x float32 PyTorch's worst error in this case of the float64 gradient's maximum, the prediction within
    max(2.5 x float32's error, 2.5e-6); the weight-gradient rows of dead units exactly zero.
    Measured on an MI355X, worst err / tol_case over a case's tensors (and the prediction's err / its bar): hidden128 0.25 (0.26),
    hidden64_depth3 0.30 (0.35), hidden256 0.33 (0.68), padded100 0.25 (0.21), depth4 0.17 (0.13); tol_case was 5.0e-6 (the cap)
    but for hidden256's 3.9e-6.  Without the a.m x b.m product of mfma_bf3 the gradient ratios are 3.3 .. 5.5; with the tape
    rounded to 16 bits 0.45 .. 1.55."""
    c = tc.calibrated(name)
    out, g = _step(c.params, c.dims, c.nodes, c.ea, c.ei, c.w, dev)
    err_out = tc.rel_err(out.cpu().numpy(), c.out64)
    print(f"\n[train domain] {name}: prediction err {err_out:.3e} bar {c.out_tol:.3e} (float32 torch {c.out_err32:.3e}); tol_case {c.tol_case:.3e}")
    worst = ("", 0.0)
    for k, r in c.g64.items():
        got = g[k].cpu().numpy()
        assert got.shape == r.shape and np.isfinite(got).all(), k
        if np.abs(r).max() == 0:
            assert not got.any(), k
            continue
        err = tc.rel_err(got, r)
        print(f"[train domain] {name} {k}: err {err:.3e} (float32 torch {c.err32[k]:.3e}) ratio {err / c.tol_case:.3f}")
        if err / c.tol_case > worst[1]:
            worst = (k, err / c.tol_case)
    print(f"[train domain] {name}: worst gradient ratio {worst[1]:.3f} ({worst[0]}), prediction ratio {err_out / c.out_tol:.3f}")
    assert err_out <= c.out_tol, (err_out, c.out_tol)
    assert worst[1] <= 1.0, worst
    for mlp in tc.mlp_prefixes(c.dims[5]):           # half the units of every hidden Linear are dead on every row
        for l in range(c.dims[4]):
            dead = torch.from_numpy(c.params[f"{mlp}.{2 * l}.bias"] < 0).to(dev)
            assert not bool(g[f"{mlp}.{2 * l}.weight"][dead].any()) and not bool(g[f"{mlp}.{2 * l}.bias"][dead].any()), (mlp, l)


@pytest.mark.parametrize("hidden", tc.ROW_MAGNITUDE_HIDDEN)
def test_rows_of_very_different_feature_magnitude(dev, hidden):
    """The training forward's twin of test_gpu_domain.test_rows_of_very_different_magnitude: node and edge rows scaled by
    10^U(-6, 4) with one all-zero row each, an uncalibrated model.  Prediction within max(2.5 x float32's error, 2.5e-6) of float64;
    the gradients of the L1 loss to the rule of tests/yardstick.py (sign flips are possible for this model)."""
    dims, params, nodes, ea, ei, seed = tc.row_magnitude_case(hidden)
    target = np.random.default_rng(seed).standard_normal((nodes.shape[0], 3)).astype(np.float32)
    m = _model(params, dims, dev)
    out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev))
    loss = torch.nn.functional.l1_loss(out, _t(target, dev), reduction="sum") / out.shape[0]
    loss.backward()
    ref_out, ref_loss, ref_g = torch_epd.loss_and_grads(params, nodes, ea, ei, target, dims[4], dims[5])
    out32, _, g32 = torch_epd.loss_and_grads(params, nodes, ea, ei, target, dims[4], dims[5], torch.float32)
    err, err32 = tc.rel_err(out.detach().cpu().numpy(), ref_out), tc.rel_err(out32, ref_out)
    print(f"\n[train domain] row magnitudes hidden {hidden}: prediction err {err:.3e} (float32 torch {err32:.3e})")
    assert err <= max(2.5 * err32, tc.FORWARD_FLOOR), (err, err32)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * abs(ref_loss)
    print("[train domain] gradients:", _compare_gradients(m, params, nodes, ea, ei, target, dims[4], dims[5], ref_g, g32))


# ------------------------------------------------------------------------------------------ 3. non-finite values
@pytest.mark.parametrize("hidden", tc.NAN_HIDDEN)
@pytest.mark.parametrize("what", list(tc.BAD_VALUES))
def test_non_finite_value_shows_in_prediction_loss_and_gradients(dev, hidden, what):
    """One NaN / inf in a feature row, or one NaN in a weight after a diverged optimiser step.  fmaxf(z, 0) is 0 for a NaN z: a
    chain that applies its ReLU that way hands the next Linear a clean row and returns a finite, wrong prediction, loss and
    gradients.  The contract is the float32 restatement's: its NaN rows are NaN here, every other row is bit-equal to the healthy
    step, the L1 loss (train_dyn.py:65) is NaN, and every parameter gradient that is non-finite there holds a non-finite value
    here -- no optimiser step can proceed as if the batch were healthy."""
    c = tc.nan_case(hidden, what)
    idx, tgt = _t(c.ei, dev), _t(c.target, dev)
    healthy = _model(c.params, c.dims, dev).forward(_t(c.nodes, dev), _t(c.ea, dev), idx)
    assert healthy.grad_fn is not None and torch.isfinite(healthy).all()
    m = _model(c.bad_params, c.dims, dev)
    out = m.forward(_t(c.bad_nodes, dev), _t(c.bad_ea, dev), idx)
    loss = torch.nn.functional.l1_loss(out, tgt, reduction="sum") / out.shape[0]
    loss.backward()
    rows = torch.from_numpy(c.nan_rows).to(dev)
    got = torch.isnan(out.detach()).all(dim=1)
    print(f"\n[train domain] {what} hidden {hidden}: {int(rows.sum())} NaN rows in the reference, {int(got.sum())} on the device, loss {float(loss.detach())}")
    assert bool(got[rows].all()), (int(rows.sum()), int(got[rows].sum()))
    assert torch.equal(out.detach()[~rows], healthy.detach()[~rows])
    assert bool(torch.isnan(loss))
    grads = dict(m.named_parameters())
    finite = [k for k in c.nonfinite_grads if bool(torch.isfinite(grads[k].grad).all())]
    assert not finite, finite


@pytest.mark.parametrize("hidden", [128, 64])
@pytest.mark.parametrize("what", tc.FEATURE_CASES)
def test_standalone_blocks_keep_a_non_finite_row_visible(dev, hidden, what):
    """The same rule for h_out / e_out of the standalone GraphIndependent and InteractionNetwork under autograd (the training
    entry points of the blocks; they take the kernels' own widths), with the bad value in a raw feature row and in a latent row."""
    c = tc.nan_case(hidden, "nan_node_feature")
    m = _model(c.params, c.dims, dev)
    idx = _t(c.ei, dev)
    for kind, block, prefix, clean in (("encoder", m.encoder, "encoder.", (c.nodes, c.ea)),
                                       ("processor", m.processor[0], "processor.0.", tc.block_latents(hidden))):
        a0, b0 = (_t(v, dev).requires_grad_(True) for v in clean)
        h0, e0, _ = block(a0, b0, idx)
        assert h0.grad_fn is not None and torch.isfinite(h0).all() and torch.isfinite(e0).all()
        bad_a, bad_b = tc.with_bad_value(*clean, what)
        ref_h, ref_e, ref_bad = tc.standalone_reference(c.params, kind, bad_a, bad_b, c.ei)
        a1, b1 = _t(bad_a, dev).requires_grad_(True), _t(bad_b, dev).requires_grad_(True)
        m.zero_grad()
        h1, e1, _ = block(a1, b1, idx)
        (h1.abs().sum() + e1.abs().sum()).backward()
        for name, got, base, ref in (("h_out", h1, h0, ref_h), ("e_out", e1, e0, ref_e)):
            rows = torch.from_numpy(np.isnan(ref).any(axis=1)).to(dev)
            print(f"\n[train domain] {kind} {what} hidden {hidden} {name}: {int(rows.sum())} NaN rows in the reference, "
                  f"{int(torch.isnan(got.detach()).all(dim=1).sum())} on the device")
            assert bool(torch.isnan(got.detach()[rows]).all()), (kind, name)
            assert torch.equal(got.detach()[~rows], base.detach()[~rows]), (kind, name)
        grads = {prefix + k: p.grad for k, p in block.named_parameters()}
        finite = [k for k in ref_bad if bool(torch.isfinite(grads[k]).all())]
        assert not finite, (kind, finite)
