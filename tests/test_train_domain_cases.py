"""The cases of tests/train_domain_cases.py are in the regimes they were built for (CPU; no GPU and no library): the rescalings are
exact in float32, the calibrated models keep every pre-activation away from zero by a margin and float32 PyTorch's gradients
within 1.25e-6 of float64's, and a non-finite value reaches exactly the rows the edge list says."""
import numpy as np
import pytest

from oracle import epd_oracle as orc
import train_domain_cases as tc


# ------------------------------------------------------------------------------------------ 1. exact rescalings
@pytest.mark.parametrize("hidden", tc.HOMOGENEITY_HIDDEN)
def test_rescaled_arrays_are_exact_in_float32(hidden):
    """Every array a homogeneity test scales -- loss weights, Linear pairs, features, first weights -- scales without overflow or
    a subnormal result, so both runs of a pair see the same numbers but for the exponent; and the float32 oracle's prediction of
    the rescaled model is the unscaled one's, bit for bit (the function is unchanged)."""
    dims, params, nodes, ea, ei, w = tc.homogeneity_case(hidden)
    assert 3000 <= ei.shape[1] <= 4600 and nodes.shape[0] == 300
    for k in tc.GRAD_SCALE_LOG2:
        assert tc.is_exact_pow2(w, k)
    ref0 = orc.epd_forward(params, nodes, ea, ei, dims[4], dims[5])
    for k in tc.WEIGHT_SCALE_LOG2:
        for mlp in tc.MLPS:
            for l in range(dims[4]):
                for name in (f"{mlp}.{2 * l}.weight", f"{mlp}.{2 * l}.bias"):
                    assert tc.is_exact_pow2(params[name], k), (name, k)
                assert tc.is_exact_pow2(params[f"{mlp}.{2 * l + 2}.weight"], -k), (mlp, l, k)
    p = tc.rescale_linear_pair(params, "processor.0.phi_edge", 1, 12)
    assert np.abs(orc.epd_forward(p, nodes, ea, ei, dims[4], dims[5]) - ref0).max() <= 2e-6 * np.abs(ref0).max()
    for k in tc.FEATURE_SCALE_LOG2:
        assert tc.is_exact_pow2(nodes, k) and tc.is_exact_pow2(ea, k), k
        for name in ("encoder.phi_node.0.weight", "encoder.phi_edge.0.weight"):
            assert tc.is_exact_pow2(params[name], -k), (name, k)
    p, nodes_c, ea_c = tc.rescale_features(params, nodes, ea, 13)
    assert np.abs(orc.epd_forward(p, nodes_c, ea_c, ei, dims[4], dims[5]) - ref0).max() <= 2e-6 * np.abs(ref0).max()


def test_row_factors_span_sixty_binades_and_keep_a_zero_row():
    f = tc.row_factors(300, 3)
    r = np.log2(f[f > 0])
    assert f.shape == (300, 1) and f.dtype == np.float32
    assert float(f[tc.ROW_ZERO, 0]) == 0.0 and int((f == 0).sum()) == 1
    assert r.min() == tc.ROW_SCALE_LOG2[0] and r.max() == tc.ROW_SCALE_LOG2[1] and np.array_equal(r, np.round(r))
    assert len(np.unique(r)) > 40                               # inside one 128-row tile, too
    assert len(np.unique(np.log2(f[:128][f[:128] > 0]))) > 30
    g = np.random.default_rng(1).standard_normal((300, 64)).astype(np.float32)
    nz = f[:, 0] > 0
    assert np.array_equal((g * f)[nz] / f[nz], g[nz])           # the scaled gradient rows are exact


# ------------------------------------------------------------------------------------------ 2. calibrated models
@pytest.mark.parametrize("name", list(tc.CALIBRATED))
def test_calibrated_case_keeps_every_relu_away_from_zero(name):
    c = tc.calibrated(name)
    nl, ms = c.dims[4], c.dims[5]
    reg = c.regime()
    assert len(reg) == nl * (3 + 2 * ms)
    for mlp, l, margin, active in reg:
        print(f"[train domain] {name} {mlp}.{2 * l}: min |z| / rms(z) {margin:.2e}, active {active:.3f}")
        assert margin >= tc.MARGIN_MIN, (mlp, l, margin)
        assert 0.3 <= active <= 0.7, (mlp, l, active)
    print(f"[train domain] {name}: tol_case {c.tol_case:.3e} (uncapped {c.tol_raw:.3e}), float32 torch worst {max(c.err32.values()):.3e} "
          f"median {np.median(list(c.err32.values())):.3e}, forward {c.out_err32:.3e}")
    assert c.tol_case <= tc.TOL_CASE_MAX, c.tol_case            # the bar can never quietly loosen
    assert c.tol_raw <= tc.TOL_RAW_MAX, c.tol_raw                # float32 PyTorch is itself in the continuous regime on this host
    assert c.tol_case >= 4 * 2.0 ** -24                          # ... nor drop below what float32 itself resolves
    assert 3000 <= c.ei.shape[1] <= 4600 and 200 <= c.nodes.shape[0] <= 300
    # the mask is mixed: every hidden Linear has dead units, and a dead unit's row of the weight gradient is exactly zero
    for mlp in tc.mlp_prefixes(ms):
        for l in range(nl):
            g = c.g64[f"{mlp}.{2 * l}.weight"]
            dead = c.params[f"{mlp}.{2 * l}.bias"] < 0
            assert dead.sum() == len(dead) - len(dead) // 2 and not g[dead].any() and c.g64[f"{mlp}.{2 * l}.bias"][~dead].all()
    assert all(np.abs(v).max() > 0 for v in c.g64.values())     # no tensor without a gradient to compare


@pytest.mark.parametrize("hidden", tc.ROW_MAGNITUDE_HIDDEN)
def test_row_magnitude_case_spans_ten_orders(hidden):
    dims, params, nodes, ea, ei, seed = tc.row_magnitude_case(hidden)
    for a, zero in ((nodes, 7), (ea, 11)):
        m = np.abs(a).max(axis=1)
        assert m[zero] == 0.0 and np.isfinite(a).all()
        assert m[m > 0].max() / m[m > 0].min() > 1e8
    assert np.ptp(np.log10(np.abs(nodes[:128]).max(axis=1)[8:])) > 8      # inside the first node tile


# ------------------------------------------------------------------------------------------ 3. non-finite values
@pytest.mark.parametrize("hidden", tc.NAN_HIDDEN)
@pytest.mark.parametrize("what", list(tc.BAD_VALUES))
def test_non_finite_case_reaches_the_rows_the_edge_list_says(hidden, what):
    c = tc.nan_case(hidden, what)
    n = c.nodes.shape[0]
    assert c.all_nan and np.isnan(c.ref_loss)
    assert np.array_equal(c.nan_rows, c.expected), (int(c.nan_rows.sum()), int(c.expected.sum()))
    assert np.isfinite(c.ref_out[~c.nan_rows]).all()
    assert c.nonfinite_grads, "the reference's backward must show the bad step"
    if what in tc.FEATURE_CASES:
        assert 0 < c.nan_rows.sum() <= n // 2 and c.nan_rows[c.bad_row]
        assert c.nan_rows.sum() > 1                              # the bad value does travel along edges
    elif what == "nan_encoder_weight":
        assert c.nan_rows.all()
    else:
        assert np.array_equal(c.nan_rows, np.bincount(c.ei[1], minlength=n) > 0) and c.nan_rows.sum() > n // 2


@pytest.mark.parametrize("hidden", [128, 64])
@pytest.mark.parametrize("what", tc.FEATURE_CASES)
def test_standalone_references_keep_a_bad_row_local(hidden, what):
    """The encoder block is row-local: only the bad row is NaN.  One InteractionNetwork spreads a bad latent one step."""
    c = tc.nan_case(hidden, "nan_node_feature")
    n = c.nodes.shape[0]
    node_side = tc.BAD_VALUES[what][0] == "nodes"
    h1, e1, bad = tc.standalone_reference(c.params, "encoder", *tc.with_bad_value(c.nodes, c.ea, what), c.ei)
    rows_h, rows_e = np.isnan(h1).any(axis=1), np.isnan(e1).any(axis=1)
    assert np.array_equal(np.nonzero(rows_h)[0], [tc.BAD_NODE] if node_side else [])
    assert np.array_equal(np.nonzero(rows_e)[0], [] if node_side else [tc.BAD_EDGE])
    assert np.isnan(h1[rows_h]).all() and np.isnan(e1[rows_e]).all()
    assert bad and all(k.startswith("encoder.phi_node." if node_side else "encoder.phi_edge.") for k in bad)
    h1, e1, bad = tc.standalone_reference(c.params, "processor", *tc.with_bad_value(*tc.block_latents(hidden), what), c.ei)
    rows_h, rows_e = np.isnan(h1).any(axis=1), np.isnan(e1).any(axis=1)
    if node_side:
        assert np.array_equal(rows_e, (c.ei[0] == tc.BAD_NODE) | (c.ei[1] == tc.BAD_NODE))
        assert np.array_equal(rows_h, tc.neighbourhood(c.ei, n, [tc.BAD_NODE], 1))
    else:
        assert np.array_equal(np.nonzero(rows_e)[0], [tc.BAD_EDGE])
        assert np.array_equal(np.nonzero(rows_h)[0], [c.ei[1][tc.BAD_EDGE]])
    assert np.isnan(h1[rows_h]).all() and np.isnan(e1[rows_e]).all() and 0 < rows_h.sum() <= n // 2
    assert bad and all(k.startswith("processor.0.") for k in bad)
