"""The cases of sinkhorn_cases.py on the CPU: each case is in the regime its name and its `want` say (measured on the arrays), the
list covers what it was written to cover, and the kernels' arithmetic restated in numpy float32 (sinkhorn_cases.f32_restatement)
meets the GPU test's bars against the float64 references for every case -- so that a bar missed on the GPU is the kernel's doing
(__expf, the summation order, a wrong index) and not float32's or the case's.  Seeds and shapes were fixed here, under these
conditions, not by looking at GPU results."""
import numpy as np
import pytest

import sinkhorn_cases as sc


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_in_its_regime(name):
    c = sc.BY_NAME[name]
    r = sc.check_case(c)
    assert c.diameter is None and 0.0 < c.scaling < 1.0 and c.blur > 0.0
    assert r["n_eps"] == 2 + int(max(0, np.ceil((2 * np.log(c.blur) - 2 * np.log(c.d)) / (2 * np.log(c.scaling)))))   # the kernels' count


def test_cases_cover_the_list():
    R = {n: sc.regime(c) for n, c in sc.BY_NAME.items()}
    # schedules: the long one, the short ones, the shortest (both ends of sk_eps's branches at once, the smallest even count)
    assert R["scaling_0.9"]["n_eps"] == 25 and abs(sc.BY_NAME["scaling_0.9"].d - 0.55) < 1e-6
    assert {sc.BY_NAME[n].scaling for n in sc.NAMES} >= {0.9, 0.5, 0.2, 0.1}
    assert R["shortest_shifted"]["n_eps"] == R["shortest_coincident"]["n_eps"] == 2
    assert sorted(n for n in sc.NAMES if sc.BY_NAME[n].noise) == ["shortest_coincident"]
    assert {r["n_eps"] & 1 for r in R.values()} == {0, 1}                        # both ping-pong sets end up as the last one
    # A = d^2 / (2 blur^2): from below 1 to 4e4, the other Sinkhorn tests' ~80 in between
    A = sorted(r["A"] for r in R.values())
    assert A[0] < 0.5 and A[-1] > 4e4 and sum(1.5e3 < a < 2.5e4 for a in A) >= 3
    assert abs(sc.BY_NAME["blur_0.003"].d - 0.6) < 1e-6 and abs(sc.BY_NAME["blur_0.01"].d - 0.6) < 1e-6
    # sizes
    sizes = {(r["n"], r["m"]) for r in R.values()}
    assert sizes >= {(1, 300), (300, 1), (2, 65), (65, 2), (5, 64), (17, 63), (16, 129), (4, 4)}
    assert {r["m_mod_64"] for r in R.values()} >= {63, 0, 1} and {r["n_mod_4"] for r in R.values()} == {0, 1, 2, 3}
    assert any(r["n"] <= sc.SK_WG_ROWS for r in R.values()) and any(r["n"] == sc.SK_WG_ROWS + 1 for r in R.values())
    assert max(max(r["n"], r["m"]) for r in R.values()) <= 600
    # every (blur, scaling) the self-loss test runs
    assert len(sc.BLUR_SCALING) == 7
    assert set(sc.DIAMETER_CASES) | set(sc.SINGLE_POINT) | set(sc.PERMUTED) <= set(sc.NAMES)


def test_batches_are_in_their_regime():
    bs = sc.batches()
    for name in ("b6_per_pair_y", "b6_shared_y"):
        b = bs[name]
        assert b.X.shape == (6, 130, 3) and b.shared == (name == "b6_shared_y") and b.Y.shape[-2:] == (97, 3)
        n_eps = [sc.regime(b.pair(i))["n_eps"] for i in range(6)]
        assert min(n_eps) == 2 and len(set(n_eps)) == 6 and n_eps.index(max(n_eps)) not in (0, 5), (name, n_eps)   # 2 .. the longest, mixed
        assert n_eps[0] == 2 and max(n_eps) >= 10
    b = bs["b1"]
    assert b.X.shape == (1, 150, 3) and b.Y.shape == (1, 131, 3) and not b.shared
    b = bs["b70_shared_y"]
    assert b.X.shape == (70, 40, 3) and b.Y.shape == (33, 3) and b.shared
    assert len({sc.regime(b.pair(i))["n_eps"] for i in range(70)}) >= 4
    for b in bs.values():
        assert b.X.dtype == np.float32 and b.Y.dtype == np.float32 and b.w.shape == (b.X.shape[0],) and (b.w > 0.1).all()


def test_self_cloud():
    x, shifted = sc.self_cloud()
    assert x.shape == (257, 3) and abs(sc.bbox_diameter(x, x) - 0.6) < 1e-6 and not np.array_equal(x, shifted)


@pytest.mark.parametrize("name", sc.NAMES)
def test_float32_alone_meets_the_gpu_bars(name):
    """The restatement against oracle.sinkhorn_divergence / sinkhorn_grad_ref at the GPU test's bars.  Measured over the list:
    S within 1.4e-6 relative (subset; 3.5e-7 elsewhere), gradients within 2.7e-5 of max |ref| (blur_0.003; far_blobs_blur_0.01
    1.3e-5), row sums of the one-pass gradient weights between 0.9971 and 1.0010 at A = 4.4e4 and within 1e-4 of 1 below A = 2e3.
    The noise-level case is held to half of its floors: its measured error, recorded next to them, is a quarter, and the sum of
    600 roundings that it is moves with the last bit of the host's exp."""
    c = sc.BY_NAME[name]
    S, dx, dy = sc.reference(name)
    got = sc.f32_restatement(c.x, c.y, c.blur, c.scaling, c.diameter)
    assert got["n_eps"] == sc.regime(c)["n_eps"]
    part = 0.5 if c.noise else 1.0
    assert abs(got["S"] - S) <= part * sc.forward_bar(c, S), (name, got["S"], S)
    for what, g, ref in (("dx", got["dx"], dx), ("dy", got["dy"], dy)):
        assert g.shape == ref.shape and np.isfinite(g).all(), (name, what)
        assert np.abs(g - ref).max() <= part * sc.grad_bar(c, ref), (name, what, np.abs(g - ref).max(), np.abs(ref).max())
    if c.noise:
        assert abs(S) < sc.NOISE_FWD_F32_ERR and np.abs(dx).max() < 100 * sc.NOISE_GRAD_FLOOR      # at noise level indeed
    else:
        assert abs(S) > 1e4 * 2.0 ** -24 * c.blur ** 2                # far above the rounding of a potential
    # the one-pass gradient's premise: q is the row's log-normaliser, the weights of a row sum to 1 within float32's cancellation
    lo, hi = got["W"]
    tol = 4e-3 if sc.regime(c)["A"] > 2.5e4 else 2e-4
    assert 1 - tol <= lo <= hi <= 1 + tol, (name, lo, hi)


@pytest.mark.parametrize("name", ["b6_per_pair_y", "b6_shared_y", "b70_shared_y"])
def test_float32_alone_meets_the_gradient_bar_on_the_batches(name):
    """The batch tests compare the device with itself (single calls); this holds their pairs' gradients reachable as well.  The
    forward is not held: pair 0 of the B = 6 batches (n_eps = 2, clouds 0.03 across) has a divergence of 1e-5, at noise level."""
    b = sc.batches()[name]
    for i in range(0, b.X.shape[0], 1 if b.X.shape[0] <= 6 else 9):
        c = b.pair(i)
        _, dx, dy = sc.pair_reference(c)
        got = sc.f32_restatement(c.x, c.y, c.blur, c.scaling)
        for what, g, ref in (("dx", got["dx"], dx), ("dy", got["dy"], dy)):
            assert np.abs(g - ref).max() <= sc.GRAD_REL * np.abs(ref).max(), (name, i, what)


def test_restatement_knows_its_own_mutations():
    """The restatement, and with it the bars, tell a schedule at another scaling from the case's own."""
    c = sc.BY_NAME["scaling_0.2"]
    S, dx, _ = sc.reference(c.name)
    wrong = sc.f32_restatement(c.x, c.y, c.blur, 0.5)
    assert abs(wrong["S"] - S) > 100 * sc.forward_bar(c, S)
    assert np.abs(wrong["dx"] - dx).max() > 10 * sc.grad_bar(c, dx)
