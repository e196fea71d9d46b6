"""CPU: the float64 restatement of the Sinkhorn gradient convention (sinkhorn_grad_ref in sinkhorn_cases.py, the yardstick
of the HIP backward) against central finite differences of oracle.sinkhorn_divergence.

The convention differentiates only the last extrapolation with the potentials detached; that is the gradient of the divergence
once the Sinkhorn loop has converged (envelope theorem), and the loop with one update per epsilon is only approximately
converged.  At geomloss's default scaling .5 the two differ by 6-19 % (relative 2-norm) on these clouds; as scaling -> 1 (more
updates) the gap closes: 0.6-3.8 % at scaling .95, which the bound below (10 %) covers.  The check is there to catch a wrong sign, a wrong
factor or a swapped potential, which are off by 50 % and more.  The diameter is fixed so that the perturbations cannot move the
epsilon schedule."""
import numpy as np
import pytest

from oracle import epd_oracle as orc
from sinkhorn_cases import sinkhorn_grad_ref


def _fd(x, y, d, scaling, h=1e-6):
    f = lambda a, b: orc.sinkhorn_divergence(a, b, blur=0.05, scaling=scaling, diameter=d)
    gx, gy = np.zeros_like(x), np.zeros_like(y)
    for g, src, is_x in ((gx, x, True), (gy, y, False)):
        for idx in np.ndindex(src.shape):
            p, m = src.copy(), src.copy()
            p[idx] += h
            m[idx] -= h
            g[idx] = (f(p, y) - f(m, y)) / (2 * h) if is_x else (f(x, p) - f(x, m)) / (2 * h)
    return gx, gy


@pytest.mark.parametrize("n,m,seed,d", [(40, 35, 1, 0.5), (30, 50, 2, 0.4), (25, 25, 4, 0.3)])
def test_restated_gradient_against_finite_differences(n, m, seed, d):
    rng = np.random.default_rng(seed)
    x = 0.5 + 0.05 * rng.standard_normal((n, 3))
    y = 0.53 + 0.06 * rng.standard_normal((m, 3))
    errs = []
    for scaling in (0.5, 0.95):
        S, dx, dy = sinkhorn_grad_ref(x, y, blur=0.05, scaling=scaling, diameter=d)
        assert abs(S - orc.sinkhorn_divergence(x, y, blur=0.05, scaling=scaling, diameter=d)) <= 1e-12
        fx, fy = _fd(x, y, d, scaling)
        errs.append([np.linalg.norm(g - f) / np.linalg.norm(f) for g, f in ((dx, fx), (dy, fy))])
    assert max(errs[1]) < 0.10, errs
    assert max(errs[0]) < 0.30, errs            # the unconverged default schedule, for the record
    assert all(e1 < e0 for e0, e1 in zip(*errs)), errs   # and the gap closes as the loop converges
