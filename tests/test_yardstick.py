"""CPU: the gradient rule of tests/yardstick.py at its edge, and the ReLU flip allowance core of oracle/torch_epd.py
(near_zero_units, flip_bounds) on a network small enough that the allowance is known in closed form."""
import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
from oracle import torch_epd
import train_cases
import yardstick

F64 = torch.float64


# ------------------------------------------------------------------------------------------ 1. a network with a known allowance
def _tiny(z_over_rms, x=0.7):
    """y = w2 . relu(w1 x + b) on one row, loss = y.  The last unit is far from zero and sets the Linear's rms; unit u < last has
    z_u = z_over_rms[u] x rms (b is solved for that).  Returns (tape, leaves (w1, b, x), w2)."""
    h = len(z_over_rms) + 1
    w1 = torch.tensor([[0.9], [-1.3], [0.4]][:h], dtype=F64)
    w2 = torch.tensor([[1.7, -0.6, 2.2][:h]], dtype=F64)
    r = np.asarray(z_over_rms, np.float64)
    rms = 1.0 / np.sqrt(h - (r ** 2).sum())          # rms^2 = (sum_u (r_u rms)^2 + 1) / h with the last unit at z = 1
    z = torch.tensor(np.append(r * rms, 1.0), dtype=F64)
    xt = torch.tensor([[x]], dtype=F64, requires_grad=True)
    b = (z - w1[:, 0] * x).clone().requires_grad_(True)
    w1.requires_grad_(True)
    p = {"m.0.weight": w1, "m.0.bias": b, "m.2.weight": w2, "m.2.bias": torch.zeros(1, dtype=F64)}
    tape = []
    torch_epd._mlp_taped(p, "m", xt, 1, False, tape).sum().backward(retain_graph=True)
    zz = tape[0][0].detach().flatten()
    assert torch.allclose(zz[:-1] / zz.pow(2).mean().sqrt(), torch.tensor(r), rtol=1e-9, atol=0)       # the construction holds
    return tape, (w1, b, xt), w2.detach()


def test_flip_bounds_of_one_near_zero_unit_in_closed_form():
    x = 0.7
    tape, leaves, w2 = _tiny([1e-7], x)
    units = torch_epd.near_zero_units(tape)
    assert [(t, q) for _, t, q in units] == [(0, 0)] and abs(units[0][0] - 1e-7) <= 1e-16
    d_w1, d_b, d_x = torch_epd.flip_bounds(tape, units, leaves)
    g = abs(float(w2[0, 0]))                                   # |d loss / d a_0|
    assert d_w1.shape == (2, 1) and d_b.shape == (2,) and d_x.shape == (1, 1)
    assert abs(float(d_w1[0, 0]) - g * abs(x)) <= 1e-15 and float(d_w1[1, 0]) == 0.0
    assert abs(float(d_b[0]) - g) <= 1e-15 and float(d_b[1]) == 0.0
    assert abs(float(d_x[0, 0]) - g * 0.9) <= 1e-15           # |w1_0| = 0.9


def test_a_unit_a_thousandth_of_the_rms_from_zero_gets_no_allowance():
    tape, leaves, _ = _tiny([1e-3])
    units = torch_epd.near_zero_units(tape)
    assert units == []
    assert all(float(v.abs().max()) == 0.0 for v in torch_epd.flip_bounds(tape, units, leaves))


def test_max_units_keeps_the_unit_closest_to_zero():
    tape, _, _ = _tiny([3e-7, 1e-7])
    both = torch_epd.near_zero_units(tape)
    assert [q for _, _, q in both] == [1, 0]                   # the closest first
    assert [q for _, _, q in torch_epd.near_zero_units(tape, max_units=1)] == [1]
    empty = [(torch.zeros((0, 3), dtype=F64),) * 2, (torch.zeros((4, 3), dtype=F64),) * 2]
    assert torch_epd.near_zero_units(empty) == []              # no rows, and rms == 0: skipped


# ------------------------------------------------------------------------------------------ 2. the rule at its edge
G64 = np.array([[2.0, -0.5, 0.25], [1.0, 0.0, -1.5]])
SCALE = 2.0


def _off(factor, at=(1, 1), tol=yardstick.GRAD_TOL):
    got = G64.copy()
    got[at] += factor * tol * SCALE
    return got


def test_tolerance_is_the_floor_or_four_times_float32s_error():
    assert yardstick.tolerance(G64, G64) == (yardstick.GRAD_TOL, SCALE, 0.0)
    g32 = G64.copy()
    g32[0, 1] += 1e-3 * SCALE
    tol, scale, e32 = yardstick.tolerance(G64, g32)
    assert scale == SCALE and abs(e32 - 1e-3) <= 1e-15 and abs(tol - 4e-3) <= 1e-15
    yardstick.within("4 x float32", _off(0.999, tol=tol), G64, g32)
    with pytest.raises(AssertionError):
        yardstick.within("4 x float32", _off(1.001, tol=tol), G64, g32)


def test_rule_passes_just_inside_and_fails_just_outside():
    yardstick.within("inside", _off(0.999), G64, G64)
    with pytest.raises(AssertionError):
        yardstick.within("outside", _off(1.001), G64, G64)
    assert yardstick.compare({"a": _off(0.999)}, {"a": G64}, {"a": G64})[1] is None
    with pytest.raises(AssertionError):
        yardstick.compare({"a": _off(1.001)}, {"a": G64}, {"a": G64})


def test_array_allowance_holds_every_element_to_its_own_and_a_scalar_holds_the_tensor():
    got = _off(3.0, at=(1, 1))                                 # three times the bound, where the allowance is zero
    large = 10.0 * yardstick.GRAD_TOL * SCALE
    array = np.zeros_like(G64)
    array[0, 2] = large                                        # ... and a large allowance elsewhere
    calls = []

    def allow_array():
        calls.append(1)
        return array, 1
    with pytest.raises(AssertionError):
        yardstick.within("array", got, G64, G64, allow_array)
    assert calls == [1]
    yardstick.within("scalar", got, G64, G64, lambda: (large, 1))                       # the per-tensor rule
    with pytest.raises(AssertionError):
        yardstick.compare({"a": got}, {"a": G64}, {"a": G64}, lambda: ({"a": array}, 1))
    worst, after = yardstick.compare({"a": got}, {"a": G64}, {"a": G64}, lambda: ({"a": large}, 1))
    assert worst[0] == "a" and abs(worst[1] - 3.0) <= 1e-9 and abs(after[1] - 3.0 / 11.0) <= 1e-9
    array[1, 1] = large                                        # the element's own allowance: within
    yardstick.within("array", got, G64, G64, lambda: (array, 1))
    yardstick.within("part", got[1:], G64[1:], G64[1:], lambda: (array, 1), part=slice(1, None))
    never = lambda: pytest.fail("the allowance is computed only where the plain bound fails")
    yardstick.within("lazy", _off(0.5), G64, G64, never)
    yardstick.compare({"a": _off(0.5)}, {"a": G64}, {"a": G64}, never)


def test_nan_and_shape_mismatch_fail():
    got = G64.copy()
    got[0, 0] = np.nan
    for bad in (got, G64[:, :2], G64.T):
        with pytest.raises(AssertionError):
            yardstick.within("bad", bad, G64, G64, lambda: (np.inf, 0))
        with pytest.raises(AssertionError):
            yardstick.compare({"a": bad}, {"a": G64}, {"a": G64}, lambda: ({"a": np.inf}, 0))
    with pytest.raises(AssertionError):
        yardstick.compare({}, {"a": G64}, {"a": G64})          # a tensor that is missing


def test_lazy_and_bits():
    calls = []
    get = yardstick.lazy(lambda: calls.append(1) or 7)
    assert get() == 7 and get() == 7 and calls == [1]
    assert yardstick.same_bits(np.float32([0.0, 1.5]), torch.tensor([0.0, 1.5]))
    assert not yardstick.same_bits(np.float32([0.0]), np.float32([-0.0]))


# ------------------------------------------------------------------------------------------ 3. the per-tensor reduction
def test_relu_flip_allowance_is_the_maximum_of_flip_bounds_per_parameter():
    """tau = 1e-2, so that this small graph has units to toggle at all (asserted)."""
    dims, seed, tau = (25, 4, 3, 64, 2, 1), 92, 1e-2
    nodes, ea, ei = train_cases.graph(130, 0.3, seed)
    params = orc.init_params(*dims, seed)
    target = np.random.default_rng(seed).standard_normal((nodes.shape[0], dims[2])).astype(np.float32)
    allow, n_units = torch_epd.relu_flip_allowance(params, nodes, ea, ei, target, dims[4], dims[5], tau=tau)
    p = {k: torch.tensor(v, dtype=F64, requires_grad=True) for k, v in params.items()}
    tape = []
    out = torch_epd.epd_forward_taped(p, torch.tensor(nodes, dtype=F64), torch.tensor(ea, dtype=F64), torch.tensor(ei, dtype=torch.int64),
                                      dims[4], dims[5], tape)
    (torch.nn.functional.l1_loss(out, torch.tensor(target, dtype=F64), reduction="sum") / out.shape[0]).backward(retain_graph=True)
    units = torch_epd.near_zero_units(tape, tau)
    assert len(units) == n_units > 0 and units == sorted(units)
    bounds = torch_epd.flip_bounds(tape, units, list(p.values()))
    assert sorted(allow) == sorted(p)
    for name, b in zip(p, bounds):
        assert allow[name] == float(b.max()), name
    assert max(allow.values()) > 0.0
