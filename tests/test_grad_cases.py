"""CPU: the cases of tests/grad_cases.py are in their regimes, and its float64 restatement of the rollout step is the oracle's
forward with gradients that central finite differences confirm.

Forward bound: oracle/epd_oracle.py computes in float32, the restatement in float64 on the same float32 inputs; each function is
at most four float32 roundings deep on values no larger than the result's (or the position's) magnitude, so they agree within
8 x 2^-24 of the tensor's largest magnitude -- the boundary features carry the position's rounding divided by r, bounded by the
same figure with the position (<= 1) over r in place of the result.
Finite differences: float64 central differences with step h have a rounding error of about 2^-52 |f| / h and no truncation error
where the function is piecewise linear; the bound 1e-5 of the largest gradient entry leaves two orders of magnitude over that."""
import numpy as np
import pytest
import torch

from conftest import BOUNDS, STATS
from oracle import epd_oracle as orc
import grad_cases as gc
import width_cases as wc

EPS32 = 2.0 ** -24


def _close32(got, ref, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(float(np.abs(ref).max()), scale or 0.0)
    assert np.abs(got - ref).max() <= 8 * EPS32 * scale, (float(np.abs(got - ref).max()), scale)


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_layout_states_are_in_their_regime_and_match_the_oracle(name):
    L = wc.LAYOUTS[name]
    obs = gc.state(name)
    ei = gc.radius_edges(name)
    reg = gc.regime(obs, L, ei)
    print(name, reg)
    gc.assert_in_regime(reg, obs.shape[1])
    nodes = gc.node_features(gc.t64(obs), L).numpy()
    _close32(nodes, orc.compute_nodes(obs, STATS, BOUNDS, gc.R, L.cart_idx, [L.mat], L.ctrl_idx), scale=1.0 / gc.R)
    ea = gc.edge_features(gc.t64(obs[-1][:, L.cart:L.cart + 3]), torch.tensor(ei[0]), torch.tensor(ei[1])).numpy()
    _close32(ea, orc.get_edges_displacement(obs[-1][:, L.cart:L.cart + 3], ei[0], ei[1], gc.R))
    pred = gc.weights((obs.shape[1], 3), 5)
    nxt = gc.integrate(gc.t64(pred), gc.t64(obs), L).numpy()
    _close32(nxt, orc.get_position_from_prediction(STATS, L.cart_idx, pred, obs))


@pytest.mark.parametrize("name", ["step_a", "step_b"])
def test_step_states_are_in_their_regime(name):
    L = wc.LAYOUTS["default"]
    obs = gc.step_state(name)
    reg = gc.regime(obs, L, gc.radius_edges(name, "default", gc.STEP_N, gc.STEP_SIDE))
    print(name, reg)
    gc.assert_in_regime(reg, obs.shape[1])


def test_multigraph_is_in_its_regime():
    pos, ei = gc.multigraph()
    d = np.linalg.norm((pos[ei[0]].astype(np.float64) - pos[ei[1]]) / gc.R, axis=1)
    assert (ei[0] == ei[1]).sum() >= 100 and d[ei[0] != ei[1]].min() >= 1e-6
    deg = np.bincount(ei[0], minlength=len(pos)) + np.bincount(ei[1], minlength=len(pos))
    assert (deg == 0).sum() >= 1 and deg.max() >= 700


@pytest.mark.parametrize("name,with_target", [("default", True), ("moved", True), ("moved", False), ("no_control", True)])
def test_restated_state_updates_are_the_oracles(name, with_target):
    """Against width_cases.state_pre / state_post, themselves held to the oracle's rollout step by test_width_cases.py."""
    L = wc.LAYOUTS[name]
    obs = gc.state(name)
    rows = gc.rigid_rows(obs, L)
    target = gc.rigid_target(obs, L, 3) if with_target else None
    tt = None if target is None else gc.t64(target)
    pre = gc.state_pre(gc.t64(obs), L, torch.tensor(rows), tt)
    ref_pre = wc.state_pre(obs, L, target) if L.ctrl >= 0 else np.asarray(obs)
    _close32(pre.numpy(), ref_pre)
    nxt = gc.weights((obs.shape[1], 3), 9)
    post = gc.state_post(gc.t64(ref_pre), L, gc.t64(nxt), torch.tensor(rows), tt)
    assert np.array_equal(post.numpy(), wc.state_post(ref_pre, L, nxt, target).astype(np.float64))


def _fd_check(f, x, coords, h):
    """d f / d x at the flat coordinates `coords` by central differences against autograd."""
    x = x.clone().requires_grad_(True)
    g, = torch.autograd.grad(f(x), x)
    g = g.flatten()
    flat = x.detach().flatten()
    fd = []
    for c in coords:
        xp, xm = flat.clone(), flat.clone()
        xp[c] += h
        xm[c] -= h
        fd.append((float(f(xp.view_as(x))) - float(f(xm.view_as(x)))) / (2 * h))
    fd = np.asarray(fd)
    got = g[coords].numpy()
    assert np.abs(got - fd).max() <= 1e-5 * float(g.abs().max()), (np.abs(got - fd).max(), float(g.abs().max()))
    return g


@pytest.mark.parametrize("name", ["default", "k2", "moved", "no_control"])
def test_feature_gradients_match_finite_differences(name):
    L = wc.LAYOUTS[name]
    obs = gc.t64(gc.state(name))
    ei = torch.tensor(gc.radius_edges(name))
    rng = np.random.default_rng(11)
    k, n, D = obs.shape
    w_n = gc.t64(gc.weights((n, L.node_dim), 1))
    # position columns of rows with unclamped boundary features, the particle alone at the wall, and random coordinates
    u = gc.unclamped_boundary(gc.state(name), L)
    rows = list(np.nonzero((np.abs(u) < 1).any(axis=1))[0][:6]) + [gc.ALONE]
    coords = [((k - 1) * n + r) * D + L.cart + a for r in rows for a in range(3)]
    coords += [c for c in rng.integers(0, obs.numel(), 40) if c % D != L.mat]     # the material column is a label: no gradient
    _fd_check(lambda o: (gc.node_features(o, L) * w_n).sum(), obs, coords, 1e-9)
    pos = obs[-1][:, L.cart:L.cart + 3].contiguous()
    w_e = gc.t64(gc.weights((ei.shape[1], 4), 2))
    _fd_check(lambda p: (gc.edge_features(p, ei[0], ei[1]) * w_e).sum(), pos, list(rng.integers(0, pos.numel(), 40)) + [3 * gc.ALONE], 1e-9)
    w_p = gc.t64(gc.weights((n, 3), 3))
    pred = gc.t64(gc.weights((n, 3), 4))
    _fd_check(lambda o: (gc.integrate(pred, o, L) * w_p).sum(), obs, list(rng.integers(0, obs.numel(), 30)), 1e-7)
    _fd_check(lambda q: (gc.integrate(q, obs, L) * w_p).sum(), pred, list(rng.integers(0, pred.numel(), 10)), 1e-3)


def test_step_gradients_match_finite_differences_along_directions():
    """The whole step on a fixed edge list: the directional derivative along seeded directions in obs (position and control
    columns) and in rigid_target.  The model has ReLU kinks: about 5e6 hidden units see the step, with pre-activations of order
    one, so a step of 1e-9 in positions (5e-7 of a velocity feature) crosses a handful of them and a step of 1e-11 on average
    0.05.  At 1e-11 the rounding error of the difference is about 2^-52 |loss| / h = 1e-5 of |g . v| here; the bound is 1e-4."""
    L = wc.LAYOUTS["default"]
    obs_np = gc.step_state("step_a")
    rows = torch.tensor(gc.rigid_rows(obs_np, L))
    ei = torch.tensor(gc.radius_edges("step_a", "default", gc.STEP_N, gc.STEP_SIDE))
    p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in orc.init_params(*gc.STEP_DIMS, 841).items()}
    w_o = gc.t64(gc.weights(obs_np.shape, 6))
    w_p = gc.t64(gc.weights((obs_np.shape[1], 3), 7))

    def loss(o, t):
        nxt, pred = gc.step(p64, o, L, rows, t, ei, gc.STEP_DIMS[4], gc.STEP_DIMS[5])
        return (nxt * w_o).sum() + (pred * w_p).sum()

    obs = gc.t64(obs_np, True)
    tgt = gc.t64(gc.rigid_target(obs_np, L, 3), True)
    g_o, g_t = torch.autograd.grad(loss(obs, tgt), (obs, tgt))
    assert float(g_t.abs().max()) > 0 and float(g_o[-1][:, L.ctrl:L.ctrl + 3].abs().max()) > 0
    rng = np.random.default_rng(12)
    h = 1e-11
    for _ in range(3):
        v_o = np.zeros(obs_np.shape)
        v_o[:, :, L.cart:L.cart + 3] = rng.standard_normal(obs_np.shape[:2] + (3,))
        v_o[-1][:, L.ctrl:L.ctrl + 3] = rng.standard_normal((obs_np.shape[1], 3))
        v_o, v_t = gc.t64(v_o), gc.t64(rng.standard_normal(tuple(tgt.shape)))
        with torch.no_grad():
            fd = (float(loss(obs + h * v_o, tgt + h * v_t)) - float(loss(obs - h * v_o, tgt - h * v_t))) / (2 * h)
        an = float((g_o * v_o).sum() + (g_t * v_t).sum())
        print("directional derivative", fd, an, abs(fd - an) / abs(an))
        assert abs(fd - an) <= 1e-4 * abs(an), (fd, an)
