"""Differentiable SamplesLoss on the MI355X: gradients of the debiased Sinkhorn divergence from the HIP backward
(gm_sinkhorn_divergence_batched_backward) against a float64 torch restatement of geomloss's convention, the batched call
against single calls, the unchanged forward, edge cases, and composition with EncProcDecGNN's autograd Function.

The convention (geomloss tensorized backend, unpinned like the forward): the potentials are detached and only the last
extrapolation is differentiated, with the right-hand cloud of every cost matrix detached.  sinkhorn_cases.sinkhorn_grad_ref restates it; its
own check against finite differences of oracle.sinkhorn_divergence is tests/test_sinkhorn_grad_reference.py."""
import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
from sinkhorn_cases import sinkhorn_grad_ref
from gpu_support import dev, to_dev as _t

pytestmark = pytest.mark.gpu


def _clouds(n, m, seed):
    rng = np.random.default_rng(seed)
    x = (0.5 + 0.05 * rng.standard_normal((n, 3))).astype(np.float32)
    y = (0.52 + 0.06 * rng.standard_normal((m, 3))).astype(np.float32)
    return x, y


def _loss(**kw):
    from gnn_manip_amd.losses import SamplesLoss
    return SamplesLoss(loss="sinkhorn", p=2, blur=kw.pop("blur", .05), **kw)


def _grads(loss, x, y, dev, wrt):
    xt, yt = _t(x, dev).requires_grad_("x" in wrt), _t(y, dev).requires_grad_("y" in wrt)
    loss(xt, yt).backward()
    return (xt.grad.cpu().numpy() if "x" in wrt else None), (yt.grad.cpu().numpy() if "y" in wrt else None)


def test_loss_has_grad_fn_and_backward_fills_x_grad(dev):
    x, y = _clouds(300, 280, 7)
    xt = _t(x, dev).requires_grad_()
    out = _loss()(xt, _t(y, dev))
    assert out.grad_fn is not None and out.dim() == 0
    out.backward()
    g = xt.grad
    assert g is not None and g.shape == xt.shape and g.dtype == torch.float32
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0.0


@pytest.mark.parametrize("n,m,seed,blur", [(150, 130, 1, .05), (1000, 777, 2, .05), (3, 5, 3, .05), (2500, 2500, 4, .05),
                                           (900, 1100, 13, .02)])
def test_grad_vs_float64_reference(dev, n, m, seed, blur):
    """dx and dy -- each alone and both together -- against sinkhorn_grad_ref: per element 1e-4 of max |ref|.  The gradient is a
    difference of two softmax barycentres of a row, each a ratio of float32 sums over up to 2500 __expf terms whose arguments carry
    the float32 potentials of ~20 Sinkhorn iterations divided by eps (= blur^2): the potentials' relative error, ~1e-6, becomes
    a relative error of the weights of that order, and the difference of the two barycentres is an order of magnitude smaller
    than either -- 1e-4 of the largest element leaves that margin, and a wrong potential, weight or cloud is off by far more."""
    x, y = _clouds(n, m, seed)
    _, rdx, rdy = sinkhorn_grad_ref(x, y, blur=blur)
    loss = _loss(blur=blur)
    gx, _ = _grads(loss, x, y, dev, "x")
    _, gy = _grads(loss, x, y, dev, "y")
    bx, by = _grads(loss, x, y, dev, "xy")
    for what, got, ref in (("dx", gx, rdx), ("dy", gy, rdy), ("dx both", bx, rdx), ("dy both", by, rdy)):
        assert got.shape == ref.shape and np.isfinite(got).all(), what
        err = np.abs(got - ref).max() / np.abs(ref).max()
        assert err <= 1e-4, (what, err)
    np.testing.assert_array_equal(gx, bx)
    np.testing.assert_array_equal(gy, by)


def test_batched_gradients_equal_single_calls(dev):
    """grad of (w * loss.batched(X, Y)).sum(): dX[b] (and dY[b], one cloud per pair) is bit-equal to w[b] times the gradient of
    the single call on pair b -- the same kernel on the same pair, whatever schedule the batch's other pairs have.  With y shared
    by the batch, dy is the sum over the pairs, reduced in fixed order: within 1e-6 of the float64 sum, and identical bits from
    run to run."""
    rng = np.random.default_rng(31)
    n, m, B = 500, 430, 5
    spreads = [0.02, 0.3, 0.05, 1.0, 0.1]
    X = np.stack([(0.5 + sp * rng.standard_normal((n, 3))).astype(np.float32) for sp in spreads])
    Y = np.stack([(0.5 + (sp + 0.01) * rng.standard_normal((m, 3))).astype(np.float32) for sp in spreads])
    y = (0.52 + 0.04 * rng.standard_normal((m, 3))).astype(np.float32)
    w = rng.uniform(0.2, 2.0, B).astype(np.float32)
    wt = _t(w, dev)
    loss = _loss()

    Xt, Yt = _t(X, dev).requires_grad_(), _t(Y, dev).requires_grad_()
    (wt * loss.batched(Xt, Yt)).sum().backward()
    for b in range(B):
        gx, gy = _grads(loss, X[b], Y[b], dev, "xy")
        np.testing.assert_array_equal(Xt.grad[b].cpu().numpy(), (wt[b] * _t(gx, dev)).cpu().numpy(), err_msg=f"dX[{b}]")
        np.testing.assert_array_equal(Yt.grad[b].cpu().numpy(), (wt[b] * _t(gy, dev)).cpu().numpy(), err_msg=f"dY[{b}]")

    def shared():
        Xs, ys = _t(X, dev).requires_grad_(), _t(y, dev).requires_grad_()
        (wt * loss.batched(Xs, ys)).sum().backward()
        return Xs.grad.cpu().numpy(), ys.grad.cpu().numpy()

    dX1, dy1 = shared()
    dX2, dy2 = shared()
    assert dX1.tobytes() == dX2.tobytes() and dy1.tobytes() == dy2.tobytes()
    ref = np.zeros((m, 3))
    for b in range(B):
        gx, gy = _grads(loss, X[b], y, dev, "xy")
        np.testing.assert_array_equal(dX1[b], (wt[b] * _t(gx, dev)).cpu().numpy(), err_msg=f"dX[{b}], shared y")
        ref += np.float64(w[b]) * gy.astype(np.float64)
    assert np.abs(dy1 - ref).max() <= 1e-6 * np.abs(ref).max(), np.abs(dy1 - ref).max() / np.abs(ref).max()


def test_forward_unchanged_and_planner_calls_share_the_workspace(dev):
    """The value of a grad-requiring call is bit-equal to the same call without grad; calls under torch.no_grad() (the
    planner's) reuse the loss's workspace, and a grad-requiring call leaves it alone."""
    rng = np.random.default_rng(41)
    X = (0.5 + 0.05 * rng.standard_normal((4, 600, 3))).astype(np.float32)
    y = (0.53 + 0.06 * rng.standard_normal((550, 3))).astype(np.float32)
    loss = _loss()
    with torch.no_grad():
        plain = loss.batched(_t(X, dev), _t(y, dev))
        ws = loss._ws
        again = loss.batched(_t(X, dev), _t(y, dev))
        assert loss._ws is ws and plain.grad_fn is None
        assert loss.batched(_t(X, dev).requires_grad_(), _t(y, dev)).grad_fn is None   # no_grad wins over requires_grad
    assert plain.cpu().numpy().tobytes() == again.cpu().numpy().tobytes()
    for wrt in ("x", "y", "xy"):
        Xt, yt = _t(X, dev).requires_grad_("x" in wrt), _t(y, dev).requires_grad_("y" in wrt)
        got = loss.batched(Xt, yt)
        assert got.grad_fn is not None and loss._ws is ws
        assert got.detach().cpu().numpy().tobytes() == plain.cpu().numpy().tobytes(), wrt
    one = loss(_t(X[2], dev).requires_grad_(), _t(y, dev))
    assert one.detach().cpu().numpy().tobytes() == plain[2].cpu().numpy().tobytes()
    assert loss(_t(X[2], dev), _t(y, dev)).cpu().numpy().tobytes() == plain[2].cpu().numpy().tobytes()


def test_grad_edge_cases(dev):
    """The `diameter=` path gives the default path's gradients when both use the same diameter; identical one-point clouds
    (loss 0 by definition) give zero gradient; a non-finite coordinate (reported only on the default path, propagated on the
    `diameter=` path) gives a NaN gradient for its own pair only."""
    x, y = _clouds(400, 350, 51)
    both = np.concatenate((x, y))
    d = float(np.sqrt(((both.max(0) - both.min(0)).astype(np.float32) ** 2).sum(dtype=np.float32)))   # the plan kernel's diameter
    gx, gy = _grads(_loss(), x, y, dev, "xy")
    dx, dy = _grads(_loss(diameter=d), x, y, dev, "xy")
    np.testing.assert_array_equal(gx, dx)
    np.testing.assert_array_equal(gy, dy)

    p = np.array([[0.4, 0.5, 0.6]], np.float32)
    for a, b in ((p, p), (np.repeat(p, 3, 0), np.repeat(p, 2, 0))):
        at, bt = _t(a, dev).requires_grad_(), _t(b, dev).requires_grad_()
        out = _loss()(at, bt)
        out.backward()
        assert float(out.detach()) == 0.0
        assert not at.grad.any() and not bt.grad.any()

    X = np.stack((x, x + 0.01, x - 0.02))
    Y = np.stack((y, y, y + 0.01))
    X[1, 17, 1] = np.nan
    loss = _loss(diameter=1.0)
    Xt, Yt = _t(X, dev).requires_grad_(), _t(Y, dev).requires_grad_()
    vals = loss.batched(Xt, Yt)
    vals.sum().backward()
    v = vals.detach().cpu().numpy()
    dX, dY = Xt.grad.cpu().numpy(), Yt.grad.cpu().numpy()
    assert np.isnan(v[1]) and np.isfinite(v[[0, 2]]).all()
    assert np.isnan(dX[1]).all() and np.isnan(dY[1]).all()
    assert np.isfinite(dX[[0, 2]]).all() and np.isfinite(dY[[0, 2]]).all()
    for b in (0, 2):
        gx, gy = _grads(loss, X[b], Y[b], dev, "xy")
        np.testing.assert_array_equal(dX[b], gx)
        np.testing.assert_array_equal(dY[b], gy)


def test_end_to_end_with_the_model_and_a_gradient_flow(dev):
    """A Sinkhorn loss on an EncProcDecGNN prediction: backward() through both autograd Functions gives the parameter gradients
    of out.backward(g) with g = the HIP dS/dx of the detached prediction fed by hand.  Then a 20-step gradient flow
    x <- x - N lr dS/dx on a cloud: the loss decreases at every step."""
    from gnn_manip_amd import EncProcDecGNN, scene
    from conftest import BOUNDS, CART, CTRL, MAT, STATS
    obs = scene.make_scene(300, seed=61, side=0.05)
    nodes, ea, s, r, _ = orc.process(obs, None, stats=STATS, bounds=BOUNDS, conn_r=0.015, cartesian_idx=CART, material_idx=MAT,
                                     control_idx=CTRL)
    params = orc.init_params(25, 4, 3, 128, 2, 2, 61)
    model = EncProcDecGNN(25, 4, 3, 128, 2, 2)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    model = model.to(dev)
    args = (_t(nodes, dev), _t(ea, dev), _t(np.stack((s, r)), dev))
    rng = np.random.default_rng(62)
    loss = _loss()

    out = model(*args)
    target = (out.detach() + _t((0.3 * rng.standard_normal(tuple(out.shape))).astype(np.float32), dev)).contiguous()
    loss(out, target).backward()
    composed = {k: p.grad.clone() for k, p in model.named_parameters()}
    model.zero_grad()
    out = model(*args)
    xd = out.detach().clone().requires_grad_()
    loss(xd, target).backward()
    out.backward(xd.grad)
    assert any(float(g.abs().max()) > 0.0 for g in composed.values())
    for k, p in model.named_parameters():
        assert torch.equal(composed[k], p.grad), k

    x = _t((0.45 + 0.04 * rng.standard_normal((300, 3))).astype(np.float32), dev)
    y = _t((0.55 + 0.06 * rng.standard_normal((260, 3))).astype(np.float32), dev)
    lr, vals = 0.5, []
    for _ in range(21):
        xg = x.clone().requires_grad_()
        val = loss(xg, y)
        val.backward()
        vals.append(float(val.detach()))
        x = x - x.shape[0] * lr * xg.grad
    assert all(b < a for a, b in zip(vals, vals[1:])), vals
    assert vals[-1] < 0.01 * vals[0], vals
