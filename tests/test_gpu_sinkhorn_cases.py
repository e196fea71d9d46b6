"""The Sinkhorn kernels (csrc/sinkhorn.hip) and their Python wrapper (losses.py) on the cases of sinkhorn_cases.py: epsilon
schedules of 2 to 25 entries at scaling 0.1 to 0.9, A = d^2 / (2 blur^2) from 0.25 to 4.4e4, sizes on the edges of the 4-row /
16-row / 64-lane tiling, degenerate geometry, batches of 1, 6 and 70 pairs, strided / float64 inputs, workspace reuse and the
error paths.

Bars: the project's -- |S - ref| <= 1e-5 |ref| against oracle.sinkhorn_divergence, gradients per element within 1e-4 of max |ref|
against sinkhorn_grad_ref, both float64 -- and, for the one case whose divergence is at float32's noise level, the absolute floors
recorded in sinkhorn_cases.py.  test_sinkhorn_cases.py shows on the CPU that float32 alone meets every one of them.  Where the
device is compared with itself (batch against single calls, `diameter=` against the bounding box, a view against its contiguous
copy) the bar is equal bits."""
import numpy as np
import pytest
import torch

import sinkhorn_cases as sc
from gpu_support import dev, to_dev as _t

pytestmark = pytest.mark.gpu


def _loss(c=None, **kw):
    from gnn_manip_amd.losses import SamplesLoss
    if c is not None:
        kw = {**dict(blur=c.blur, scaling=c.scaling, diameter=c.diameter), **kw}
    return SamplesLoss(loss="sinkhorn", p=2, **kw)


def _run(loss, x, y, dev, wrt="xy"):
    """(S, dS/dx, dS/dy) of one call as numpy float32 (a gradient that was not asked for: None)."""
    xt, yt = _t(x, dev).requires_grad_("x" in wrt), _t(y, dev).requires_grad_("y" in wrt)
    out = loss(xt, yt)
    out.backward()
    return out.detach().cpu().numpy(), (xt.grad.cpu().numpy() if "x" in wrt else None), (yt.grad.cpu().numpy() if "y" in wrt else None)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ every case against float64
@pytest.mark.parametrize("name", sc.NAMES)
def test_case_vs_float64(dev, name):
    """Forward and gradients -- dx alone, dy alone, both -- of every case; dx / dy alone bit-equal to the joint call, the value the
    same bits with and without grad.  Measured on an MI355X: S within 2.6e-6 relative (shortest_shifted; 1.1e-6 subset, below
    4e-7 elsewhere), gradients within 4.2e-5 of max |ref| (blur_0.003 dx; far_blobs_blur_0.01 1.7e-5, blur_0.01 1e-5, below 5e-6
    elsewhere); the noise-level case 9.3e-9 from the reference against its floor of 1.2e-8, its gradients 8.5e-11 against 1.6e-9."""
    c = sc.BY_NAME[name]
    S, rdx, rdy = sc.reference(name)
    loss = _loss(c)
    s_x, gx, none = _run(loss, c.x, c.y, dev, "x")
    s_y, none2, gy = _run(loss, c.x, c.y, dev, "y")
    s_b, bx, by = _run(loss, c.x, c.y, dev, "xy")
    assert none is None and none2 is None
    with torch.no_grad():
        s_plain = loss(_t(c.x, dev), _t(c.y, dev)).cpu().numpy()
    err = abs(float(s_b) - S)
    print(f"\n{name}: S = {float(s_b):.9e}, ref {S:.9e}, |err| = {err:.3e}, bar {sc.forward_bar(c, S):.3e}")
    worst = {}
    for what, got, ref in (("dx", gx, rdx), ("dy", gy, rdy)):
        assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), (name, what)
        worst[what] = float(np.abs(got - ref).max())
        print(f"{name}: {what} max |err| = {worst[what]:.3e}, max |ref| = {np.abs(ref).max():.3e}, bar {sc.grad_bar(c, ref):.3e}")
    assert np.isfinite(s_b) and err <= sc.forward_bar(c, S), (name, float(s_b), S)
    assert _same(s_x, s_b) and _same(s_y, s_b) and _same(s_plain, s_b), name
    assert worst["dx"] <= sc.grad_bar(c, rdx) and worst["dy"] <= sc.grad_bar(c, rdy), (name, worst)
    assert _same(gx, bx) and _same(gy, by), name


@pytest.mark.parametrize("name", sc.SINGLE_POINT)
def test_single_point_cloud_enters_the_other_gradient_exactly(dev, name):
    """dS/dq_j = (1/M) (T_qq(q_j) - T_qp(q_j)), and the barycentre T_qp over a cloud of one point p is p itself.  T_qq depends on q
    and on the schedule alone, so with the diameter named, moving p by t moves M dS/dq_j by -t for every j, up to the rounding of
    the kernel's last steps: (w (q - p)) / w, the subtraction of the self term, the product with 1/M -- 8 * 2^-24 of the operands
    bounds them with room, and a weight or a potential that entered would show at 1e-2.  The single point's own self term is an
    exact zero: its gradient is -(1/1) sum_j w_j (p - q_j) / sum_j w_j, inside the bounding box of q - p."""
    c = sc.BY_NAME[name]
    swap = c.x.shape[0] != 1                     # the single point is y
    p, q = (c.y, c.x) if swap else (c.x, c.y)
    t = np.array([1 / 64, -1 / 32, 1 / 128], np.float32)
    p2 = p + t
    loss = _loss(c, diameter=1.0)
    out = []
    for pp in (p, p2):
        _, gx, gy = _run(loss, *((q, pp) if swap else (pp, q)), dev)
        out.append((gy, gx) if swap else (gx, gy))
    m = q.shape[0]
    moved = np.float64(m) * (out[1][1].astype(np.float64) - out[0][1])
    scale = np.abs(q.astype(np.float64) - p2).max() + np.abs(q.astype(np.float64) - p).max() + m * np.abs(out[0][1]).max()
    err = np.abs(moved + (p2.astype(np.float64) - p)).max()
    print(f"\n{name}: max |M (dq' - dq) + t| = {err:.3e}, bound {8 * 2.0 ** -24 * scale:.3e}")
    assert err <= 8 * 2.0 ** -24 * scale
    for pp, (gp, _) in zip((p, p2), out):
        lo, hi = (pp.astype(np.float64) - q).min(0), (pp.astype(np.float64) - q).max(0)
        assert ((gp[0] >= lo - 1e-6) & (gp[0] <= hi + 1e-6)).all(), (name, gp, lo, hi)


# ------------------------------------------------------------------------------------------ the `diameter=` keyword
def _plan(ws):
    """(diameter, n_eps) of pair 0 and the int[4] that follows the plan in a forward workspace (csrc/sinkhorn.hip, carve_sinkhorn:
    SkPlan[B] at byte 0, then at the next multiple of 256 [0] the longest schedule on the device, [2] the parity of the host's count)."""
    raw = ws[:512].cpu().numpy()
    return float(raw[:4].view(np.float32)[0]), int(raw[4:8].view(np.int32)[0]), raw[256:272].view(np.int32)


@pytest.mark.parametrize("name", sc.DIAMETER_CASES)
def test_diameter_keyword_equals_the_bounding_box_path(dev, name):
    """With the plan kernel's own diameter (the float32 bounding box) named by the caller, the host computes the schedule's length
    that the device computes on the default path: loss and gradients are bit-equal, the device's count is numpy.arange's, and the
    host's count has the device's parity (the host's is what picks the potentials the backward reads)."""
    c = sc.BY_NAME[name]
    d, n_eps = sc.bbox_diameter(c.x, c.y), sc.regime(c)["n_eps"]
    default, named = _loss(c), _loss(c, diameter=d)
    a, b = _run(default, c.x, c.y, dev), _run(named, c.x, c.y, dev)
    for what, u, v in zip(("S", "dx", "dy"), a, b):
        assert _same(u, v), (name, what, np.abs(u - v).max())
    with torch.no_grad():
        for loss in (default, named):
            s = loss(_t(c.x, dev), _t(c.y, dev)).cpu().numpy()
            assert _same(s, a[0])
            diam, dev_n, tail = _plan(loss._ws)
            print(f"\n{name}: device diameter {diam!r} (numpy {d!r}), n_eps device {dev_n}, longest {tail[0]}, host parity {tail[2]}, numpy {n_eps}")
            assert np.float32(diam) == np.float32(d) and dev_n == n_eps and tail[0] == n_eps and tail[2] == (n_eps & 1) and tail[1] == 0


# ------------------------------------------------------------------------------------------ batches
def _batched(loss, b, dev, grad_y=True):
    Xt, Yt, wt = _t(b.X, dev).requires_grad_(), _t(b.Y, dev).requires_grad_(grad_y), _t(b.w, dev)
    vals = loss.batched(Xt, Yt)
    (wt * vals).sum().backward()
    return vals.detach().cpu().numpy(), Xt.grad.cpu().numpy(), (Yt.grad.cpu().numpy() if grad_y else None)


@pytest.mark.parametrize("name", ["b6_per_pair_y", "b6_shared_y", "b70_shared_y"])
def test_batch_pairs_equal_single_calls(dev, name):
    """Every pair of a batch -- schedules of 2 entries up to the batch's longest side by side, so that finished pairs pass their
    potentials through while others go on -- is bit-equal to its single call, loss and dX (and dY[b] with one y per pair).  A
    shared y's gradient is the sum over the pairs in fixed order: within 1e-6 of the float64 sum of the single calls' gradients
    (the bar of test_batched_gradients_equal_single_calls) and the same bits on a second run."""
    b = sc.batches()[name]
    loss = _loss(blur=b.blur, scaling=b.scaling)
    vals, dX, dY = _batched(loss, b, dev)
    wt = _t(b.w, dev)
    ref = np.zeros(b.Y.shape[-2:])
    for i in range(b.X.shape[0]):
        c = b.pair(i)
        s, gx, gy = _run(loss, c.x, c.y, dev)
        assert _same(vals[i], s), (name, i, vals[i], s)
        assert _same(dX[i], (wt[i] * _t(gx, dev)).cpu().numpy()), (name, i, "dX")
        if b.shared:
            ref += np.float64(b.w[i]) * gy.astype(np.float64)
        else:
            assert _same(dY[i], (wt[i] * _t(gy, dev)).cpu().numpy()), (name, i, "dY")
    assert np.isfinite(vals).all() and (vals >= 0).all() and len(set(vals.tolist())) == len(vals)
    if b.shared:
        err = np.abs(dY - ref).max() / np.abs(ref).max()
        print(f"\n{name}: shared dy against the float64 sum of {b.X.shape[0]} single calls: {err:.3e} of max |ref|")
        assert dY.shape == b.Y.shape and err <= 1e-6
        vals2, dX2, dY2 = _batched(loss, b, dev)
        assert _same(vals, vals2) and _same(dX, dX2) and _same(dY, dY2)
        _, dX3, none = _batched(loss, b, dev, grad_y=False)
        assert none is None and _same(dX, dX3)


def test_batch_of_one_with_its_own_y(dev):
    """B = 1 with y [1, M, 3] (y_shared = 0, a stride that is never used) equals the [M, 3] call and the single call bit for bit."""
    b = sc.batches()["b1"]
    loss = _loss(blur=b.blur, scaling=b.scaling)
    vals, dX, dY = _batched(loss, b, dev)
    shared = sc.Batch("b1_shared", b.X, b.Y[0], b.w)
    vals_s, dX_s, dY_s = _batched(loss, shared, dev)
    s, gx, gy = _run(loss, b.X[0], b.Y[0], dev)
    assert vals.shape == (1,) and dY.shape == (1,) + gy.shape and dY_s.shape == gy.shape
    assert _same(vals, vals_s) and _same(vals[0], s)
    assert _same(dX, dX_s) and _same(dX[0], gx) and _same(dY[0], dY_s) and _same(dY[0], gy)
    S, rdx, rdy = sc.pair_reference(b.pair(0))
    assert abs(float(s) - S) <= sc.FWD_REL * abs(S)
    assert np.abs(gx - rdx).max() <= sc.GRAD_REL * np.abs(rdx).max() and np.abs(gy - rdy).max() <= sc.GRAD_REL * np.abs(rdy).max()


# ------------------------------------------------------------------------------------------ invariances (no reference)
@pytest.mark.parametrize("name", sc.NAMES)
def test_swapping_the_clouds(dev, name):
    """S(x, y) = S(y, x) and dS/dx of the one = dS/dy of the other: the a-side and the b-side launches on each other's data."""
    c = sc.BY_NAME[name]
    loss = _loss(c)
    s, gx, gy = _run(loss, c.x, c.y, dev)
    s2, hy, hx = _run(loss, c.y, c.x, dev)
    print(f"\n{name}: |S(x, y) - S(y, x)| = {abs(float(s) - float(s2)):.3e}, dx {np.abs(gx - hx).max():.3e}, dy {np.abs(gy - hy).max():.3e}")
    assert abs(float(s) - float(s2)) <= sc.forward_bar(c, float(s))
    assert np.abs(gx - hx).max() <= sc.grad_bar(c, gx) and np.abs(gy - hy).max() <= sc.grad_bar(c, gy)


@pytest.mark.parametrize("name", sc.PERMUTED)
def test_permuting_the_rows_of_x(dev, name):
    """Another order of x's rows: other rows share a wave, the self sums run in another order; dx follows the rows."""
    c = sc.BY_NAME[name]
    perm = np.random.Generator(np.random.PCG64(77)).permutation(c.x.shape[0])
    loss = _loss(c)
    s, gx, gy = _run(loss, c.x, c.y, dev)
    s2, hx, hy = _run(loss, c.x[perm], c.y, dev)
    print(f"\n{name}: |S - S_perm| = {abs(float(s) - float(s2)):.3e}, dx {np.abs(gx[perm] - hx).max():.3e}, dy {np.abs(gy - hy).max():.3e}")
    assert abs(float(s) - float(s2)) <= sc.forward_bar(c, float(s))
    assert np.abs(gx[perm] - hx).max() <= sc.grad_bar(c, gx) and np.abs(gy - hy).max() <= sc.grad_bar(c, gy)


@pytest.mark.parametrize("blur,scaling", sc.BLUR_SCALING)
def test_a_cloud_against_itself(dev, blur, scaling):
    """loss(x, x) is within 1e-7 of zero at every (blur, scaling) of the case list, and its gradient is zero within the gradient
    bar at the scale of this cloud's gradient against a shifted copy of itself."""
    x, shifted = sc.self_cloud()
    loss = _loss(blur=blur, scaling=scaling)
    s, gx, gy = _run(loss, x, x.copy(), dev)
    _, rx, _ = _run(loss, x, shifted, dev)
    print(f"\nblur {blur}, scaling {scaling}: S(x, x) = {float(s):.3e}, max |dx| = {np.abs(gx).max():.3e} against {np.abs(rx).max():.3e}")
    assert abs(float(s)) <= 1e-7
    assert np.abs(rx).max() > 0 and max(np.abs(gx).max(), np.abs(gy).max()) <= sc.GRAD_REL * np.abs(rx).max()


# ------------------------------------------------------------------------------------------ the Python wrapper
def test_masked_column_slice_of_a_state(dev):
    """x = state[-1][mask][:, 2:5], the planner's view of a [k, N, 8] state: the value of the contiguous call, its gradient in the
    masked rows and columns 2:5 of the last frame, zeros everywhere else."""
    rng = np.random.Generator(np.random.PCG64(601))
    k, N = 3, 500
    state = _t(rng.standard_normal((k, N, 8)).astype(np.float32) * 0.05 + 0.5, dev).requires_grad_()
    mask = _t(rng.random(N) < 0.6, dev)
    y = _t((0.52 + 0.06 * rng.standard_normal((230, 3))).astype(np.float32), dev)
    loss = _loss()
    x = state[-1][mask][:, 2:5]
    assert not x.is_contiguous() and x.shape[0] not in (0, N)
    out = loss(x, y)
    out.backward()
    xc = state.detach()[-1][mask][:, 2:5].contiguous().requires_grad_()
    outc = loss(xc, y)
    outc.backward()
    assert _same(out.detach().cpu().numpy(), outc.detach().cpu().numpy())
    g = state.grad.clone()
    rows = mask.nonzero().squeeze(1)
    assert float(xc.grad.abs().max()) > 0 and torch.equal(g[-1][rows][:, 2:5], xc.grad)
    g[-1, rows, 2:5] = 0
    assert not g.any()
    # the batched form on the stacked final frames of two candidates, as TrajectoryCMAsolver builds them
    finals = torch.stack((state.detach(), state.detach() + 0.01)).requires_grad_()
    X = finals[:, -1].index_select(1, rows)[:, :, 2:5]
    assert not X.is_contiguous()
    vals = loss.batched(X, y)
    vals.sum().backward()
    assert _same(vals[0].detach().cpu().numpy(), outc.detach().cpu().numpy())
    assert torch.equal(finals.grad[0, -1][rows][:, 2:5], xc.grad) and not finals.grad[:, :-1].any() and not finals.grad[..., :2].any()


def test_float64_input(dev):
    c = sc.BY_NAME["size_17_63"]
    loss = _loss(c)
    s, gx, gy = _run(loss, c.x, c.y, dev)
    xt, yt = _t(c.x, dev).double().requires_grad_(), _t(c.y, dev).double().requires_grad_()
    out = loss(xt, yt)
    out.backward()
    assert xt.grad.dtype == torch.float64 and yt.grad.dtype == torch.float64
    assert _same(out.detach().cpu().numpy(), s)
    assert np.array_equal(xt.grad.cpu().numpy(), gx.astype(np.float64)) and np.array_equal(yt.grad.cpu().numpy(), gy.astype(np.float64))


@pytest.mark.parametrize("order", [((600, 550), (40, 33), (700, 10)), ((40, 33), (700, 10), (600, 550))])
def test_shared_workspace_reuse(dev, order):
    """One SamplesLoss at three sizes, its shared workspace filled with NaN bytes between the calls: every result is a fresh
    object's.  The first order starts at the largest size (the workspace is reused), the second grows it twice."""
    rng = np.random.Generator(np.random.PCG64(602))
    loss = _loss()
    sizes = []
    with torch.no_grad():
        for n, m in order:
            x, y = _t((0.5 + 0.05 * rng.standard_normal((n, 3))).astype(np.float32), dev), _t((0.53 + 0.06 * rng.standard_normal((m, 3))).astype(np.float32), dev)
            if loss._ws is not None:
                loss._ws.fill_(0xFF)
            got = loss(x, y).cpu().numpy()
            want = _loss()(x, y).cpu().numpy()
            assert np.isfinite(got) and got > 0 and _same(got, want), (n, m, got, want)
            sizes.append(loss._ws.numel())
    assert sizes == sorted(sizes) and (len(set(sizes)) == 1) == (order[0] == (600, 550)), sizes


def test_wrong_shapes_raise_value_error(dev):
    loss = _loss()
    z = lambda *s: torch.zeros(s, device=dev)
    for x, y in ((z(2, 10, 3), z(3, 7, 3)), (z(2, 10, 2), z(7, 3)), (z(2, 10, 3), z(7, 4)), (z(10, 3), z(7, 3)), (z(2, 10, 3), z(2, 2, 7, 3))):
        with pytest.raises(ValueError, match="point clouds must be"):
            loss.batched(x, y)
    for x, y in ((z(10, 2), z(7, 3)), (z(10, 3), z(7, 4)), (z(1, 10, 3), z(7, 3)), (z(10, 3), z(1, 7, 3))):
        with pytest.raises(ValueError, match="point clouds must be"):
            loss(x, y)


def test_bad_arguments_raise_gm_error(dev):
    """scaling outside (0, 1) and blur <= 0 are refused by the library, with its message, before anything is launched -- with and
    without grad; so is a workspace one byte short, forward and backward, through the C ABI itself.  A good call still works after."""
    from gnn_manip_amd._lib import GMError, check, current_stream, lib, ptr
    c = sc.BY_NAME["size_17_63"]
    x, y = _t(c.x, dev), _t(c.y, dev)
    for kw in (dict(scaling=0.0), dict(scaling=1.0), dict(scaling=1.5), dict(blur=0.0), dict(blur=-0.05)):
        for grad in (False, True):
            with pytest.raises(GMError, match="need blur > 0 and 0 < scaling < 1") as e:
                _loss(**kw)(x.clone().requires_grad_(grad), y)
            assert e.value.code != 0 and lib().gm_last_error().decode() in str(e.value)
    L = lib()
    n, m = c.x.shape[0], c.y.shape[0]
    need = L.gm_sinkhorn_batched_workspace_bytes(1, n, m)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.full((1,), -1.0, device=dev)
    fwd = lambda nbytes: L.gm_sinkhorn_divergence_batched(ptr(x), 1, n, ptr(y), m, 1, 0.05, 0.5, 0.0, ptr(out), ptr(ws), nbytes, current_stream())
    with pytest.raises(GMError, match=f"workspace {need - 1} < {need}"):
        check(fwd(need - 1))
    assert float(out) == -1.0
    check(fwd(need))
    assert _same(out[0].cpu().numpy(), _loss()(x, y).cpu().numpy())
    one, dx, dy = torch.ones(1, device=dev), torch.full_like(x, -1.0), torch.full_like(y, -1.0)
    need_b = L.gm_sinkhorn_batched_backward_workspace_bytes(1, n, m, 1)
    assert need_b >= m * 12 and L.gm_sinkhorn_batched_backward_workspace_bytes(1, n, m, 0) == 0
    wsb = torch.empty(need_b, dtype=torch.uint8, device=dev)
    bwd = lambda fbytes, b, bbytes: L.gm_sinkhorn_divergence_batched_backward(ptr(x), 1, n, ptr(y), m, 1, 0.05, 0.5, ptr(one), ptr(dx), ptr(dy), ptr(ws),
                                                                              fbytes, b, bbytes, current_stream())
    for args in ((need - 1, ptr(wsb), need_b), (need, ptr(wsb), need_b - 1), (need, None, 0)):
        with pytest.raises(GMError, match="workspace"):
            check(bwd(*args))
    assert float(dx.max()) == -1.0 and float(dy.max()) == -1.0
    check(bwd(need, ptr(wsb), need_b))
    _, gx, gy = _run(_loss(), c.x, c.y, dev)
    assert _same(dx.cpu().numpy(), gx) and _same(dy.cpu().numpy(), gy)


def test_second_backward_raises(dev):
    c = sc.BY_NAME["size_5_64"]
    xt = _t(c.x, dev).requires_grad_()
    out = _loss(c)(xt, _t(c.y, dev))
    out.backward(retain_graph=True)
    first = xt.grad.clone()
    with pytest.raises(RuntimeError, match="backward runs once"):
        out.backward()
    assert torch.equal(xt.grad, first)
