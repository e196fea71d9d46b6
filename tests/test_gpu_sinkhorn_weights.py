"""Weighted point clouds in the Sinkhorn loss on the MI355X: gm_sinkhorn_divergence_weighted and its backward (csrc/sinkhorn.hip),
SamplesLoss's four-argument call and `batched(..., a=, b=)` (losses.py), and the planner's density targets (planner.py), on the
cases of sinkhorn_weight_cases.py.

Bars: the project's, from sinkhorn_cases.py -- |S - ref| <= FWD_REL |ref| and gradients per element within GRAD_REL of max |ref|
against the float64 restatement; test_sinkhorn_weight_cases.py shows on the CPU that float32 alone stays within half of them on
every case.  Where the device is compared with itself (padding with zero-weight points, a = b = NULL against the unweighted entry
points, a batch against its single calls, a second run, a poisoned workspace, the planner's calls against the hand-made chain)
the bar is equal bits.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import sinkhorn_cases as sc
import sinkhorn_weight_cases as wc
from gpu_support import dev, planner_solver, poison_allocator, step_solver, to_dev
from oracle import epd_oracle as orc

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return None if a is None else to_dev(a, dev)


def _loss(blur=0.05, scaling=0.5, diameter=None):
    from gnn_manip_amd.losses import SamplesLoss
    return SamplesLoss(loss="sinkhorn", p=2, blur=blur, scaling=scaling, diameter=diameter)


def _run(loss, x, y, a, b, dev):
    """(S, dS/dx, dS/dy) of one weighted call as numpy float32."""
    xt, yt = _t(x, dev).requires_grad_(), _t(y, dev).requires_grad_()
    out = loss(_t(a, dev), xt, _t(b, dev), yt)
    out.backward()
    return out.detach().cpu().numpy(), xt.grad.cpu().numpy(), yt.grad.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------ 1. every case against float64
@pytest.mark.parametrize("given", [False, True])
@pytest.mark.parametrize("name", wc.NAMES)
def test_case_vs_float64(dev, name, given):
    """Loss, dx and dy of every case, with the bounding-box diameter and with `diameter=` given; the value is the same bits with and
    without grad; the gradient rows of zero-weight points are exactly 0.0.  Measured on an MI355X over the 60 runs: S within 2.6e-7
    relative (1_300 uniform), gradients within 1.7e-6 of max |ref|."""
    c = wc.BY_NAME[name]
    S, rdx, rdy = wc.reference(name, given)
    loss = _loss(c.blur, c.scaling, c.diameter(given))
    s, gx, gy = _run(loss, c.x, c.y, c.a, c.b, dev)
    with torch.no_grad():
        s_plain = loss(_t(c.a, dev), _t(c.x, dev), _t(c.b, dev), _t(c.y, dev)).cpu().numpy()
    err = abs(float(s) - S)
    print(f"\n{name} given={given}: S = {float(s):.9e}, ref {S:.9e}, |err| / |ref| = {err / abs(S):.3e}")
    worst = {}
    for what, got, ref in (("dx", gx, rdx), ("dy", gy, rdy)):
        assert got.shape == ref.shape and got.dtype == np.float32 and np.isfinite(got).all(), (name, what)
        worst[what] = float(np.abs(got - ref).max()) / float(np.abs(ref).max())
        print(f"{name} given={given}: {what} max |err| / max |ref| = {worst[what]:.3e}")
    assert np.isfinite(s) and err <= sc.FWD_REL * abs(S), (name, float(s), S)
    assert _same(s_plain, s), name
    assert worst["dx"] <= sc.GRAD_REL and worst["dy"] <= sc.GRAD_REL, (name, worst)
    for w, g in ((c.a, gx), (c.b, gy)):
        if w is not None and (w == 0).any():
            assert _same(g[w == 0], np.zeros_like(g[w == 0])), name


# ------------------------------------------------------------------------------------------ 2. multiplicities
def test_multiplicities_equal_the_unweighted_call_on_repeated_points(dev):
    """Weights k_i / sum k on distinct points against the existing two-argument call on the cloud with point i repeated k_i times:
    both within FWD_REL of the oracle's float64 value on the repeated cloud, hence within 2 FWD_REL of each other; the weighted
    gradient against the repeated cloud's summed over the copies, both within GRAD_REL of the float64 sums."""
    x, y, kx, ky = wc.multiplicity_pair()
    X, ix = wc.expand(x, kx)
    Y, iy = wc.expand(y, ky)
    a, b = (kx / kx.sum()).astype(np.float32), (ky / ky.sum()).astype(np.float32)
    want = orc.sinkhorn_divergence(X, Y, blur=0.05, scaling=0.5)
    _, rX, rY = sc.sinkhorn_grad_ref(X, Y, blur=0.05, scaling=0.5)
    loss = _loss()
    s_w, gx, gy = _run(loss, x, y, a, b, dev)
    Xt, Yt = _t(X, dev).requires_grad_(), _t(Y, dev).requires_grad_()
    s_u = loss(Xt, Yt)
    s_u.backward()
    s_u = float(s_u.detach().cpu())
    print(f"\nmultiplicities: weighted {float(s_w):.9e}, repeated {s_u:.9e}, float64 {want:.9e}")
    assert abs(float(s_w) - want) <= sc.FWD_REL * abs(want) and abs(s_u - want) <= sc.FWD_REL * abs(want)
    assert abs(float(s_w) - s_u) <= 2 * sc.FWD_REL * abs(want)
    for what, g, G, idx, ref in (("dx", gx, Xt.grad, ix, rX), ("dy", gy, Yt.grad, iy, rY)):
        summed, rsum = np.zeros(g.shape), np.zeros(g.shape)
        np.add.at(summed, idx, G.cpu().numpy().astype(np.float64))
        np.add.at(rsum, idx, ref)
        top = np.abs(rsum).max()
        print(f"multiplicities {what}: weighted - float64 {np.abs(g - rsum).max() / top:.3e}, repeated - float64 {np.abs(summed - rsum).max() / top:.3e}, "
              f"weighted - repeated {np.abs(g - summed).max() / top:.3e} of max |ref|")
        assert np.abs(g - rsum).max() <= sc.GRAD_REL * top and np.abs(summed - rsum).max() <= sc.GRAD_REL * top
        assert np.abs(g - summed).max() <= 2 * sc.GRAD_REL * top


# ------------------------------------------------------------------------------------------ 3. padding
@pytest.mark.parametrize("pad_x,pad_y", [(20, 0), (0, 20), (1, 31)])
def test_zero_weight_padding_changes_no_bit(dev, pad_x, pad_y):
    """`diameter=` given, zero-weight points appended to either cloud (64 -> 65 rows opens a fifth 16-row workgroup, 65 -> 96 points
    a second sweep of the 64 lanes; the points lie far outside the clouds): the loss and the real rows' gradients keep their bits,
    the appended rows' gradients are 0.0."""
    c = wc.BY_NAME["64_65_blur0.05_sc0.5_lognormal"]
    rng = np.random.Generator(np.random.PCG64(771))
    far = lambda k: (3.0 + rng.standard_normal((k, 3))).astype(np.float32)
    x2, y2 = np.concatenate((c.x, far(pad_x))), np.concatenate((c.y, far(pad_y)))
    a2, b2 = np.concatenate((c.a, np.zeros(pad_x, np.float32))), np.concatenate((c.b, np.zeros(pad_y, np.float32)))
    loss = _loss(c.blur, c.scaling, wc.DIAMETER_GIVEN)
    s, gx, gy = _run(loss, c.x, c.y, c.a, c.b, dev)
    s2, gx2, gy2 = _run(loss, x2, y2, a2, b2, dev)
    n, m = c.x.shape[0], c.y.shape[0]
    print(f"\npadding +{pad_x} / +{pad_y}: S {float(s)!r} -> {float(s2)!r}, max |d dx| {np.abs(gx2[:n] - gx).max():.3e}, max |d dy| {np.abs(gy2[:m] - gy).max():.3e}")
    assert np.isfinite(s) and _same(s, s2) and _same(gx2[:n], gx) and _same(gy2[:m], gy)
    assert _same(gx2[n:], np.zeros((pad_x, 3), np.float32)) and _same(gy2[m:], np.zeros((pad_y, 3), np.float32))


# ------------------------------------------------------------------------------------------ 4. reduction to the unweighted path
def _abi_call(dev, a, X, b, Y, diameter=0.0, weighted=True):
    """The entry points through ctypes on a batch X [B, n, 3] against Y ([m, 3] or [B, m, 3]): (losses, dX, dY) with grad_loss = 1."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    bsz, n, m, shared = X.shape[0], X.shape[1], Y.shape[-2], 1 if Y.dim() == 2 else 0
    out, dX, dY, ones = torch.full((bsz,), -1.0, device=dev), torch.full_like(X, -1.0), torch.full_like(Y, -1.0), torch.ones(bsz, device=dev)
    wsb = torch.empty(max(L.gm_sinkhorn_batched_backward_workspace_bytes(bsz, n, m, shared), 1), dtype=torch.uint8, device=dev)
    if weighted:
        ws = torch.empty(L.gm_sinkhorn_weighted_workspace_bytes(bsz, n, m, a is not None, b is not None, shared), dtype=torch.uint8, device=dev)
        check(L.gm_sinkhorn_divergence_weighted(ptr(a), ptr(X), bsz, n, ptr(b), ptr(Y), m, shared, 0.05, 0.5, diameter, ptr(out), ptr(ws), ws.numel(),
                                                current_stream()))
        check(L.gm_sinkhorn_divergence_weighted_backward(ptr(a), ptr(X), bsz, n, ptr(b), ptr(Y), m, shared, 0.05, 0.5, ptr(ones), ptr(dX), ptr(dY),
                                                         ptr(ws), ws.numel(), ptr(wsb), wsb.numel(), current_stream()))
    else:
        ws = torch.empty(L.gm_sinkhorn_batched_workspace_bytes(bsz, n, m), dtype=torch.uint8, device=dev)
        check(L.gm_sinkhorn_divergence_batched(ptr(X), bsz, n, ptr(Y), m, shared, 0.05, 0.5, diameter, ptr(out), ptr(ws), ws.numel(), current_stream()))
        check(L.gm_sinkhorn_divergence_batched_backward(ptr(X), bsz, n, ptr(Y), m, shared, 0.05, 0.5, ptr(ones), ptr(dX), ptr(dY), ptr(ws), ws.numel(),
                                                        ptr(wsb), wsb.numel(), current_stream()))
    return out.cpu().numpy(), dX.cpu().numpy(), dY.cpu().numpy()


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("diameter", [0.0, wc.DIAMETER_GIVEN])
def test_no_weights_is_the_unweighted_entry_point(dev, shared, diameter):
    """a = b = NULL through gm_sinkhorn_divergence_weighted and its backward: the bits of gm_sinkhorn_divergence_batched and its
    backward (loss, dx, dy), on a batch whose pairs have schedules of their own."""
    X, Y, _, _, _ = wc.batch(shared)
    Xt, Yt = _t(X, dev), _t(Y, dev)
    got = _abi_call(dev, None, Xt, None, Yt, diameter, weighted=True)
    want = _abi_call(dev, None, Xt, None, Yt, diameter, weighted=False)
    assert np.isfinite(want[0]).all() and (want[0] > 0).all() and np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0
    for what, u, v in zip(("S", "dx", "dy"), got, want):
        assert _same(u, v), (what, np.abs(u - v).max())


@pytest.mark.parametrize("side", ["a", "b"])
def test_a_null_side_agrees_with_explicit_uniform_weights(dev, side):
    """One side NULL (the scalar -log n in the uniform instantiation, the mean in the cost) against the same side as explicit 1/n
    (log of the float32 1/n per point): within the bars of each other, the other side carrying Dirichlet weights."""
    c = wc.BY_NAME["150_130_blur0.05_sc0.5_dirichlet"]
    n, m = c.x.shape[0], c.y.shape[0]
    other = wc.weights("dirichlet", n if side == "b" else m, np.random.Generator(np.random.PCG64(772)))
    null = dict(a=None, b=other) if side == "a" else dict(a=other, b=None)
    full = dict(null, **{side: np.full(n if side == "a" else m, 1.0 / (n if side == "a" else m), np.float32)})
    loss = _loss()
    s0, gx0, gy0 = _run(loss, c.x, c.y, null["a"], null["b"], dev)
    s1, gx1, gy1 = _run(loss, c.x, c.y, full["a"], full["b"], dev)
    print(f"\nNULL {side}: S {float(s0):.9e} against explicit {float(s1):.9e}; dx {np.abs(gx0 - gx1).max() / np.abs(gx1).max():.3e}, "
          f"dy {np.abs(gy0 - gy1).max() / np.abs(gy1).max():.3e} of the largest element")
    assert float(s1) > 0 and abs(float(s0) - float(s1)) <= sc.FWD_REL * abs(float(s1))
    assert np.abs(gx0 - gx1).max() <= sc.GRAD_REL * np.abs(gx1).max() and np.abs(gy0 - gy1).max() <= sc.GRAD_REL * np.abs(gy1).max()


# ------------------------------------------------------------------------------------------ 5. batches
def _batched(loss, X, Y, A, Bw, w, dev):
    Xt, Yt = _t(X, dev).requires_grad_(), _t(Y, dev).requires_grad_()
    vals = loss.batched(Xt, Yt, a=_t(A, dev), b=_t(Bw, dev))
    (_t(w, dev) * vals).sum().backward()
    return vals.detach().cpu().numpy(), Xt.grad.cpu().numpy(), Yt.grad.cpu().numpy()


@pytest.mark.parametrize("shared", [True, False])
def test_batch_pairs_equal_single_weighted_calls(dev, shared):
    """Pair b of a weighted batch -- schedules of 2 to 8 entries side by side, zero weights among the others -- is its single
    weighted call to the bit (loss, dX[b], and dY[b] with a y and b per pair).  A shared y's gradient is the pair-order sum: within
    1e-6 of the float64 sum of the single calls' gradients (the bar of test_gpu_sinkhorn_cases).  A second run and a run whose
    workspaces come out of a poisoned allocator give the same bits."""
    X, Y, A, Bw, w = wc.batch(shared)
    loss = _loss()
    vals, dX, dY = _batched(loss, X, Y, A, Bw, w, dev)
    wt = _t(w, dev)
    ref = np.zeros(Y.shape[-2:])
    lengths = set()
    for i in range(X.shape[0]):
        y_i, b_i = (Y, Bw) if shared else (Y[i], Bw[i])
        lengths.add(sc.schedule_length(sc.bbox_diameter(X[i], y_i), 0.05, 0.5))
        s, gx, gy = _run(loss, X[i], y_i, A[i], b_i, dev)
        assert _same(vals[i], s), (i, vals[i], s)
        assert _same(dX[i], (wt[i] * _t(gx, dev)).cpu().numpy()), (i, "dX")
        assert (A[i] == 0).any() and not dX[i][A[i] == 0].any() and np.abs(dX[i][A[i] > 0]).max() > 0
        if shared:
            ref += np.float64(w[i]) * gy.astype(np.float64)
        else:
            assert _same(dY[i], (wt[i] * _t(gy, dev)).cpu().numpy()), (i, "dY")
    assert len(lengths) >= 3, lengths
    assert np.isfinite(vals).all() and (vals > 0).all()
    if shared:
        err = np.abs(dY - ref).max() / np.abs(ref).max()
        print(f"\nshared dy against the float64 sum of {X.shape[0]} single calls: {err:.3e} of max |ref|")
        assert dY.shape == Y.shape and err <= 1e-6 and not dY[Bw == 0].any()
    again = _batched(loss, X, Y, A, Bw, w, dev)
    poison_allocator(dev, float("nan"))
    poisoned = _batched(_loss(), X, Y, A, Bw, w, dev)
    for other in (again, poisoned):
        assert _same(vals, other[0]) and _same(dX, other[1]) and _same(dY, other[2])


# ------------------------------------------------------------------------------------------ 6. refusals
BAD = dict(negative=-0.01, nan=float("nan"), inf=float("inf"))


@pytest.mark.parametrize("side", ["a", "b"])
@pytest.mark.parametrize("what", [*BAD, "all_zero"])
def test_bad_weights_are_refused(dev, what, side):
    """A weight that is negative, NaN or Inf, or a cloud whose weights are all zero: GMError naming the weights on the default path
    (where the host reads the plan back anyway); with `diameter=` given nothing is read back and the loss and gradients are NaN.  A
    good call works afterwards."""
    from gnn_manip_amd._lib import GMError
    c = wc.BY_NAME["17_63_blur0.05_sc0.5_multiplicity"]
    w = {"a": c.a.copy(), "b": c.b.copy()}
    if what == "all_zero":
        w[side][:] = 0.0
    else:
        w[side][len(w[side]) - 2] = BAD[what]
    x, y, a, b = _t(c.x, dev), _t(c.y, dev), _t(w["a"], dev), _t(w["b"], dev)
    for grad in (False, True):
        with pytest.raises(GMError, match="weights must be finite") as e:
            _loss()(a, x.clone().requires_grad_(grad), b, y)
        assert e.value.code != 0
    s, gx, gy = _run(_loss(diameter=wc.DIAMETER_GIVEN), c.x, c.y, w["a"], w["b"], dev)
    assert np.isnan(s) and np.isnan(gx).all() and np.isnan(gy).all()
    good = _loss()(_t(c.a, dev), x, _t(c.b, dev), y)
    assert abs(float(good) - wc.reference(c.name, False)[0]) <= sc.FWD_REL * wc.reference(c.name, False)[0]


def test_bad_pair_of_a_batch_with_diameter_given_leaves_the_others(dev):
    """`diameter=` given: the pair with a refused weight is NaN, every other pair of the batch keeps its bits."""
    X, Y, A, Bw, w = wc.batch(False)
    loss = _loss(diameter=wc.DIAMETER_GIVEN)
    vals, dX, dY = _batched(loss, X, Y, A, Bw, w, dev)
    A2 = A.copy()
    A2[2, 5] = -1.0
    vals2, dX2, dY2 = _batched(loss, X, Y, A2, Bw, w, dev)
    keep = [0, 1, 3]
    assert np.isfinite(vals).all() and np.isnan(vals2[2]) and np.isnan(dX2[2]).all() and np.isnan(dY2[2]).all()
    assert _same(vals[keep], vals2[keep]) and _same(dX[keep], dX2[keep]) and _same(dY[keep], dY2[keep])


def test_wrong_weight_arguments_raise(dev):
    """Weights are float32 constants of the clouds' shape on the clouds' device; the call takes two or four positional arguments;
    loss(x, y) and the constructor's refusals are what they were."""
    c = wc.BY_NAME["17_63_blur0.05_sc0.5_multiplicity"]
    x, y, a, b = _t(c.x, dev), _t(c.y, dev), _t(c.a, dev), _t(c.b, dev)
    loss = _loss()
    for bad_a, bad_b in ((a.clone().requires_grad_(), b), (a, b.clone().requires_grad_())):
        with pytest.raises(ValueError, match="constants"):
            loss(bad_a, x, bad_b, y)
    for bad_a, bad_b in ((a[:-1], b), (a, b[:-1]), (a.unsqueeze(0), b), (a, b.unsqueeze(1)), (a.double(), b), (a, b.half()), (a.cpu(), b), (a, b.cpu()),
                         (c.a, b), (a, c.b.tolist())):
        with pytest.raises(ValueError, match="weights . must be a float32 tensor"):
            loss(bad_a, x, bad_b, y)
    X, Y, A, Bw, _ = wc.batch(False)
    Xt, Yt, At, Bt = _t(X, dev), _t(Y, dev), _t(A, dev), _t(Bw, dev)
    for bad_a, bad_b, yy in ((At[0], Bt, Yt), (At, Bt[0], Yt), (At, Bt, Yt[0]), (At[:2], Bt, Yt)):
        with pytest.raises(ValueError, match="weights . must be a float32 tensor"):
            loss.batched(Xt, yy, a=bad_a, b=bad_b)
    assert loss.batched(Xt, Yt[0], a=At, b=Bt[0]).shape == (4,)
    for args in ((a, x, b), (x,), (a, x, b, y, y)):
        with pytest.raises(TypeError, match="positional arguments"):
            loss(*args)
    from gnn_manip_amd.losses import SamplesLoss
    for kw in (dict(loss="energy"), dict(p=1), dict(debias=False), dict(reach=1.0)):
        with pytest.raises(NotImplementedError, match="only loss='sinkhorn'"):
            SamplesLoss(**kw)
    plain = loss(x, y)
    want = orc.sinkhorn_divergence(c.x, c.y, blur=0.05, scaling=0.5)
    assert abs(float(plain) - want) <= sc.FWD_REL * want
    assert _same(loss(None, x, None, y).cpu().numpy(), plain.cpu().numpy())


# ------------------------------------------------------------------------------------------ 7. the planner
def _x0(s):
    return np.concatenate((s.sample_traj[:, 0], s.sample_traj[:, 1]))


def test_planner_objective_with_a_density_target(dev):
    """After set_density_target, cma_objective(x) is the hand-made chain rollout_candidates -> weighted loss -> _assemble_loss to
    the bit, and population_losses is the list of cma_objective values."""
    from gnn_manip_amd.planner import density_target
    s, _, _ = planner_solver(dev)
    cloud = s.desired_pos.clone()
    s.set_density_target(cloud, 0.01)
    centres, weights = density_target(cloud, 0.01)
    assert torch.equal(s.desired_pos, centres) and torch.equal(s.desired_weights, weights)
    assert 1 < len(weights) < len(cloud) and abs(float(weights.double().sum()) - 1) <= 1e-6
    x = 1.1 * _x0(s)
    got = s.cma_objective(x)
    traj, actions = s.get_rigid_body_trajectory_from_diff(x)
    with torch.no_grad():
        finals = s._engine(1).rollout_candidates(s.initial_state[0].contiguous(), torch.stack([traj]), horizon=s.horizon)
        w = _loss()(None, s._end_positions(finals)[0], weights, centres)
    want = s._assemble_loss(float(w.double().cpu()), actions)[0]
    s.desired_weights = None
    unweighted = s.cma_objective(x)
    s.desired_weights = weights
    print(f"\nplanner: {len(cloud)} particles -> {len(weights)} cells; objective {got!r}, chain {want!r}, same centres unweighted {unweighted!r}")
    assert got == want and np.isfinite(got) and got != unweighted
    rng = np.random.default_rng(6)
    X = [_x0(s) + 0.05 * rng.standard_normal(len(x)) for _ in range(6)]
    one = [s.cma_objective(v) for v in X]
    assert s.population_losses(X) == one


def test_planner_gradient_with_weights(dev):
    """loss_and_grad with desired_weights = 1/M given explicitly against the unweighted one (value within 1e-5 relative, gradient
    within GRAD_REL of its largest element), and with a density target population_loss_and_grad's rows against
    loss_and_grad(sweep="library") to the bit."""
    s = step_solver(dev)[0]
    x = 1.1 * _x0(s)
    loss0, grad0 = s.loss_and_grad(x, sweep="library")
    m = s.desired_pos.shape[0]
    s.desired_weights = torch.full((m,), 1.0 / m, dtype=torch.float32, device=dev)
    loss1, grad1 = s.loss_and_grad(x, sweep="library")
    print(f"\nplanner gradient: unweighted {loss0!r}, explicit 1/M {loss1!r}; max |d grad| / max |grad| = {np.abs(grad1 - grad0).max() / np.abs(grad0).max():.3e}")
    assert abs(loss1 - loss0) <= 1e-5 * abs(loss0)
    assert np.abs(grad1 - grad0).max() <= sc.GRAD_REL * np.abs(grad0).max() and np.count_nonzero(grad1) == len(x)
    s.set_density_target(s.desired_pos, 0.01)
    assert 1 < s.desired_weights.shape[0] < m
    X = [1.1 * _x0(s), 0.9 * _x0(s), 1.05 * _x0(s)]
    single = [s.loss_and_grad(v, sweep="library") for v in X]
    s.candidates_per_gpu = 2
    losses, grads = s.population_loss_and_grad(X, sweep="library")
    for p, (loss, grad) in enumerate(single):
        print(f"planner gradient, density target, candidate {p}: single {loss!r}, in its block {losses[p]!r}")
        assert losses[p] == loss and np.array_equal(grads[p], grad), p
    assert single[0][0] != loss1 and np.count_nonzero(grads) == grads.size


def test_interpolated_solver_takes_the_weights_forward_only(dev):
    from gnn_manip_amd.planner import InterpolatedCMAsolver
    s = step_solver(dev, InterpolatedCMAsolver)[0]
    s.set_density_target(s.desired_pos, 0.01)
    x = np.zeros(4)
    weighted = s.cma_objective(x)
    s.desired_weights = None
    assert np.isfinite(weighted) and weighted != s.cma_objective(x)
    with pytest.raises(NotImplementedError, match="no gradient"):
        s.loss_and_grad(x)
