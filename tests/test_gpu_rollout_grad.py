"""Trajectory gradients on the MI355X: gm_rigid_transform_backward and planner.rigid_body_trajectory, the inputs-only model
backward (gm_epd_backward_inputs_only), RolloutEngine.differentiable_rollout (values, gradients, constant memory) and
TrajectoryCMAsolver.loss_and_grad.

Yardstick of the gradients through the model: the rule of tests/yardstick.py (`within`), the flip allowance per element, against
the float64 restatement of tests/rollout_grad_cases.py (checked on the CPU) on the edge lists the
device returned.  The rigid transform's transpose is a plain sum: its bar is the element-wise float32 summation bound
Nr 2^-23 sum |terms|.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
import grad_cases as gc
import rollout_grad_cases as rc
from gpu_support import dev, load_model as _model, step_engine as _engine, step_solver as _solver, to_dev as _t
from grad_cases import L0, flip_allowance, split as _split, step_allowance as _step_allowance, step_reference as _step_reference
from rollout_grad_cases import objective_reference as _objective_reference
from sinkhorn_cases import sinkhorn_grad_ref
from train_cases import HUB_E, HUB_N, graph as _graph, hub_graph as _hub_graph
from yardstick import lazy as _lazy, within as _within

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ 1. the rigid transform's transpose
def _rigid_case(nr, steps, seed):
    rng = np.random.default_rng(seed)
    init = (0.4 + 0.2 * rng.random((nr, 3))).astype(np.float32)
    rot = rng.uniform(2.5, 3.5, steps)
    ty = 1e-3 * rng.standard_normal(steps)
    g = rng.standard_normal((steps, nr, 3)).astype(np.float32)
    return init, rot, ty, g


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("nr", [0, 1, 63, 64, 65, 257, 1000])
def test_rigid_transform_backward(dev, nr, steps):
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    init, rot, ty, g = _rigid_case(nr, steps, 100 * nr + steps)
    cst = np.stack((np.cos(rot), np.sin(rot), 0.5 + ty), axis=1).astype(np.float32)
    t3 = (C.c_float * 3)(*rc.TY_INIT)
    d_init, d_cst, d_g = _t(init, dev), _t(cst, dev), _t(g, dev)
    outs = []
    for _ in range(2):
        out = torch.full((steps, 3), float("nan"), device=dev)
        check(lib().gm_rigid_transform_backward(ptr(d_init), nr, ptr(d_cst), steps, C.byref(t3), ptr(d_g), ptr(out), current_stream(dev)))
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    ref, terms = rc.rigid_transform_transpose(init, rc.TY_INIT, g)
    got = outs[0].cpu().numpy().astype(np.float64)
    bound = nr * 2.0 ** -23 * terms
    print(f"\n[rollout grads] rigid transpose Nr={nr} T={steps}: max err / bound "
          f"{(np.abs(got - ref) / np.maximum(bound, 1e-300)).max() if nr else 0.0:.3e}, max |ref| {np.abs(ref).max():.3e}")
    assert (np.abs(got - ref) <= bound).all(), (got, ref, bound)
    if nr == 0:
        assert not got.any()


@pytest.mark.parametrize("nr", [1, 65, 257])
def test_rigid_body_trajectory_is_the_numpy_functions_and_differentiates(dev, nr):
    from gnn_manip_amd.planner import get_rigid_body_trajectory, rigid_body_trajectory
    init, rot, ty, g = _rigid_case(nr, 3, 7 + nr)
    rp = _t(init, dev)
    want = get_rigid_body_trajectory(rot, ty, 3, list(rc.TY_INIT), rp)
    r, t = gc.t64(rot, True), gc.t64(ty, True)
    got = rigid_body_trajectory(r, t, 3, list(rc.TY_INIT), rp)
    assert torch.equal(got.detach(), want)
    (got * _t(g, dev)).sum().backward()
    r64, t64 = gc.t64(rot, True), gc.t64(ty, True)
    (rc.poses(r64, t64, rc.TY_INIT, gc.t64(init)) * gc.t64(g)).sum().backward()
    # chain rule over the float32 kernel's sums: the summation bound of each (cos, sin, ty) entry, carried through |d cos|, |d sin| <= 1,
    # plus the float32 rounding of cos / sin themselves on sums of that size
    _, terms = rc.rigid_transform_transpose(init, rc.TY_INIT, g)
    bound_r = (nr + 2) * 2.0 ** -23 * (terms[:, 0] + terms[:, 1])
    bound_t = nr * 2.0 ** -23 * terms[:, 2]
    for what, a, b, bound in (("rot", r.grad, r64.grad, bound_r), ("ty", t.grad, t64.grad, bound_t)):
        err = np.abs(a.numpy() - b.numpy())
        print(f"\n[rollout grads] rigid_body_trajectory Nr={nr} d_{what}: max err / bound {(err / bound).max():.3e}")
        assert (err <= bound).all(), (what, err, bound)
    with pytest.raises(IndexError):
        rigid_body_trajectory(r, t, 4, list(rc.TY_INIT), rp)


# ------------------------------------------------------------------------------------------ 2. the inputs-only backward
def _both_backwards(m, nodes, ea, ei, w, dev):
    """gm_epd_forward_train once, then gm_epd_backward_inputs and gm_epd_backward_inputs_only on that tape (the second on a copy
    taken before the first ran, in a workspace filled with NaN bytes): ((d_nodes, d_edge_attr) of each, parameter gradient views)."""
    from gnn_manip_amd._lib import ModelDesc, check, current_stream, lib, ptr
    from gnn_manip_amd.epd_gnn import _grad_arrays
    from gnn_manip_amd.graph import _ws
    L = lib()
    with torch.no_grad():
        desc_t, handle, tensors, key = m._training_spec([p.detach() for p in m.parameters()])
    h = handle.get(desc_t, tensors, dev, key)
    d = C.byref(ModelDesc(*desc_t))
    x, a, idx, go = _t(nodes, dev), _t(ea, dev), _t(ei, dev), _t(w, dev)
    n, e = x.shape[0], a.shape[0]
    tape = _ws(L.gm_train_tape_bytes(d, n, e), dev)
    out = torch.empty((n, m.dims[2]), device=dev)
    check(L.gm_epd_forward_train(h, ptr(x), n, ptr(a), ptr(idx), e, ptr(out), ptr(tape), tape.numel(), current_stream(dev)))
    tape2 = tape.clone()
    tensors, views, t_arr, g_arr = _grad_arrays(tensors, dev)
    need = L.gm_train_backward_inputs_workspace_bytes(d, n, e)
    ws = _ws(need, dev)
    full = (torch.full_like(x, float("nan")), torch.full_like(a, float("nan")))
    check(L.gm_epd_backward_inputs(h, t_arr, len(tensors), ptr(x), ptr(a), n, e, ptr(go), g_arr, ptr(full[0]), ptr(full[1]), ptr(tape),
                                   tape.numel(), ptr(ws), ws.numel(), current_stream(dev)))
    res = [full]
    for which in ((True, True), (True, False), (False, True)):
        if e == 0 and not which[0]:               # no edges: an empty d_edge_attr has no address, there is nothing to ask for
            res.append((None, torch.empty_like(a)))
            continue
        ws2 = _ws(need, dev).fill_(0xff)          # the query's size is enough, and nothing is read that the call did not write
        dx = torch.full_like(x, float("nan")) if which[0] else None
        da = torch.full_like(a, float("nan")) if which[1] else None
        check(L.gm_epd_backward_inputs_only(h, t_arr, len(tensors), ptr(x), ptr(a), n, e, ptr(go), ptr(dx), ptr(da), ptr(tape2.clone()),
                                            tape2.numel(), ptr(ws2), ws2.numel(), current_stream(dev)))
        res.append((dx, da))
    rc_none = L.gm_epd_backward_inputs_only(h, t_arr, len(tensors), ptr(x), ptr(a), n, e, ptr(go), None, None, ptr(tape2), tape2.numel(),
                                            ptr(ws), ws.numel(), current_stream(dev))
    assert rc_none == -1 and b"both null" in L.gm_last_error()
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("hidden", [64, 128, 256, 100])
def test_inputs_only_is_bit_equal_on_the_same_tape(dev, hidden):
    dims = (25, 4, 3, hidden, 2, 2)
    nodes, ea, ei = _graph(300, 0.06, 400 + hidden)
    m = _model(orc.init_params(*dims, 400 + hidden), dims, dev)
    full, both, only_x, only_a = _both_backwards(m, nodes, ea, ei, gc.weights((300, 3), hidden), dev)
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[1]).all() and float(full[0].abs().max()) > 0
    assert torch.equal(both[0], full[0]) and torch.equal(both[1], full[1])
    assert torch.equal(only_x[0], full[0]) and torch.equal(only_a[1], full[1])


def test_inputs_only_on_the_hub_multigraph_in_random_edge_order(dev):
    ei = _hub_graph()
    rng = np.random.Generator(np.random.PCG64(411))
    nodes = rng.standard_normal((HUB_N, 25)).astype(np.float32)
    ea = rng.standard_normal((HUB_E, 4)).astype(np.float32)
    dims = (25, 4, 3, 128, 2, 2)
    m = _model(orc.init_params(*dims, 411), dims, dev)
    full, both, _, _ = _both_backwards(m, nodes, ea, ei, gc.weights((HUB_N, 3), 412), dev)
    assert torch.equal(both[0], full[0]) and torch.equal(both[1], full[1])


def test_inputs_only_on_a_graph_without_edges(dev):
    dims = (25, 4, 3, 128, 2, 2)
    nodes = np.random.default_rng(5).standard_normal((130, 25)).astype(np.float32)
    m = _model(orc.init_params(*dims, 99), dims, dev)
    full, both, only_x, _ = _both_backwards(m, nodes, np.zeros((0, 4), np.float32), np.zeros((2, 0), np.int64), gc.weights((130, 3), 6), dev)
    assert torch.equal(both[0], full[0]) and torch.equal(only_x[0], full[0]) and both[1].shape == (0, 4)


def _module_run(m, nodes, ea, ei, w, dev):
    x, a = _t(nodes, dev).requires_grad_(True), _t(ea, dev).requires_grad_(True)
    out = m.forward(x, a, _t(ei, dev))
    (out * _t(w, dev)).sum().backward()
    return out.detach(), x.grad, a.grad


@pytest.mark.parametrize("hidden", [128, 100])
def test_module_takes_the_inputs_only_path_when_it_can(dev, hidden):
    """All parameters frozen: the inputs' gradients of the full path bit for bit, every .grad None.  One parameter unfrozen: the
    full path, parameter gradient bit-equal to the all-trainable model's.  forward_inputs_only on a model nobody froze: the
    same input gradients, no .grad touched."""
    dims = (25, 4, 3, hidden, 2, 2)
    params = orc.init_params(*dims, 420 + hidden)
    nodes, ea, ei = _graph(300, 0.06, 420)
    w = gc.weights((300, 3), 421)
    trainable = _model(params, dims, dev)
    out0, dx0, da0 = _module_run(trainable, nodes, ea, ei, w, dev)
    frozen = _model(params, dims, dev).requires_grad_(False)
    out1, dx1, da1 = _module_run(frozen, nodes, ea, ei, w, dev)
    assert torch.equal(out1, out0) and torch.equal(dx1, dx0) and torch.equal(da1, da0)
    assert all(p.grad is None for p in frozen.parameters())
    one = _model(params, dims, dev).requires_grad_(False)
    name = "processor.1.phi_edge.0.weight"
    dict(one.named_parameters())[name].requires_grad_(True)
    _, dx2, da2 = _module_run(one, nodes, ea, ei, w, dev)
    assert torch.equal(dx2, dx0) and torch.equal(da2, da0)
    for k, p in one.named_parameters():
        if k == name:
            assert torch.equal(p.grad, dict(trainable.named_parameters())[k].grad)
        else:
            assert p.grad is None, k
    free = _model(params, dims, dev)
    x, a = _t(nodes, dev).requires_grad_(True), _t(ea, dev).requires_grad_(True)
    out = free.forward_inputs_only(x, a, _t(ei, dev))
    (out * _t(w, dev)).sum().backward()
    assert torch.equal(out.detach(), out0) and torch.equal(x.grad, dx0) and torch.equal(a.grad, da0)
    assert all(p.requires_grad and p.grad is None for p in free.parameters())


def test_flagged_edge_index_gives_zero_rows_on_the_inputs_only_path(dev):
    from gnn_manip_amd import EncProcDecGNN
    from gnn_manip_amd._lib import GMError
    torch.manual_seed(3)
    n, e = 300, 4000
    m = EncProcDecGNN(25, 4, 3, 128, 2, 2).to(dev).requires_grad_(False)
    x, ea = torch.randn(n, 25, device=dev).requires_grad_(), torch.randn(e, 4, device=dev).requires_grad_()
    bad = torch.randint(0, n, (2, e), device=dev)
    bad[1, 17] = n + 5
    out = m.forward(x, ea, bad)
    out.abs().sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert x.grad.shape == x.shape and float(x.grad.abs().max()) == 0.0
    assert ea.grad.shape == ea.shape and float(ea.grad.abs().max()) == 0.0
    with pytest.raises(GMError, match="out of range"):
        m.status()


# ------------------------------------------------------------------------------------------ 3. the rollout
def _weighted(dev):
    w = gc.weights(gc.step_state("step_a").shape, 6)
    return (lambda final: (final * _t(w, dev)).sum()), (lambda nxt: w)


def _sinkhorn(obs_np, dev):
    from gnn_manip_amd.losses import SamplesLoss
    fluid, cloud = rc.desired_cloud(obs_np)
    fl, c = _t(fluid, dev), slice(L0.cart, L0.cart + 3)
    loss = SamplesLoss(loss="sinkhorn", p=2, blur=.05)

    def end_loss(nxt):
        g = np.zeros_like(nxt)
        s, dx, _ = sinkhorn_grad_ref(nxt[-1][fluid][:, c], cloud)
        g[-1][fluid, c] = dx
        end_loss.value = s
        return g
    return (lambda final: loss(final[-1][fl][:, c], _t(cloud, dev))), end_loss


def _rollout(eng, obs_np, traj_np, dev, device_loss, steps=rc.T):
    obs = _t(obs_np, dev).requires_grad_(True)
    tr = None if traj_np is None else _t(traj_np, dev).requires_grad_(True)
    final, eis = eng.differentiable_rollout(obs, tr, horizon=steps, return_edges=True)
    assert final.grad_fn is not None and eis == []
    loss = device_loss(final)
    loss.backward()
    assert len(eis) == steps
    return final.detach(), float(loss.detach()), obs.grad, None if tr is None else tr.grad, [e.cpu().numpy() for e in eis]


@pytest.mark.parametrize("end", ["weighted sum", "samples loss"])
@pytest.mark.parametrize("with_trajectory", [True, False])
def test_differentiable_rollout(dev, with_trajectory, end):
    params = rc.params()
    m = _model(params, gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    traj_np = rc.trajectory("step_a") if with_trajectory else None
    device_loss, end_loss = _weighted(dev) if end == "weighted sum" else _sinkhorn(obs_np, dev)
    final, loss, d_obs, d_traj, eis = _rollout(eng, obs_np, traj_np, dev, device_loss)
    with torch.no_grad():
        plain = eng.rollout(_t(obs_np, dev), None if traj_np is None else _t(traj_np, dev), horizon=rc.T)
    assert torch.equal(final, plain)
    assert all(p.grad is None for p in m.parameters())          # requires_grad=True, and constants of the rollout all the same
    targets = [None] * rc.T if traj_np is None else list(traj_np)
    end64, _, g_obs, g_t = _step_reference(params, obs_np, targets, eis, None, None, torch.float64, end_loss)
    if end == "samples loss":
        print(f"\n[rollout grads] loss {loss:.6e} reference {end_loss.value:.6e}")
        assert abs(loss - end_loss.value) <= 1e-5 * abs(end_loss.value)     # the forward bar of tests/test_gpu_planner.py for this loss
    end_grad = end_loss(end64)
    _, _, g_obs32, g_t32 = _step_reference(params, obs_np, targets, eis, None, None, torch.float32, end_loss)
    allow = _step_allowance(params, obs_np, targets, eis, None, None, end_grad=end_grad)
    what = f"rollout {end}" + (" with trajectory" if with_trajectory else "")
    _split(what, d_obs.cpu().numpy(), g_obs, g_obs32, allow)
    if with_trajectory:
        for t in range(rc.T):
            _within(f"{what} d_trajectory[{t}]", d_traj[t].cpu().numpy(), g_t[t], g_t32[t], lambda t=t: (allow()[0][1 + t], allow()[1]))
    if end == "weighted sum":                                    # the same call again: the same bits
        final2, _, d_obs2, d_traj2, eis2 = _rollout(eng, obs_np, traj_np, dev, device_loss)
        assert torch.equal(final2, final) and torch.equal(d_obs2, d_obs) and all(np.array_equal(a, b) for a, b in zip(eis, eis2))
        assert d_traj is None or torch.equal(d_traj2, d_traj)
        m.requires_grad_(False)                                  # frozen or not: the parameters are constants either way
        final3, _, d_obs3, d_traj3, _ = _rollout(eng, obs_np, traj_np, dev, device_loss)
        assert torch.equal(final3, final) and torch.equal(d_obs3, d_obs) and (d_traj is None or torch.equal(d_traj3, d_traj))


def test_differentiable_rollout_with_two_candidates(dev):
    """candidates = 2: each scene's end state and gradients are the single-scene call's, bit for bit."""
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    names = ["step_a", "step_b"]
    device_loss, _ = _weighted(dev)
    single = [_rollout(_engine(m, dev), gc.step_state(s), rc.trajectory(s), dev, device_loss) for s in names]
    w = gc.weights(gc.step_state("step_a").shape, 6)
    w2 = _t(np.concatenate((w, w), axis=1), dev)
    both = np.concatenate([gc.step_state(s) for s in names], axis=1)
    traj = np.concatenate([rc.trajectory(s) for s in names], axis=1)
    final, _, d_obs, d_traj, eis = _rollout(_engine(m, dev, candidates=2), both, traj, dev, lambda f: (f * w2).sum())
    n, nr = gc.STEP_N, rc.trajectory("step_a").shape[1]
    for b in range(2):
        rows = slice(b * n, (b + 1) * n)
        assert torch.equal(final[:, rows], single[b][0]), b
        assert torch.equal(d_obs[:, rows], single[b][2]), b
        assert torch.equal(d_traj[:, b * nr:(b + 1) * nr], single[b][3]), b
    for t in range(rc.T):
        e0 = single[0][4][t].shape[1]
        assert np.array_equal(eis[t][:, :e0], single[0][4][t]) and np.array_equal(eis[t][:, e0:], single[1][4][t] + n)


# ------------------------------------------------------------------------------------------ 4. constant memory
def test_rollout_memory_does_not_grow_with_the_horizon(dev):
    """Peak memory of forward + backward at T = 6 and at T = 2 differ by less than half a tape.  An unrolled chain keeps every
    step's tape until backward() and differs by four; the reverse sweep keeps one tape whatever T, and four more windows and poses
    (k N D and n_rigid 3 floats each: under 0.1 MB here)."""
    from gnn_manip_amd._lib import ModelDesc, lib
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    traj = rc.trajectory("step_a", 3, 6)
    device_loss, _ = _weighted(dev)
    _rollout(eng, obs_np, traj[:2], dev, device_loss, steps=2)          # one-time allocations (weight images, the engine's own)
    peaks, edges = {}, 0
    for steps in (6, 2):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        *_, eis = _rollout(eng, obs_np, traj[:steps], dev, device_loss, steps=steps)
        torch.cuda.synchronize()
        peaks[steps] = torch.cuda.max_memory_allocated(dev) - base
        edges = max(edges, max(e.shape[1] for e in eis))
    tape = lib().gm_train_tape_bytes(C.byref(ModelDesc(*m.model_desc())), gc.STEP_N, edges)
    print(f"\n[rollout grads] peak above the start: T=6 {peaks[6]} B, T=2 {peaks[2]} B, difference {peaks[6] - peaks[2]} B; one tape {tape} B")
    assert peaks[2] > tape                                               # the measurement sees the tape at all
    assert abs(peaks[6] - peaks[2]) < tape / 2


# ------------------------------------------------------------------------------------------ 5. the planner's objective
@pytest.mark.parametrize("what", ["inside the limits", "one rotation increment clipped"])
def test_loss_and_grad(dev, what):
    s, obs_np, init, fluid, cloud = _solver(dev)
    x = np.concatenate((s.sample_traj[:, 0], s.sample_traj[:, 1])) * 1.1
    if what != "inside the limits":
        x[1] = -1.5 * s.max_rot
    eis = []
    loss, grad = s.loss_and_grad(x, edges=eis)
    eis = [e.cpu().numpy() for e in eis]
    assert len(eis) == 4 and grad.shape == x.shape and all(p.grad is None for p in s.model.parameters())
    value = s.cma_objective(x)
    print(f"\n[rollout grads] loss_and_grad {what}: {loss:.9e}, cma_objective {value:.9e}")
    assert abs(loss - value) <= 1e-5 * abs(value)
    ref, g64, end_grad = _objective_reference(s, x, obs_np, init, fluid, cloud, eis, torch.float64)
    _, g32, _ = _objective_reference(s, x, obs_np, init, fluid, cloud, eis, torch.float32)
    print(f"[rollout grads] float64 objective {ref:.9e}; gradient {grad}, float64 {g64}")
    leaf = gc.t64(x, True)
    allow = _lazy(lambda: flip_allowance(lambda fwd: _objective_reference(s, leaf, obs_np, init, fluid, cloud, eis, torch.float64, fwd, end_grad),
                                         [leaf]))
    _within(f"loss_and_grad {what}", grad, g64, g32, lambda: (allow()[0][0], allow()[1]))
    if what != "inside the limits":
        assert grad[1] == 0.0 and g64[1] == 0.0 and np.count_nonzero(grad) == len(x) - 1


def test_interpolated_solver_has_no_gradient(dev):
    from gnn_manip_amd.planner import InterpolatedCMAsolver
    s = _solver(dev, InterpolatedCMAsolver)[0]
    with pytest.raises(NotImplementedError):
        s.loss_and_grad(np.zeros(4))
