"""The reverse sweep of a rollout inside the library, on the MI355X: gm_state_pre_backward / gm_state_post_backward,
gm_rollout_step_backward, gm_rollout_backward, and the Python layer on top (RolloutEngine.step_backward,
differentiable_rollout(sweep="library"), TrajectoryCMAsolver.loss_and_grad(sweep="library")).

Yardsticks.  The state transposes copy, negate or add two float32 terms: the device result IS the float32 restatement of
tests/rollout_vjp_cases.py (checked on the CPU), bit for bit.  Gradients through the model: the rule of
tests/yardstick.py (`within`), the flip allowance per element, against the float64 restatements of tests/grad_cases.py (one step) and
tests/rollout_grad_cases.py (reverse_sweep), on the edge lists get_connectivity returns for the pre-step positions: the same kernel
on the same input as the library's own list.  Every figure is printed before it is asserted."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import BOUNDS, STATS
import grad_cases as gc
import rollout_grad_cases as rc
import rollout_vjp_cases as vc
from gpu_support import (K_NB, dev, edges_of as _edges_of, feature_desc, forward_windows as _forward_windows, load_model as _model,
                         step_call as _step_call, step_engine as _engine, step_solver as _solver, sweep_call as _sweep_call, to_dev as _t)
from grad_cases import L0, flip_allowance, split as _split, step_allowance as _step_allowance, step_reference as _step_reference
from rollout_grad_cases import objective_reference as _objective_reference
from yardstick import bits as _bits, lazy as _lazy, same_bits as _same_bits, within as _within

pytestmark = pytest.mark.gpu

W_SEED = 6


# ------------------------------------------------------------------------------------------ 1. the state transposes alone
def _state_transposes(g_np, L, rank_np, has_target, dev):
    """Both transposes on outputs pre-filled with NaN: (pre: d_obs, d_target), (post: d_obs, d_next, d_target)."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    fd = feature_desc(gc.R, L)
    n = g_np.shape[1]
    nr = int((rank_np >= 0).sum())
    g, rank = _t(g_np, dev), _t(rank_np, dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)
    pre = (nan(*g.shape), nan(nr, 3) if nr else None)
    check(lib().gm_state_pre_backward(ptr(g), n, C.byref(fd), ptr(rank), int(has_target), ptr(pre[0]), ptr(pre[1]), current_stream(dev)))
    post = (nan(*g.shape), nan(n, 3), nan(nr, 3) if nr else None)
    check(lib().gm_state_post_backward(ptr(g), n, C.byref(fd), ptr(rank), int(has_target), ptr(post[0]), ptr(post[1]), ptr(post[2]),
                                       current_stream(dev)))
    return pre, post


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_state_transposes_are_the_float32_restatement(dev, case):
    n, k, rigid, has_target = case
    L = vc.LAYOUTS[k]
    rank = vc.rigid_rank(n, rigid)
    g = vc.gradient(n, k, 7 * n + k)
    pre, post = _state_transposes(g, L, rank, has_target, dev)
    pre2, post2 = _state_transposes(g, L, rank, has_target, dev)
    want_pre = vc.state_pre_transpose(g, L, rank, has_target)
    want_post = vc.state_post_transpose(g, L, rank, has_target)
    for what, got, again, want in (("pre", pre, pre2, want_pre), ("post", post, post2, want_post)):
        for i, w in enumerate(want):
            if got[i] is None:
                assert w.size == 0
                continue
            assert torch.isfinite(got[i]).all(), (what, i)              # every element written
            assert _same_bits(got[i], w), (what, i, np.abs(got[i].cpu().numpy() - w).max())
            assert _same_bits(got[i], again[i]), (what, i)


def test_state_transposes_without_a_rank_or_a_target_buffer(dev):
    """gm_state_post_backward with rigid_rank NULL treats every row as non-rigid; a NULL d_rigid_target is skipped."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L, n = vc.LAYOUTS[6], 257
    g_np = vc.gradient(n, 6, 5)
    g, fd = _t(g_np, dev), feature_desc(gc.R, L)
    d_obs, d_next = torch.full_like(g, float("nan")), torch.full((n, 3), float("nan"), device=dev)
    check(lib().gm_state_post_backward(ptr(g), n, C.byref(fd), None, 1, ptr(d_obs), ptr(d_next), None, current_stream(dev)))
    want = vc.state_post_transpose(g_np, L, vc.rigid_rank(n, "none"), True)
    assert _same_bits(d_obs, want[0]) and _same_bits(d_next, want[1])
    rank_np = vc.rigid_rank(n, "all")
    rank = _t(rank_np, dev)
    d_obs2 = torch.full_like(g, float("nan"))
    check(lib().gm_state_pre_backward(ptr(g), n, C.byref(fd), ptr(rank), 1, ptr(d_obs2), None, current_stream(dev)))
    assert _same_bits(d_obs2, vc.state_pre_transpose(g_np, L, rank_np, True)[0])


def test_state_transposes_refuse_bad_arguments(dev):
    from gnn_manip_amd._lib import current_stream, lib, ptr
    from gnn_manip_amd.graph import make_feature_desc
    import width_cases as wc
    Ln = wc.LAYOUTS["no_control"]
    fd_n = make_feature_desc(gc.R, STATS, BOUNDS, Ln.cart_idx, [Ln.mat], None, Ln.k, Ln.D)
    n = 65
    g = torch.zeros((Ln.k, n, Ln.D), device=dev)
    out, rank = torch.full_like(g, 7.0), _t(vc.rigid_rank(n, "one"), dev)
    L = lib()
    assert L.gm_state_pre_backward(ptr(g), n, C.byref(fd_n), ptr(rank), 1, ptr(out), None, current_stream(dev)) == -1
    assert L.gm_last_error() == b"gm_state_pre_backward: descriptor has no control columns"
    fd = feature_desc(gc.R, vc.LAYOUTS[6])
    assert L.gm_state_pre_backward(ptr(g), n, C.byref(fd), None, 1, ptr(out), None, current_stream(dev)) == -1       # no rank
    assert L.gm_last_error() == b"gm_state_pre_backward: null pointer"
    assert L.gm_state_pre_backward(None, n, C.byref(fd), ptr(rank), 1, ptr(out), None, current_stream(dev)) == -1
    assert L.gm_state_post_backward(ptr(g), n, C.byref(fd), ptr(rank), 1, ptr(out), None, None, current_stream(dev)) == -1   # no d_next_pos
    assert L.gm_last_error() == b"gm_state_post_backward: null pointer"
    assert L.gm_state_post_backward(ptr(g), n, C.byref(fd), ptr(rank), 1, ptr(g), ptr(out), None, current_stream(dev)) == -1    # in place
    torch.cuda.synchronize()
    assert float(out.min()) == 7.0 and float(out.max()) == 7.0                                       # nothing was launched


# ------------------------------------------------------------------------------------------ 2. the step
@functools.lru_cache(maxsize=None)
def _weights():
    w = gc.weights(gc.step_state("step_a").shape, W_SEED)
    w.setflags(write=False)
    return w


def _end_grad(final):
    return _weights()


_STEP_REF = {}


def _step_refs(name, with_target, ei):
    """float64 and float32 restatement gradients of one step of scene `name` on the edge list `ei`, computed once."""
    key = (name, with_target)
    if key not in _STEP_REF:
        obs_np = gc.step_state(name)
        target = gc.rigid_target(obs_np, L0, 3) if with_target else None
        r64 = _step_reference(rc.params(), obs_np, [target], [ei], None, None, torch.float64, _end_grad)
        r32 = _step_reference(rc.params(), obs_np, [target], [ei], None, None, torch.float32, _end_grad)
        _STEP_REF[key] = (ei, r64[2], r64[3][0], r32[2], r32[3][0])
    assert np.array_equal(_STEP_REF[key][0], ei)
    return _STEP_REF[key][1:]


@pytest.mark.parametrize("with_target", [True, False])
@pytest.mark.parametrize("name", ["step_a", "step_b"])
def test_step_vjp(dev, name, with_target):
    from gnn_manip_amd.graph import _ws
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state(name)
    target_np = gc.rigid_target(obs_np, L0, 3) if with_target else None
    obs = _t(obs_np, dev)
    assert eng.set_scene(obs) == len(gc.rigid_rows(obs_np, L0)) > 0
    tgt = _t(target_np, dev) if with_target else None
    g = _t(_weights(), dev)
    d_obs, d_tgt, e = _step_call(eng, obs, tgt, g, dev)
    assert torch.equal(obs, _t(obs_np, dev))                                   # the pre-step window is an input
    ei = _edges_of(obs, eng)
    print(f"\n[rollout vjp] {name}: edges {e}, get_connectivity {ei.shape[1]}")
    assert e == ei.shape[1]
    g_obs, g_t, g_obs32, g_t32 = _step_refs(name, with_target, ei)
    # for information: the autograd composition of the same entry points
    with torch.enable_grad():
        o = obs.clone().requires_grad_(True)
        t = tgt.clone().requires_grad_(True) if with_target else None
        nxt, _, ei2 = eng.differentiable_step(o, t, inputs_only=True)
        auto = torch.autograd.grad(nxt, [o, t] if with_target else [o], grad_outputs=g)
    assert np.array_equal(ei2.cpu().numpy(), ei)
    print(f"[rollout vjp] {name}: max |library - autograd| d_obs {float((d_obs - auto[0]).abs().max()):.3e}"
          + (f", d_rigid_target {float((d_tgt - auto[1]).abs().max()):.3e}" if with_target else ""))
    allow = _step_allowance(rc.params(), obs_np, [target_np], [ei], None, None, end_grad=_weights())
    what = f"step vjp {name}" + (" with target" if with_target else "")
    _split(what, d_obs.cpu().numpy(), g_obs, g_obs32, allow)
    if with_target:
        _within(f"{what} d_rigid_target", d_tgt.cpu().numpy(), g_t, g_t32, lambda: (allow()[0][1], allow()[1]))
    # the same call again, and in a workspace of 0xff bytes: the same bits (nothing is read that the call did not write)
    again = _step_call(eng, obs, tgt, g, dev)
    h, tensors, t_arr, md = eng._training_model()
    from gnn_manip_amd._lib import lib
    need = lib().gm_rollout_step_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    dirty = _step_call(eng, obs, tgt, g, dev, ws=_ws(need, dev).fill_(0xff))
    for other in (again, dirty):
        assert other[2] == e and _same_bits(other[0], d_obs)
        assert d_tgt is None or _same_bits(other[1], d_tgt)
    # the engine's wrapper is the same call
    w_obs, w_tgt, w_e = eng.step_backward(obs, tgt, g, return_edge_count=True)
    assert w_e == e and _same_bits(w_obs, d_obs) and (w_tgt is None) == (d_tgt is None)
    assert d_tgt is None or _same_bits(w_tgt, d_tgt)
    with pytest.raises(ValueError):
        eng.step_backward(obs, tgt, g[:, :-1].contiguous())


# ------------------------------------------------------------------------------------------ 3. two candidates
def test_step_vjp_with_two_candidates(dev):
    """nodes_per_graph = 400 over step_a | step_b: each scene's rows are the single-scene call's, bit for bit."""
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    names = ["step_a", "step_b"]
    scenes = [gc.step_state(s) for s in names]
    targets = [gc.rigid_target(s, L0, 3 + i) for i, s in enumerate(scenes)]
    w = _weights()
    single = []
    for s, t in zip(scenes, targets):
        eng = _engine(m, dev)
        eng.set_scene(_t(s, dev))
        single.append(_step_call(eng, _t(s, dev), _t(t, dev), _t(w, dev), dev))
    eng2 = _engine(m, dev, candidates=2)
    assert eng2.fdesc.nodes_per_graph == gc.STEP_N
    both = _t(np.concatenate(scenes, axis=1), dev)
    eng2.set_scene(both)
    d_obs, d_tgt, e = _step_call(eng2, both, _t(np.concatenate(targets), dev), _t(np.concatenate((w, w), axis=1), dev), dev)
    assert e == single[0][2] + single[1][2]
    n, nr = gc.STEP_N, targets[0].shape[0]
    for b in range(2):
        assert _same_bits(d_obs[:, b * n:(b + 1) * n], single[b][0]), b
        assert _same_bits(d_tgt[b * nr:(b + 1) * nr], single[b][1]), b


# ------------------------------------------------------------------------------------------ 4. the whole sweep
@pytest.mark.parametrize("with_trajectory", [True, False])
def test_rollout_backward(dev, with_trajectory):
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    traj_np = rc.trajectory("step_a") if with_trajectory else None
    windows, final = _forward_windows(eng, obs_np, traj_np, rc.T, dev)
    with torch.no_grad():
        plain = eng.rollout(_t(obs_np, dev), None if traj_np is None else _t(traj_np, dev), horizon=rc.T)
    assert torch.equal(final, plain)
    eis = [_edges_of(windows[t], eng) for t in range(rc.T)]
    tr = None if traj_np is None else _t(traj_np, dev)
    g = _t(_weights(), dev)
    d_obs0, d_traj = _sweep_call(eng, windows, tr, rc.T, g, dev)
    _, g_obs, g_tr = rc.reverse_sweep(obs_np, traj_np, eis, _end_grad)
    _, g_obs32, g_tr32 = rc.reverse_sweep(obs_np, traj_np, eis, _end_grad, dtype=torch.float32)
    targets = [None] * rc.T if traj_np is None else list(traj_np)
    allow = _step_allowance(rc.params(), obs_np, targets, eis, None, None, end_grad=_weights())
    what = "sweep" + (" with trajectory" if with_trajectory else "")
    _split(what, d_obs0.cpu().numpy(), g_obs, g_obs32, allow)
    if with_trajectory:
        for t in range(rc.T):
            _within(f"{what} d_trajectory[{t}]", d_traj[t].cpu().numpy(), g_tr[t], g_tr32[t], lambda t=t: (allow()[0][1 + t], allow()[1]))
    again = _sweep_call(eng, windows, tr, rc.T, g, dev)
    assert _same_bits(again[0], d_obs0) and (d_traj is None or _same_bits(again[1], d_traj))
    # the sweep is the loop of the step: its last step by hand
    _, t3, _ = _step_call(eng, windows[rc.T - 1], None if tr is None else tr[rc.T - 1], g, dev)
    if with_trajectory:
        assert _same_bits(t3, d_traj[rc.T - 1])
    # fewer steps than poses: the later rows of d_trajectory are exactly zero, the earlier ones those of the shorter trajectory
    if with_trajectory:
        short = _sweep_call(eng, windows, tr, 2, g, dev)
        assert not _bits(short[1][2:]).any()
        cut = _sweep_call(eng, windows, tr[:2].contiguous(), 2, g, dev)
        assert _same_bits(short[0], cut[0]) and _same_bits(short[1][:2], cut[1])
        no_out = _sweep_call(eng, windows, tr, rc.T, g, dev, want_traj=False)      # d_trajectory NULL
        assert no_out[1] is None and _same_bits(no_out[0], d_obs0)
    none = _sweep_call(eng, windows, tr, 0, g, dev)                                # no steps: d_final comes back
    assert _same_bits(none[0], g) and (none[1] is None or not _bits(none[1]).any())


def test_sweeps_of_any_length_run_in_the_same_workspace(dev):
    """The workspace query takes no horizon; a T = 6 sweep and a T = 2 sweep run in one buffer of exactly that size, and the T = 2
    result is the one a fresh buffer gives."""
    from gnn_manip_amd._lib import ModelDesc, lib
    from gnn_manip_amd.graph import _ws
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    traj = rc.trajectory("step_a", 3, 6)
    md = ModelDesc(*m.model_desc())
    need = lib().gm_rollout_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    step = lib().gm_rollout_step_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    window = 4 * L0.k * gc.STEP_N * L0.D
    print(f"\n[rollout vjp] workspace: step {step} B, sweep {need} B, one window {window} B")
    assert step < need <= step + 2 * (window + 256)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    g = _t(_weights(), dev)
    res = {}
    for steps in (6, 2):
        windows, _ = _forward_windows(eng, obs_np, traj[:steps], steps, dev)
        res[steps] = _sweep_call(eng, windows, _t(traj[:steps], dev), steps, g, dev, ws=ws)
        assert torch.isfinite(res[steps][0]).all() and torch.isfinite(res[steps][1]).all()
        if steps == 2:
            fresh = _sweep_call(eng, windows, _t(traj[:2], dev), 2, g, dev)
            assert _same_bits(fresh[0], res[2][0]) and _same_bits(fresh[1], res[2][1])
    assert not _same_bits(res[6][0], res[2][0])


# ------------------------------------------------------------------------------------------ 5. the Python layer
def _rollout(eng, obs_np, traj_np, dev, **kw):
    obs = _t(obs_np, dev).requires_grad_(True)
    tr = None if traj_np is None else _t(traj_np, dev).requires_grad_(True)
    final = eng.differentiable_rollout(obs, tr, horizon=rc.T, **kw)
    assert final.grad_fn is not None
    (final * _t(_weights(), dev)).sum().backward()
    return final.detach(), obs.grad, None if tr is None else tr.grad


@pytest.mark.parametrize("with_trajectory", [True, False])
def test_differentiable_rollout_with_the_library_sweep(dev, with_trajectory):
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    traj_np = rc.trajectory("step_a") if with_trajectory else None
    final0, d_obs0, d_traj0 = _rollout(eng, obs_np, traj_np, dev)
    final, d_obs, d_traj = _rollout(eng, obs_np, traj_np, dev, sweep="library")
    assert torch.equal(final, final0)
    assert all(p.grad is None for p in m.parameters())
    print(f"\n[rollout vjp] library against autograd sweep: d_obs {float((d_obs - d_obs0).abs().max()):.3e}"
          + (f", d_trajectory {float((d_traj - d_traj0).abs().max()):.3e}" if with_trajectory else ""))
    windows, _ = _forward_windows(eng, obs_np, traj_np, rc.T, dev)
    eis = [_edges_of(windows[t], eng) for t in range(rc.T)]
    _, g_obs, g_tr = rc.reverse_sweep(obs_np, traj_np, eis, _end_grad)
    _, g_obs32, g_tr32 = rc.reverse_sweep(obs_np, traj_np, eis, _end_grad, dtype=torch.float32)
    targets = [None] * rc.T if traj_np is None else list(traj_np)
    allow = _step_allowance(rc.params(), obs_np, targets, eis, None, None, end_grad=_weights())
    what = "library sweep" + (" with trajectory" if with_trajectory else "")
    _split(what, d_obs.cpu().numpy(), g_obs, g_obs32, allow)
    if with_trajectory:
        assert d_traj.shape == d_traj0.shape
        for t in range(rc.T):
            _within(f"{what} d_trajectory[{t}]", d_traj[t].cpu().numpy(), g_tr[t], g_tr32[t], lambda t=t: (allow()[0][1 + t], allow()[1]))
    _, d_obs2, d_traj2 = _rollout(eng, obs_np, traj_np, dev, sweep="library")
    assert _same_bits(d_obs2, d_obs) and (d_traj is None or _same_bits(d_traj2, d_traj))
    obs = _t(obs_np, dev).requires_grad_(True)
    with pytest.raises(ValueError, match="return_edges"):
        eng.differentiable_rollout(obs, None, horizon=rc.T, return_edges=True, sweep="library")
    with pytest.raises(ValueError, match="sweep"):
        eng.differentiable_rollout(obs, None, horizon=rc.T, sweep="tape")


def test_loss_and_grad_with_the_library_sweep(dev):
    """test_gpu_rollout_grad.test_loss_and_grad's bars, with the reverse sweep in the library: the value is cma_objective's to 1e-5,
    the gradient is within the rule (`_within`) of the float64 objective on the edge lists of the default sweep's recomputation (the same
    windows, hence the same graphs)."""
    s, obs_np, init, fluid, cloud = _solver(dev)
    x = np.concatenate((s.sample_traj[:, 0], s.sample_traj[:, 1])) * 1.1
    eis = []
    loss0, grad0 = s.loss_and_grad(x, edges=eis)
    eis = [e.cpu().numpy() for e in eis]
    loss, grad = s.loss_and_grad(x, sweep="library")
    assert grad.shape == x.shape and all(p.grad is None for p in s.model.parameters())
    value = s.cma_objective(x)
    print(f"\n[rollout vjp] loss_and_grad library {loss:.9e}, autograd {loss0:.9e}, cma_objective {value:.9e}; gradient {grad}, autograd {grad0}")
    assert abs(loss - value) <= 1e-5 * abs(value)
    ref, g64, end_grad = _objective_reference(s, x, obs_np, init, fluid, cloud, eis, torch.float64)
    _, g32, _ = _objective_reference(s, x, obs_np, init, fluid, cloud, eis, torch.float32)
    leaf = gc.t64(x, True)
    allow = _lazy(lambda: flip_allowance(lambda fwd: _objective_reference(s, leaf, obs_np, init, fluid, cloud, eis, torch.float64, fwd, end_grad),
                                         [leaf]))
    _within("loss_and_grad library sweep", grad, g64, g32, lambda: (allow()[0][0], allow()[1]))
    with pytest.raises(ValueError, match="return_edges"):
        s.loss_and_grad(x, edges=[], sweep="library")
