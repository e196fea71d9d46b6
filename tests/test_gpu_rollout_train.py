"""Training through a rollout on the MI355X: gm_rollout_step_backward_train, gm_rollout_backward_train and the Python layer on top
(RolloutEngine.step_backward(d_record=, grads=), differentiable_rollout(sweep="library", record=, params=)).

Yardstick: the rule of tests/yardstick.py (`within`; grad_cases.split for d_obs), the flip allowance per element (computed for this
input, parameters among the leaves) -- against the float64 restatement of tests/rollout_train_cases.py (reverse_sweep, checked
on the CPU) on the edge lists get_connectivity returns for each pre-step window: the same kernel on the same input as the library's
own list.  Where two calls run the same launches on the same operands the comparison is bit for bit.  Every figure is printed
before it is asserted.

Zeros as a record gradient: x + (-0) is x for every float x, bits included, so a d_record of negative zeros reproduces the plain
call bit for bit; x + (+0) differs from x in the one case x = -0 (the sum is +0), so a d_record of zeros reproduces its values."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import grad_cases as gc
import rollout_grad_cases as rc
import rollout_train_cases as tc
from oracle import epd_oracle as orc
from gpu_support import (K_NB, dev, edges_of as _edges_of, forward_windows as _forward_windows, load_model as _model,
                         step_call as _step_call, step_engine as _engine, sweep_call as _sweep_call, to_dev as _t)
from grad_cases import L0, flip_allowance, split as _split
from yardstick import bits as _bits, lazy as _lazy, same_bits as _same_bits, within as _within

pytestmark = pytest.mark.gpu

NAMES = list(rc.params())        # the state_dict's order, which is the order of `tensors` and `grads`


# ------------------------------------------------------------------------------------------ the calls
def _zero_grads(tensors):
    grads = [torch.zeros_like(t) for t in tensors]
    return grads, (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])


def _step_train(eng, obs, tgt, g, dev, d_record=None, with_grads=False, ws=None):
    """gm_rollout_step_backward_train through ctypes, outputs pre-filled with NaN, grads zeroed: (d_obs, d_target, edges, grads)."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    from gnn_manip_amd.graph import _ws
    L = lib()
    h, tensors, t_arr, md = eng._training_model()
    need = L.gm_rollout_step_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    ws = _ws(need, dev) if ws is None else ws
    assert need > 0 and ws.numel() >= need
    grads, g_arr = _zero_grads(tensors) if with_grads else (None, None)
    d_obs = torch.full_like(obs, float("nan"))
    d_tgt = None if tgt is None else torch.full_like(tgt, float("nan"))
    e = C.c_int64(-1)
    check(L.gm_rollout_step_backward_train(h, t_arr, len(tensors), ptr(obs), eng.n, C.byref(eng.fdesc), K_NB, ptr(eng.rigid_rank), ptr(tgt),
                                           ptr(g), ptr(d_record), g_arr, ptr(d_obs), ptr(d_tgt), C.byref(e), ptr(ws), need,
                                           current_stream(dev)))
    return d_obs, d_tgt, int(e.value), grads


def _sweep_train(eng, windows, traj, steps, d_final, dev, d_records=None, with_grads=False, ws=None, grads=None):
    """gm_rollout_backward_train through ctypes: (d_obs0, d_trajectory, grads).  grads: buffers to accumulate into (else zeroed)."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    from gnn_manip_amd.graph import _ws
    L = lib()
    h, tensors, t_arr, md = eng._training_model()
    need = L.gm_rollout_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    ws = _ws(need, dev) if ws is None else ws
    assert need > 0 and ws.numel() >= need
    g_arr = None
    if grads is not None:
        g_arr = (C.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    elif with_grads:
        grads, g_arr = _zero_grads(tensors)
    d_obs0 = torch.full_like(d_final, float("nan"))
    d_traj = None if traj is None else torch.full_like(traj, float("nan"))
    check(L.gm_rollout_backward_train(h, t_arr, len(tensors), ptr(windows), eng.n, C.byref(eng.fdesc), K_NB, ptr(eng.rigid_rank), ptr(traj),
                                      0 if traj is None else traj.shape[0], eng.n_rigid, steps, ptr(d_final), ptr(d_records), g_arr,
                                      ptr(d_obs0), ptr(d_traj), ptr(ws), need, current_stream(dev)))
    return d_obs0, d_traj, grads


def _same_grads(a, b):
    return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------ the references
_REFS = {}


def _refs(key, params_np, obs_np, traj_np, eis, w_final, w_records):
    """float64 and float32 restated sweeps on the edge lists `eis`, computed once per key."""
    if key not in _REFS:
        r64 = tc.reverse_sweep(params_np, obs_np, traj_np, eis, w_final, w_records)
        r32 = tc.reverse_sweep(params_np, obs_np, traj_np, eis, w_final, w_records, dtype=torch.float32)
        _REFS[key] = ([np.array(e) for e in eis], r64, r32)
    kept = _REFS[key][0]
    assert len(kept) == len(eis) and all(np.array_equal(a, b) for a, b in zip(kept, eis)), key
    return _REFS[key][1], _REFS[key][2]


def _allowance(params_np, obs_np, targets, eis, w_final, w_records):
    """flip_allowance of the unrolled loss with the parameters among the leaves, evaluated at most once: a function returning
    dict(obs=, targets=[...], params={name: ...}, units=) of per-element bounds."""
    def compute():
        p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params_np.items()}
        obs = gc.t64(obs_np, True)
        tg = None if targets is None else [gc.t64(t, True) for t in targets]

        def run(fwd):
            final, recs = tc.unrolled(p, obs, tg, eis, forward=fwd)
            return tc.loss_of(final, recs, w_final, w_records)
        bounds, units = flip_allowance(run, [obs] + (tg or []) + list(p.values()))
        nt = len(tg or [])
        return dict(obs=bounds[0], targets=bounds[1:1 + nt], params=dict(zip(p, bounds[1 + nt:])), units=units)
    return _lazy(compute)


def _hold(what, got, r64, r32, allow, with_params):
    """(d_obs0, d_trajectory, grads) of a device call against the two restated sweeps, tensor by tensor."""
    d_obs, d_traj, grads = got
    a = allow
    _split(what, d_obs.cpu().numpy(), r64[2], r32[2], lambda: ([a()["obs"]], a()["units"]))
    if r64[3] is not None:
        for t in range(len(r64[3])):
            _within(f"{what} d_trajectory[{t}]", d_traj[t].cpu().numpy(), r64[3][t], r32[3][t], lambda t=t: (a()["targets"][t], a()["units"]))
    if with_params:
        assert len(grads) == len(NAMES)
        for name, g in zip(NAMES, grads):
            _within(f"{what} {name}", g.detach().cpu().numpy(), r64[4][name], r32[4][name], lambda name=name: (a()["params"][name], a()["units"]))


def _scene(name, with_target, dev, m=None):
    m = m or _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state(name)
    target_np = gc.rigid_target(obs_np, L0, 3) if with_target else None
    obs = _t(obs_np, dev)
    assert eng.set_scene(obs) == len(gc.rigid_rows(obs_np, L0)) > 0
    return m, eng, obs_np, target_np, obs, (_t(target_np, dev) if with_target else None)


# ------------------------------------------------------------------------------------------ 1. the step
def _chain_by_hand(eng, obs, tgt, g, dev):
    """The step's parameter gradients from the same entry points, called one by one: gm_state_pre, gm_node_features, the radius
    graph, gm_edge_features, gm_epd_forward_train, gm_state_post_backward, gm_integrate_backward, gm_epd_backward_inputs."""
    from gnn_manip_amd import get_connectivity, get_edges_displacement
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    from gnn_manip_amd.graph import _node_features, _ws
    L, fd, n, s = lib(), eng.fdesc, eng.n, current_stream(dev)
    h, tensors, t_arr, md = eng._training_model()
    pre = obs.clone()
    check(L.gm_state_pre(ptr(pre), n, C.byref(fd), ptr(eng.rigid_rank), ptr(tgt), s))
    nodes = _node_features(pre, fd)
    pos = pre[-1][:, L0.cart:L0.cart + 3]
    snd, rcv = get_connectivity(pos, gc.R, K_NB, eng.n_per if eng.candidates > 1 else None)
    ea = get_edges_displacement(pos, snd, rcv, gc.R).contiguous()
    ei = torch.stack((snd, rcv)).contiguous()
    e = int(ei.shape[1])
    tape = _ws(L.gm_train_tape_bytes(C.byref(md), n, e), dev)
    pred = torch.empty((n, 3), device=dev)
    check(L.gm_epd_forward_train(h, ptr(nodes), n, ptr(ea), ptr(ei), e, ptr(pred), ptr(tape), tape.numel(), s))
    g_post, d_next, t_post = torch.empty_like(obs), torch.empty((n, 3), device=dev), torch.empty((max(eng.n_rigid, 1), 3), device=dev)
    check(L.gm_state_post_backward(ptr(g), n, C.byref(fd), ptr(eng.rigid_rank), int(tgt is not None), ptr(g_post), ptr(d_next), ptr(t_post), s))
    d_pred, g_int = torch.empty((n, 3), device=dev), torch.empty_like(obs)
    check(L.gm_integrate_backward(ptr(d_next), n, C.byref(fd), ptr(d_pred), ptr(g_int), s))
    grads, g_arr = _zero_grads(tensors)
    ws = _ws(L.gm_train_backward_inputs_workspace_bytes(C.byref(md), n, e), dev)
    d_nodes, d_ea = torch.empty_like(nodes), torch.empty_like(ea)
    check(L.gm_epd_backward_inputs(h, t_arr, len(tensors), ptr(nodes), ptr(ea), n, e, ptr(d_pred), g_arr, ptr(d_nodes),
                                   ptr(d_ea), ptr(tape), tape.numel(), ptr(ws), ws.numel(), s))
    torch.cuda.synchronize()
    return grads, e


@pytest.mark.parametrize("with_target", [True, False], ids=["target", "no_target"])
@pytest.mark.parametrize("name", ["step_a", "step_b"])
def test_step_with_parameter_gradients_and_a_record(dev, name, with_target):
    m, eng, obs_np, target_np, obs, tgt = _scene(name, with_target, dev)
    g = _t(tc.final_weights(), dev)
    plain = _step_call(eng, obs, tgt, g, dev)                                    # gm_rollout_step_backward
    null = _step_train(eng, obs, tgt, g, dev)                                    # both new pointers NULL
    assert null[2] == plain[2] and _same_bits(null[0], plain[0]) and (tgt is None or _same_bits(null[1], plain[1]))
    # ---- grads into zeroed buffers: the window's and the pose's gradients keep their bits
    got = _step_train(eng, obs, tgt, g, dev, with_grads=True)
    assert got[2] == plain[2] and _same_bits(got[0], plain[0]) and (tgt is None or _same_bits(got[1], plain[1]))
    ei = _edges_of(obs, eng)
    assert got[2] == ei.shape[1]
    by_hand, e = _chain_by_hand(eng, obs, tgt, g, dev)
    assert e == got[2]
    for k, a, b in zip(NAMES, got[3], by_hand):
        assert _same_bits(a, b), (k, float((a - b).abs().max()))
    traj_np = None if target_np is None else target_np[None]
    what = f"step {name}" + (" with target" if with_target else "")
    r64, r32 = _refs(("step", name, with_target, False), rc.params(), obs_np, traj_np, [ei], tc.final_weights(), None)
    allow = _allowance(rc.params(), obs_np, None if target_np is None else [target_np], [ei], tc.final_weights(), None)
    _hold(what, (got[0], None if tgt is None else got[1][None], got[3]), r64, r32, allow, True)
    # ---- a gradient on the record, no grads
    w_rec = tc.record_weights()[:1]
    rec = _step_train(eng, obs, tgt, g, dev, d_record=_t(w_rec[0], dev))
    r64, r32 = _refs(("step", name, with_target, True), rc.params(), obs_np, traj_np, [ei], tc.final_weights(), w_rec)
    allow = _allowance(rc.params(), obs_np, None if target_np is None else [target_np], [ei], tc.final_weights(), w_rec)
    _hold(what + " record", (rec[0], None if tgt is None else rec[1][None], None), r64, r32, allow, False)
    assert not _same_bits(rec[0][-1], plain[0][-1]) and _same_bits(rec[0][:-1], plain[0][:-1])       # the last frame alone
    both = _step_train(eng, obs, tgt, g, dev, d_record=_t(w_rec[0], dev), with_grads=True)
    assert _same_bits(both[0], rec[0]) and (tgt is None or _same_bits(both[1], rec[1]))
    assert _same_grads(both[3], got[3])                 # one step: the record joins behind the model, no parameter sees it
    # ---- zeros
    zeros = torch.zeros((eng.n, L0.D), device=dev)
    neg = _step_train(eng, obs, tgt, g, dev, d_record=-zeros)
    assert _bits(-zeros).min() == 0x80000000
    assert _same_bits(neg[0], plain[0]) and (tgt is None or _same_bits(neg[1], plain[1]))
    pos = _step_train(eng, obs, tgt, g, dev, d_record=zeros)
    assert torch.equal(pos[0], plain[0]) and (tgt is None or torch.equal(pos[1], plain[1]))
    # ---- the engine's wrapper is the same call
    grads = [torch.zeros_like(t) for t in eng._training_model()[1]]
    w_obs, w_tgt = eng.step_backward(obs, tgt, g, d_record=_t(w_rec[0], dev), grads=grads)
    assert _same_bits(w_obs, both[0]) and (tgt is None or _same_bits(w_tgt, both[1])) and _same_grads(grads, both[3])
    with pytest.raises(ValueError):
        eng.step_backward(obs, tgt, g, d_record=zeros[:, :-1].contiguous())
    with pytest.raises(ValueError):
        eng.step_backward(obs, tgt, g, grads=grads[:-1])


# ------------------------------------------------------------------------------------------ 2. the sweep
def _sweep_setup(dev, with_trajectory, name="step_a", steps=tc.T):
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state(name)
    traj_np = rc.trajectory(name) if with_trajectory else None
    windows, final = _forward_windows(eng, obs_np, traj_np, steps, dev)
    eis = [_edges_of(windows[t], eng) for t in range(steps)]
    return m, eng, obs_np, traj_np, windows, eis, (None if traj_np is None else _t(traj_np, dev))


@pytest.mark.parametrize("with_records", [True, False], ids=["records", "no_records"])
@pytest.mark.parametrize("with_trajectory", [True, False], ids=["trajectory", "no_trajectory"])
def test_sweep_with_records_and_parameter_gradients(dev, with_trajectory, with_records):
    m, eng, obs_np, traj_np, windows, eis, tr = _sweep_setup(dev, with_trajectory)
    g = _t(tc.final_weights(), dev)
    w_rec = tc.record_weights() if with_records else None
    d_rec = _t(w_rec, dev) if with_records else None
    off = _sweep_train(eng, windows, tr, tc.T, g, dev, d_records=d_rec)
    on = _sweep_train(eng, windows, tr, tc.T, g, dev, d_records=d_rec, with_grads=True)
    assert _same_bits(on[0], off[0]) and (tr is None or _same_bits(on[1], off[1]))           # grads change no other bit
    if not with_records:                                                                    # both new pointers NULL: the existing call
        plain = _sweep_call(eng, windows, tr, tc.T, g, dev)
        assert _same_bits(off[0], plain[0]) and (tr is None or _same_bits(off[1], plain[1]))
    key = ("sweep", with_trajectory, with_records)
    r64, r32 = _refs(key, rc.params(), obs_np, traj_np, eis, tc.final_weights(), w_rec)
    allow = _allowance(rc.params(), obs_np, None if traj_np is None else list(traj_np), eis, tc.final_weights(), w_rec)
    what = "train sweep" + (" with trajectory" if with_trajectory else "") + (" with records" if with_records else "")
    _hold(what, on, r64, r32, allow, True)


def test_sweep_is_repeatable_needs_no_clean_workspace_and_reads_only_its_steps(dev):
    from gnn_manip_amd._lib import lib
    from gnn_manip_amd.graph import _ws
    m, eng, obs_np, traj_np, windows, eis, tr = _sweep_setup(dev, True)
    g, d_rec = _t(tc.final_weights(), dev), _t(tc.record_weights(), dev)
    first = _sweep_train(eng, windows, tr, tc.T, g, dev, d_records=d_rec, with_grads=True)
    again = _sweep_train(eng, windows, tr, tc.T, g, dev, d_records=d_rec, with_grads=True)
    md = eng._training_model()[3]
    need = lib().gm_rollout_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    dirty = _sweep_train(eng, windows, tr, tc.T, g, dev, d_records=d_rec, with_grads=True, ws=_ws(need, dev).fill_(0xff))
    for other in (again, dirty):
        assert _same_bits(other[0], first[0]) and _same_bits(other[1], first[1]) and _same_grads(other[2], first[2])
    assert all(torch.isfinite(x).all() for x in first[2]) and any(float(x.abs().max()) > 0 for x in first[2])
    # ---- no steps: grads untouched, d_final comes back, d_records not read
    sevens = [torch.full_like(t, 7.0) for t in eng._training_model()[1]]
    nan_rec = torch.full_like(d_rec, float("nan"))
    none = _sweep_train(eng, windows, tr, 0, g, dev, d_records=nan_rec, grads=sevens)
    assert _same_bits(none[0], g) and not _bits(none[1]).any()
    assert all(float(x.min()) == 7.0 and float(x.max()) == 7.0 for x in sevens)
    # ---- two steps of four poses: the later rows of d_trajectory are zero, the records of steps 2 and 3 are not read
    half = d_rec.clone()
    half[2:] = float("nan")
    short = _sweep_train(eng, windows, tr, 2, g, dev, d_records=half, with_grads=True)
    assert not _bits(short[1][2:]).any()
    assert torch.isfinite(short[0]).all() and torch.isfinite(short[1]).all() and all(torch.isfinite(x).all() for x in short[2])
    cut = _sweep_train(eng, windows[:2].contiguous(), tr[:2].contiguous(), 2, g, dev, d_records=d_rec[:2].contiguous(), with_grads=True)
    assert _same_bits(short[0], cut[0]) and _same_bits(short[1][:2], cut[1]) and _same_grads(short[2], cut[2])
    # ---- a one-step sweep is the step entry point, parameter gradients included
    one = _sweep_train(eng, windows, tr, 1, g, dev, d_records=d_rec, with_grads=True)
    step = _step_train(eng, windows[0], tr[0], g, dev, d_record=d_rec[0], with_grads=True)
    assert _same_bits(one[0], step[0]) and _same_bits(one[1][0], step[1]) and _same_grads(one[2], step[3])
    # ---- accumulation: the sweep's parameter gradients are its steps' added from the last to the first
    acc = [torch.zeros_like(t) for t in eng._training_model()[1]]
    g_after = g
    for t in range(tc.T - 1, -1, -1):
        part = _sweep_train(eng, windows[t:t + 1].contiguous(), tr[t:t + 1].contiguous(), 1, g_after, dev,
                            d_records=d_rec[t:t + 1].contiguous(), grads=acc)
        g_after = part[0]
    assert _same_bits(g_after, first[0]) and _same_grads(acc, first[2])


# ------------------------------------------------------------------------------------------ 3. two candidates
def test_step_with_two_candidates(dev):
    """nodes_per_graph = 400 over step_a | step_b: each scene's rows of d_obs are the single-scene call's, bit for bit; a parameter
    gradient sums over both scenes and is held to the sum of the two float64 references."""
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    names = ["step_a", "step_b"]
    scenes = [gc.step_state(s) for s in names]
    targets = [gc.rigid_target(s, L0, 3 + i) for i, s in enumerate(scenes)]
    w, w_rec = tc.final_weights(), tc.record_weights()[0]
    single, refs, allows = [], [], []
    for i, (s, t) in enumerate(zip(scenes, targets)):
        eng = _engine(m, dev)
        eng.set_scene(_t(s, dev))
        single.append(_step_train(eng, _t(s, dev), _t(t, dev), _t(w, dev), dev, d_record=_t(w_rec, dev), with_grads=True))
        ei = _edges_of(_t(s, dev), eng)
        refs.append(_refs(("two", i), rc.params(), s, t[None], [ei], w, w_rec[None]))
        allows.append(_allowance(rc.params(), s, [t], [ei], w, w_rec[None]))
    eng2 = _engine(m, dev, candidates=2)
    assert eng2.fdesc.nodes_per_graph == gc.STEP_N
    both = _t(np.concatenate(scenes, axis=1), dev)
    eng2.set_scene(both)
    d_obs, d_tgt, e, grads = _step_train(eng2, both, _t(np.concatenate(targets), dev), _t(np.concatenate((w, w), axis=1), dev), dev,
                                         d_record=_t(np.concatenate((w_rec, w_rec)), dev), with_grads=True)
    assert e == single[0][2] + single[1][2]
    n, nr = gc.STEP_N, targets[0].shape[0]
    for b in range(2):
        assert _same_bits(d_obs[:, b * n:(b + 1) * n], single[b][0]), b
        assert _same_bits(d_tgt[b * nr:(b + 1) * nr], single[b][1]), b
    for k, name in enumerate(NAMES):
        g64 = refs[0][0][4][name] + refs[1][0][4][name]
        g32 = refs[0][1][4][name] + refs[1][1][4][name]
        _within(f"two candidates {name}", grads[k].cpu().numpy(), g64, g32,
                lambda name=name: (allows[0]()["params"][name] + allows[1]()["params"][name], allows[0]()["units"] + allows[1]()["units"]))


# ------------------------------------------------------------------------------------------ 4. the Python layer
def _train_rollout(eng, m, obs_np, traj_np, dev, record, params, w_rec, grad_inputs=True):
    for p in m.parameters():
        p.grad = None
    obs = _t(obs_np, dev).requires_grad_(grad_inputs)
    tr = None if traj_np is None else _t(traj_np, dev).requires_grad_(grad_inputs)
    out = eng.differentiable_rollout(obs, tr, horizon=tc.T, sweep="library", record=record, params=params)
    final, records = out if record else (out, None)
    loss = (final * _t(tc.final_weights(), dev)).sum()
    if record and w_rec is not None:
        loss = loss + (records * _t(w_rec, dev)).sum()
    loss.backward()
    return final.detach(), None if records is None else records.detach(), obs.grad, None if tr is None else tr.grad


def test_differentiable_rollout_trains(dev):
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np, traj_np = gc.step_state("step_a"), rc.trajectory("step_a")
    w_rec = tc.record_weights()
    with torch.no_grad():
        plain, recs = eng.rollout(_t(obs_np, dev), _t(traj_np, dev), horizon=tc.T, record=True)
    final, records, d_obs, d_traj = _train_rollout(eng, m, obs_np, traj_np, dev, True, True, w_rec)
    assert _same_bits(final, plain) and records.shape == recs.shape and _same_bits(records, recs)
    grads = [p.grad.clone() for p in m.parameters()]
    assert [k for k, _ in m.named_parameters()] == NAMES and all(g.shape == p.shape for g, p in zip(grads, m.parameters()))
    windows, _ = _forward_windows(eng, obs_np, traj_np, tc.T, dev)
    eis = [_edges_of(windows[t], eng) for t in range(tc.T)]
    r64, r32 = _refs(("sweep", True, True), rc.params(), obs_np, traj_np, eis, tc.final_weights(), w_rec)
    allow = _allowance(rc.params(), obs_np, list(traj_np), eis, tc.final_weights(), w_rec)
    _hold("differentiable_rollout record params", (d_obs, d_traj, grads), r64, r32, allow, True)
    # the same through the library call on the same windows: bit for bit
    lib_call = _sweep_train(eng, windows, _t(traj_np, dev), tc.T, _t(tc.final_weights(), dev), dev, d_records=_t(w_rec, dev), with_grads=True)
    assert _same_bits(d_obs, lib_call[0]) and _same_bits(d_traj, lib_call[1]) and _same_grads(grads, lib_call[2])
    # ---- nobody has to set requires_grad on obs0
    _train_rollout(eng, m, obs_np, traj_np, dev, True, True, w_rec, grad_inputs=False)
    assert _same_grads([p.grad for p in m.parameters()], grads)
    # ---- params=False: the parameters are constants
    f2, r2, d_obs2, d_traj2 = _train_rollout(eng, m, obs_np, traj_np, dev, True, False, w_rec)
    assert all(p.grad is None for p in m.parameters())
    assert _same_bits(f2, plain) and _same_bits(r2, recs) and _same_bits(d_obs2, d_obs) and _same_bits(d_traj2, d_traj)
    # ---- params=True without record: one output, the existing library sweep's input gradients
    f3, r3, d_obs3, d_traj3 = _train_rollout(eng, m, obs_np, traj_np, dev, False, True, None)
    assert r3 is None and _same_bits(f3, plain) and all(p.grad is not None for p in m.parameters())
    r64n, r32n = _refs(("sweep", True, False), rc.params(), obs_np, traj_np, eis, tc.final_weights(), None)
    allow_n = _allowance(rc.params(), obs_np, list(traj_np), eis, tc.final_weights(), None)
    _hold("differentiable_rollout params", (d_obs3, d_traj3, [p.grad for p in m.parameters()]), r64n, r32n, allow_n, True)
    # ---- a record the loss does not touch
    grads3 = [p.grad.clone() for p in m.parameters()]
    f4, r4, d_obs4, d_traj4 = _train_rollout(eng, m, obs_np, traj_np, dev, True, True, None)
    assert _same_bits(r4, recs) and _same_bits(d_obs4, d_obs3) and _same_bits(d_traj4, d_traj3)
    assert _same_grads([p.grad for p in m.parameters()], grads3)
    # ---- for information: a plain autograd unroll of differentiable_step (four tapes)
    for p in m.parameters():
        p.grad = None
    obs, tr = _t(obs_np, dev).requires_grad_(True), _t(traj_np, dev).requires_grad_(True)
    cur, loss = obs, 0.0
    for t in range(tc.T):
        nxt, _, _ = eng.differentiable_step(cur, tr[t])
        loss = loss + (nxt[-2] * _t(w_rec[t], dev)).sum()
        cur = nxt
    (loss + (cur * _t(tc.final_weights(), dev)).sum()).backward()
    worst = max(float((p.grad - g).abs().max() / g.abs().max()) for p, g in zip(m.parameters(), grads))
    print(f"\n[rollout train] autograd unroll against the library sweep: d_obs {float((obs.grad - d_obs).abs().max()):.3e}, "
          f"d_trajectory {float((tr.grad - d_traj).abs().max()):.3e}, worst parameter tensor (relative) {worst:.3e}")
    with pytest.raises(ValueError, match="sweep='library'"):
        eng.differentiable_rollout(obs, tr, horizon=tc.T, record=True)


@functools.lru_cache(maxsize=None)
def _params48():
    return orc.init_params(25, 4, 3, 48, 2, 2, 843)


def test_differentiable_rollout_trains_at_a_hidden_size_between_the_widths(dev):
    """Hidden 48 runs zero-padded at 64: the padded tensors are built under autograd, the gradients arrive in the checkpoint's
    shapes and are held to float64 on the UNPADDED model."""
    dims = (25, 4, 3, 48, 2, 2)
    m = _model(_params48(), dims, dev)
    eng = _engine(m, dev)
    obs_np, traj_np = gc.step_state("step_a"), rc.trajectory("step_a")
    w_rec = tc.record_weights()
    final, records, d_obs, d_traj = _train_rollout(eng, m, obs_np, traj_np, dev, True, True, w_rec)
    with torch.no_grad():
        plain, recs = eng.rollout(_t(obs_np, dev), _t(traj_np, dev), horizon=tc.T, record=True)
    assert _same_bits(final, plain) and _same_bits(records, recs)
    names = [k for k, _ in m.named_parameters()]
    assert names == list(_params48())
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert all(grads[k] is not None and tuple(grads[k].shape) == _params48()[k].shape for k in names)
    windows, _ = _forward_windows(eng, obs_np, traj_np, tc.T, dev)
    eis = [_edges_of(windows[t], eng) for t in range(tc.T)]
    r64, r32 = _refs(("hidden 48",), _params48(), obs_np, traj_np, eis, tc.final_weights(), w_rec)
    a = _allowance(_params48(), obs_np, list(traj_np), eis, tc.final_weights(), w_rec)
    _split("hidden 48", d_obs.cpu().numpy(), r64[2], r32[2], lambda: ([a()["obs"]], a()["units"]))
    for t in range(tc.T):
        _within(f"hidden 48 d_trajectory[{t}]", d_traj[t].cpu().numpy(), r64[3][t], r32[3][t], lambda t=t: (a()["targets"][t], a()["units"]))
    for k in names:
        _within(f"hidden 48 {k}", grads[k].cpu().numpy(), r64[4][k], r32[4][k], lambda k=k: (a()["params"][k], a()["units"]))


# ------------------------------------------------------------------------------------------ 5. memory
def test_training_memory_does_not_grow_with_the_horizon(dev):
    """tests/test_gpu_rollout_grad.py's test_rollout_memory_does_not_grow_with_the_horizon with params=True, record=True: what the
    forward keeps (windows, records) grows with T; the backward's peak above that -- one tape, one backward workspace, ONE set of
    parameter gradients -- differs between T = 6 and T = 2 by less than half a tape."""
    from gnn_manip_amd._lib import ModelDesc, lib
    m = _model(rc.params(), gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    traj = rc.trajectory("step_a", 3, 6)
    w_f = _t(tc.final_weights(), dev)
    w_r = _t(tc.record_weights(6), dev)

    def forward(steps):
        obs, tr = _t(obs_np, dev).requires_grad_(True), _t(traj[:steps], dev).requires_grad_(True)
        final, records = eng.differentiable_rollout(obs, tr, horizon=steps, sweep="library", record=True, params=True)
        return (final * w_f).sum() + (records * w_r[:steps]).sum(), eng.status()

    forward(2)[0].backward()          # one-time allocations (weight images, the engine's own, the backward workspace)
    peaks, kept, edges = {}, {}, 0
    for steps in (6, 2):
        for p in m.parameters():
            p.grad = None
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated(dev)
        loss, e = forward(steps)
        torch.cuda.synchronize()
        kept[steps] = torch.cuda.memory_allocated(dev) - base
        torch.cuda.reset_peak_memory_stats(dev)
        loss.backward()
        torch.cuda.synchronize()
        peaks[steps] = torch.cuda.max_memory_allocated(dev) - base - kept[steps]
        edges = max(edges, e)
        del loss
    tape = lib().gm_train_tape_bytes(C.byref(ModelDesc(*m.model_desc())), gc.STEP_N, edges)
    window = 4 * L0.k * gc.STEP_N * L0.D
    print(f"\n[rollout train] kept by the forward: T=6 {kept[6]} B, T=2 {kept[2]} B (one window {window} B); backward peak above it: "
          f"T=6 {peaks[6]} B, T=2 {peaks[2]} B, difference {peaks[6] - peaks[2]} B; one tape {tape} B")
    assert kept[6] - kept[2] >= 4 * window                               # the forward's arrays do grow: four more windows
    assert peaks[2] > sum(p.numel() for p in m.parameters()) * 4         # the measurement sees the set of parameter gradients
    assert abs(peaks[6] - peaks[2]) < tape / 2
