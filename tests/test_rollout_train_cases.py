"""CPU: the references and the bindings of training through a rollout (tests/rollout_train_cases.py).  In float64 the restated
sweep -- one step at a time, the record's gradient joining before state_pre's transpose, parameter gradients accumulated from the
last step to the first -- equals plain autograd through the unrolled chain, to tests/test_rollout_grad_cases.py's bar for the
existing sweep (1e-12 of the tensor's largest entry), for d_obs0, d_trajectory and every parameter; the identity the forward takes
its records by holds on the oracle's rollout; the cases reach what they are there for; the two new entry points are declared,
bound with the header's signatures, exported, and refuse their arguments before any device call."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import BOUNDS, ROOT, STATS
from oracle import epd_oracle as orc
import grad_cases as gc
import rollout_grad_cases as rc
import rollout_train_cases as tc
from rollout_vjp_cases import ctype as _ctype

NEW_SYMBOLS = ("gm_rollout_step_backward_train", "gm_rollout_backward_train")
BAR = 1e-12              # tests/test_rollout_grad_cases.py: test_reverse_sweep_is_autograd_through_the_unrolled_chain


@functools.lru_cache(maxsize=None)
def _both(with_trajectory, with_records):
    """(reference, restated sweep) of step_a on the oracle's edge lists, computed once."""
    obs = gc.step_state("step_a")
    tr = rc.trajectory("step_a") if with_trajectory else None
    eis = rc.oracle_edge_lists("step_a", with_trajectory)
    wr = tc.record_weights() if with_records else None
    ref = tc.reference(rc.params(), obs, tr, eis, tc.F64, tc.final_weights(), wr)
    got = tc.reverse_sweep(rc.params(), obs, tr, eis, tc.final_weights(), wr)
    return ref, got


@pytest.mark.parametrize("with_records", [True, False], ids=["records", "no_records"])
@pytest.mark.parametrize("with_trajectory", [True, False], ids=["trajectory", "no_trajectory"])
def test_restated_sweep_is_autograd_through_the_unrolled_chain(with_trajectory, with_records):
    (final, records, g_obs, g_tr, g_p), (final2, records2, s_obs, s_tr, s_p) = _both(with_trajectory, with_records)
    assert np.array_equal(final, final2) and np.array_equal(records, records2)    # frame k-2 of the next window IS the record
    assert records.shape == (tc.T,) + final.shape[1:]
    assert np.abs(s_obs - g_obs).max() <= BAR * np.abs(g_obs).max()
    if with_trajectory:
        assert np.abs(g_tr).max(axis=(1, 2)).min() > 0
        assert np.abs(s_tr - g_tr).max() <= BAR * np.abs(g_tr).max()
    else:
        assert g_tr is None and s_tr is None
    assert set(s_p) == set(g_p) == set(rc.params())
    for k, g in g_p.items():
        assert np.abs(g).max() > 0, k                                             # every parameter takes part
        assert np.abs(s_p[k] - g).max() <= BAR * np.abs(g).max(), k


def test_sweep_without_parameters_is_the_existing_sweep():
    """with_params=False and no records: tests/rollout_grad_cases.reverse_sweep's numbers (the same algorithm, the step written out)."""
    obs, tr, eis = gc.step_state("step_a"), rc.trajectory("step_a"), rc.oracle_edge_lists("step_a", True)
    final, _, d_obs, d_tr, d_p = tc.reverse_sweep(rc.params(), obs, tr, eis, tc.final_weights(), None, with_params=False)
    final0, d_obs0, d_tr0 = rc.reverse_sweep(obs, tr, eis, rc.weighted_sum())
    assert d_p is None and np.array_equal(final, final0)
    assert np.abs(d_obs - d_obs0).max() <= BAR * np.abs(d_obs0).max() and np.abs(d_tr - d_tr0).max() <= BAR * np.abs(d_tr0).max()


def test_record_is_frame_k_minus_2_of_the_next_window_on_the_oracles_rollout():
    """oracle/epd_oracle.rollout's records against its own states: record[t] is frame k-2 of the state after step t, bit for bit
    (the window shift moves the last frame there unchanged)."""
    obs, tr = gc.step_state("step_a"), rc.trajectory("step_a")
    args = (STATS, BOUNDS, gc.R, rc.L0.cart_idx, [rc.L0.mat], rc.L0.ctrl_idx, gc.STEP_DIMS[4], gc.STEP_DIMS[5])
    _, recs = orc.rollout(rc.params(), obs, tr, tc.T, *args, record=True)
    assert recs.shape == (tc.T,) + obs.shape[1:]
    for t in range(tc.T):
        after = orc.rollout(rc.params(), obs, tr, t + 1, *args)
        assert np.array_equal(after[-2].view(np.uint32), recs[t].view(np.uint32)), t
        assert not np.array_equal(after[-1], recs[t])                              # and not the frame the step wrote


def test_record_weights_reach_every_column_they_can():
    """A gradient on ONE record: it passes through to d_obs0's last frame only for t = 0; on the last step's record alone it moves
    d_trajectory[T-1] (through state_pre's transpose: control = pose - xyz) and leaves the earlier poses' gradients as they were
    when the final-state term is absent; every w_t moves d_obs0 and the parameters' gradients of steps <= t."""
    obs, tr, eis = gc.step_state("step_a"), rc.trajectory("step_a"), rc.oracle_edge_lists("step_a", True)
    zero_final = np.zeros_like(tc.final_weights())
    rows = gc.rigid_rows(obs, rc.L0)
    u = slice(rc.L0.ctrl, rc.L0.ctrl + 3)
    for t in range(tc.T):
        wr = np.zeros_like(tc.record_weights())
        wr[t] = tc.record_weights()[t]
        _, _, d_obs, d_tr, d_p = tc.reverse_sweep(rc.params(), obs, tr, eis, zero_final, wr)
        assert np.abs(d_obs).max() > 0, t
        assert all(np.abs(d_tr[s]).max() > 0 for s in range(t + 1)), t            # the pose of every step up to t, step t's included
        assert not d_tr[t + 1:].any(), t                                          # and of no later step
        # step t's pose enters record t only through the control columns of the rigid rows: exactly w_t there
        if t == tc.T - 1:
            assert np.abs(d_tr[t] - wr[t][rows][:, u]).max() <= BAR * np.abs(wr[t]).max()
        if t == 0:      # record 0 is a function of the initial window and pose 0 alone: no parameter, every column of the last frame
            assert all(not g.any() for g in d_p.values())
            free = [c for c in range(rc.L0.D) if not (u.start <= c < u.stop)]
            assert (d_obs[-1][:, free] != 0).all()
        else:
            assert all(np.abs(g).max() > 0 for g in d_p.values()), t


# ------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    from gnn_manip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, header), "not declared in the header"
    assert name in _lib.PROTOTYPES, "not bound in _lib.py"
    assert hasattr(_lib.lib(), name), "not exported by the library"
    assert _lib.lib().gm_abi_version() == 7                                      # a pure addition


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_binding_has_the_headers_signature(name):
    """Parameter by parameter, as tests/test_rollout_vjp_cases.py does for the existing pair; and the new entry point's parameters
    are the existing one's with d_record(s) and grads after the upstream gradient."""
    from gnn_manip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ret, params = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header).groups()
    names = [" ".join(p.split()) for p in params.split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is C.c_int and ret == "int"
    assert args == [_ctype(p) for p in names], (name, args)
    old = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name[:-len("_train")], header).group(1)
    old = [" ".join(p.split()) for p in old.split(",")]
    at = next(i for i, p in enumerate(names) if p.split()[-1] in ("d_record", "d_records"))
    assert names[:at] + names[at + 2:] == old
    assert names[at].startswith("const float*") and names[at + 1] == "float* const* grads"
    assert names[at - 1].split()[-1] in ("d_obs_after", "d_final")


def _null_args(name):
    from gnn_manip_amd import _lib
    return [None if t in (C.c_void_p, _lib._FD, C.POINTER(C.c_int64)) else 0 for t in _lib.PROTOTYPES[name][1]]


def test_new_entry_points_check_their_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    for name in NEW_SYMBOLS:
        assert getattr(L, name)(*_null_args(name)) == -1, name
        assert L.gm_last_error() == f"{name}: null pointer".encode()
    # the existing pair still speaks under its own names
    for name in ("gm_rollout_step_backward", "gm_rollout_backward"):
        assert getattr(L, name)(*_null_args(name)) == -1, name
        assert L.gm_last_error() == f"{name}: null pointer".encode()


def test_python_keywords_are_checked_before_anything_runs():
    """record= / params= with the autograd sweep raise ValueError before the engine looks at its tensors (no device needed: the
    engine object is not even built); the existing keyword checks still come first."""
    from gnn_manip_amd.rollout import RolloutEngine
    eng = object.__new__(RolloutEngine)
    for kw in (dict(record=True), dict(params=True), dict(record=True, params=True), dict(record=True, sweep="autograd")):
        with pytest.raises(ValueError, match="sweep='library'"):
            RolloutEngine.differentiable_rollout(eng, None, **kw)
    with pytest.raises(ValueError, match="sweep must be"):
        RolloutEngine.differentiable_rollout(eng, None, sweep="tape", record=True)
    import inspect
    sig = inspect.signature(RolloutEngine.differentiable_rollout).parameters
    assert sig["sweep"].default == "autograd" and sig["record"].default is False and sig["params"].default is False
    sig = inspect.signature(RolloutEngine.step_backward).parameters
    assert sig["d_record"].default is None and sig["grads"].default is None
