"""CPU: the references and the bindings of the library's reverse sweep.  The float32 transposes of the two state updates
(tests/rollout_vjp_cases.py) are float64 autograd's gradients through grad_cases.state_pre / state_post; the new entry points are
declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the built library, and
refuse their arguments before any device call.

Bar of the transposes: an element is a copy, a negation or ONE float32 addition of two float32 terms, so it differs from the
float64 value by at most 2^-24 of that value (round to nearest), and is zero exactly where that is."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
import grad_cases as gc
import rollout_vjp_cases as vc
from rollout_vjp_cases import ctype as _ctype

NEW_SYMBOLS = ("gm_state_pre_backward", "gm_state_post_backward", "gm_rollout_step_backward_workspace_bytes", "gm_rollout_step_backward",
               "gm_rollout_backward_workspace_bytes", "gm_rollout_backward")


def _close(got, ref64):
    got = np.asarray(got, np.float64)
    assert got.shape == ref64.shape
    assert (np.abs(got - ref64) <= 2.0 ** -24 * np.abs(ref64)).all()


@pytest.mark.parametrize("case", vc.CASES, ids=vc.case_id)
def test_state_transposes_are_autograds_gradients(case):
    n, k, rigid, has_target = case
    L = vc.LAYOUTS[k]
    rank = vc.rigid_rank(n, rigid)
    rows = torch.tensor(np.nonzero(rank >= 0)[0])
    nr = len(rows)
    rng = np.random.default_rng(n + k)
    g = vc.gradient(n, k, 7 * n + k)
    obs = gc.t64(rng.standard_normal((k, n, L.D)), True)
    tgt = gc.t64(rng.standard_normal((nr, 3)), True) if has_target else None
    nxt = gc.t64(rng.standard_normal((n, 3)), True)

    leaves = [obs] + ([tgt] if has_target else [])
    ref = torch.autograd.grad(gc.state_pre(obs, L, rows, tgt), leaves, grad_outputs=gc.t64(g), allow_unused=True)
    d_obs, d_tgt = vc.state_pre_transpose(g, L, rank, has_target)
    _close(d_obs, ref[0].numpy())
    assert d_tgt.shape == (nr, 3) and d_tgt.dtype == np.float32
    _close(d_tgt, ref[1].numpy() if has_target and nr else np.zeros((nr, 3)))

    leaves = [obs, nxt] + ([tgt] if has_target else [])
    ref = torch.autograd.grad(gc.state_post(obs, L, nxt, rows, tgt), leaves, grad_outputs=gc.t64(g), allow_unused=True)
    d_obs, d_nxt, d_tgt = vc.state_post_transpose(g, L, rank, has_target)
    _close(d_obs, ref[0].numpy())
    _close(d_nxt, ref[1].numpy())
    _close(d_tgt, ref[2].numpy() if has_target and nr else np.zeros((nr, 3)))
    assert not d_obs[0].any()                                       # the frame that fell out of the window


def test_cases_cover_the_launch_edges():
    assert set(vc.SIZES) >= {1, 63, 64, 65, 257, 1000} and set(vc.KS) == {2, 6} and set(vc.RIGID) == {"none", "one", "all"}
    assert len(vc.CASES) == len(vc.SIZES) * 2 * 3 * 2
    for k, L in vc.LAYOUTS.items():
        assert L.k == k and L.ctrl >= 0
    r = vc.rigid_rank(65, "one")
    assert (r >= 0).sum() == 1 and r[0] == -1
    assert np.array_equal(np.sort(vc.rigid_rank(65, "all")), np.arange(65))


# ------------------------------------------------------------------------------------------ the bindings
@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    from gnn_manip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\b%s\s*\(" % name, header), "not declared in the header"
    assert name in _lib.PROTOTYPES, "not bound in _lib.py"
    assert hasattr(_lib.lib(), name), "not exported by the library"
    assert _lib.lib().gm_abi_version() == 7


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_binding_has_the_headers_signature(name):
    """Parameter by parameter: the declaration in the header against the argtypes in _lib.py (pointers to the two descriptors and to
    the int64 the edge count comes back in are typed, every other pointer is void*)."""
    from gnn_manip_amd import _lib
    header = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ret, params = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, header).groups()
    want = [_ctype(" ".join(p.split())) for p in params.split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is (C.c_int if ret == "int" else C.c_size_t)
    assert args == want, (name, args, want)


def _fdesc(control=True):
    from gnn_manip_amd.graph import make_feature_desc
    from conftest import BOUNDS, STATS
    L = vc.LAYOUTS[6]
    return make_feature_desc(gc.R, STATS, BOUNDS, L.cart_idx, [L.mat], L.ctrl_idx if control else None, L.k, L.D)


def test_state_transposes_check_their_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    assert L.gm_state_pre_backward(None, 5, None, None, 1, None, None, None) == -1
    assert L.gm_last_error() == b"gm_state_pre_backward: null feature descriptor"
    assert L.gm_state_pre_backward(None, 5, C.byref(fd), None, 1, None, None, None) == -1
    assert L.gm_last_error() == b"gm_state_pre_backward: null pointer"
    assert L.gm_state_pre_backward(None, 0, C.byref(fd), None, 1, None, None, None) == 0          # no rows: nothing to write
    assert L.gm_state_pre_backward(None, 5, C.byref(_fdesc(control=False)), None, 1, None, None, None) == -1
    assert L.gm_last_error() == b"gm_state_pre_backward: descriptor has no control columns"
    assert L.gm_state_post_backward(None, 5, None, None, 0, None, None, None, None) == -1
    assert L.gm_last_error() == b"gm_state_post_backward: null feature descriptor"
    assert L.gm_state_post_backward(None, 5, C.byref(fd), None, 0, None, None, None, None) == -1
    assert L.gm_last_error() == b"gm_state_post_backward: null pointer"
    assert L.gm_state_post_backward(None, -1, C.byref(fd), None, 0, None, None, None, None) == -1
    assert L.gm_state_post_backward(None, 0, C.byref(fd), None, 0, None, None, None, None) == 0
    assert L.gm_state_post_backward(None, 0, C.byref(_fdesc(control=False)), None, 0, None, None, None, None) == 0   # no control: fine here


def test_step_and_sweep_check_their_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    for name in ("gm_rollout_step_backward", "gm_rollout_backward"):
        args = [None if t in (C.c_void_p, _lib._FD, C.POINTER(C.c_int64)) else 0 for t in _lib.PROTOTYPES[name][1]]
        assert getattr(L, name)(*args) == -1, name
        assert L.gm_last_error() == f"{name}: null pointer".encode()


def test_workspace_queries_take_no_horizon_and_nest():
    """The queries' arguments are the two descriptors, n_nodes and max_neighbours: there is no horizon to depend on.  The sweep's
    workspace is the step's plus two gradient windows (k N D floats each, 256-byte aligned)."""
    from gnn_manip_amd import _lib
    L = _lib.lib()
    for name in ("gm_rollout_step_backward_workspace_bytes", "gm_rollout_backward_workspace_bytes"):
        assert _lib.PROTOTYPES[name][1] == [_lib._MD, _lib._FD, C.c_int64, C.c_int]
    md = _lib.ModelDesc(*gc.STEP_DIMS, 1e-5)
    fd = _fdesc()
    n, K = gc.STEP_N, 20
    step = L.gm_rollout_step_backward_workspace_bytes(C.byref(md), C.byref(fd), n, K)
    sweep = L.gm_rollout_backward_workspace_bytes(C.byref(md), C.byref(fd), n, K)
    window = -(-fd.k_steps * n * fd.data_dim * 4 // 256) * 256
    assert step >= L.gm_train_tape_bytes(C.byref(md), n, n * K) + L.gm_train_backward_inputs_workspace_bytes(C.byref(md), n, n * K)
    assert sweep == step + 2 * window
    assert L.gm_rollout_step_backward_workspace_bytes(None, C.byref(fd), n, K) == 0
    assert L.gm_rollout_backward_workspace_bytes(C.byref(md), None, n, K) == 0
    assert L.gm_rollout_backward_workspace_bytes(C.byref(md), C.byref(fd), -1, K) == 0


def test_python_keyword_is_checked_before_anything_runs():
    """sweep= is validated before the engine looks at its tensors: an unknown value and return_edges with the library sweep raise
    ValueError (no device needed: the engine object is not even built)."""
    from gnn_manip_amd.rollout import RolloutEngine
    eng = object.__new__(RolloutEngine)
    with pytest.raises(ValueError, match="sweep"):
        RolloutEngine.differentiable_rollout(eng, None, sweep="tape")
    with pytest.raises(ValueError, match="return_edges"):
        RolloutEngine.differentiable_rollout(eng, None, return_edges=True, sweep="library")
