"""CPU: the bindings of the evaluation entry points (gm_state_recorded, gm_rollout_recorded, gm_rollout_errors): declared in
include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the built library -- an addition
to ABI 7 -- and refusing their arguments before any device call."""
import ctypes as C
import os
import re

import pytest

from conftest import BOUNDS, ROOT, STATS
import eval_cases as ec

NEW_SYMBOLS = ("gm_state_recorded", "gm_rollout_recorded", "gm_rollout_errors")


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the two descriptors are typed, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        if decl.startswith("const gm_feature_desc"):
            return _lib._FD
        if decl.startswith("const gm_model_desc"):
            return _lib._MD
        return C.c_void_p
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t}[decl.rsplit(" ", 1)[0]]


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_symbol_is_declared_bound_and_exported(name):
    from gnn_manip_amd import _lib
    assert re.search(r"\b%s\s*\(" % name, _header()), "not declared in the header"
    assert name in _lib.PROTOTYPES, "not bound in _lib.py"
    assert hasattr(_lib.lib(), name), "not exported by the library"
    assert _lib.lib().gm_abi_version() == 7


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_binding_has_the_headers_signature(name):
    from gnn_manip_amd import _lib
    ret, params = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, _header()).groups()
    want = [_ctype(p) for p in params.split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is (C.c_int if ret == "int" else C.c_size_t)
    assert args == want, (name, args, want)


def test_header_constants_are_the_cases():
    h = _header()
    assert re.search(r"#define\s+GM_RECORDED_CONTROL\s+%d\b" % ec.GM_RECORDED_CONTROL, h)
    assert re.search(r"#define\s+GM_RECORDED_POSE\s+%d\b" % ec.GM_RECORDED_POSE, h)


def _fdesc(control=True, n_per=0):
    from gnn_manip_amd.graph import make_feature_desc
    L = ec.ROW_LAYOUTS[6]
    d = make_feature_desc(ec.R, STATS, BOUNDS, L.cart_idx, [L.mat], L.ctrl_idx if control else None, L.k, L.D)
    d.nodes_per_graph = n_per
    return d


def test_state_recorded_checks_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    assert L.gm_state_recorded(None, 5, None, None, None, None, 1, None) == -1
    assert L.gm_last_error() == b"gm_state_recorded: null feature descriptor"
    assert L.gm_state_recorded(None, 5, C.byref(fd), None, None, None, 2, None) == -1
    assert b"what=2" in L.gm_last_error()
    assert L.gm_state_recorded(None, 5, C.byref(_fdesc(control=False)), None, None, None, ec.GM_RECORDED_CONTROL, None) == -1
    assert L.gm_last_error() == b"gm_state_recorded: descriptor has no control columns"
    assert L.gm_state_recorded(None, 5, C.byref(fd), None, None, None, ec.GM_RECORDED_POSE, None) == -1
    assert L.gm_last_error() == b"gm_state_recorded: null pointer"
    for what in (ec.GM_RECORDED_CONTROL, ec.GM_RECORDED_POSE):
        assert L.gm_state_recorded(None, 0, C.byref(fd), None, None, None, what, None) == 0     # no rows: nothing to write
    assert L.gm_state_recorded(None, 0, C.byref(_fdesc(control=False)), None, None, None, ec.GM_RECORDED_POSE, None) == 0


def test_rollout_recorded_checks_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    args = [None if t in (C.c_void_p, _lib._FD) else 0 for t in _lib.PROTOTYPES["gm_rollout_recorded"][1]]
    assert L.gm_rollout_recorded(*args) == -1
    assert L.gm_last_error() == b"gm_rollout_recorded: null pointer"


# a recording of 10 frames: which (first_frame, steps) gm_rollout_errors takes, with and without record_pred
ERRORS_RANGES = [(1, 8, True, True), (1, 9, True, False), (0, 1, True, False), (9, 0, True, True), (10, 0, True, False),
                 (0, 10, False, True), (0, 11, False, False), (1, 9, False, True), (10, 0, False, True), (11, 0, False, False),
                 (-1, 1, False, False), (3, -1, False, False)]


@pytest.mark.parametrize("first,steps,with_pred,ok", ERRORS_RANGES)
def test_rollout_errors_refuses_frames_outside_the_recording(first, steps, with_pred, ok):
    """The range check comes before any pointer is read: steps = 0 / n = 0 return GM_OK, a bad range GM_ERR_INVALID_ARGUMENT."""
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    pred = C.c_void_p(256) if with_pred else None          # never read: n_nodes = 0
    rc = L.gm_rollout_errors(None, pred, None, 10, first, steps, 0, C.byref(fd), None, None)
    assert rc == (0 if ok else -1), (rc, L.gm_last_error())
    if not ok:
        assert L.gm_last_error().startswith(b"gm_rollout_errors: ")


def test_rollout_errors_checks_descriptor_batch_and_pointers():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    assert L.gm_rollout_errors(None, None, None, 10, 0, 1, 5, None, None, None) == -1
    assert L.gm_last_error() == b"gm_rollout_errors: null feature descriptor"
    assert L.gm_rollout_errors(None, None, None, 10, 0, 1, 7, C.byref(_fdesc(n_per=3)), None, None) == -1
    assert b"multiple of nodes_per_graph" in L.gm_last_error()
    assert L.gm_rollout_errors(None, None, None, 10, 0, 1, 6, C.byref(_fdesc(n_per=3)), None, None) == -1
    assert L.gm_last_error() == b"gm_rollout_errors: null pointer"


def test_python_surface():
    import gnn_manip_amd
    from gnn_manip_amd.rollout import RolloutEngine, evaluate_rollout
    assert gnn_manip_amd.evaluate_rollout is evaluate_rollout
    assert callable(RolloutEngine.run_recorded)
    with pytest.raises(ValueError, match="graph_attr"):
        evaluate_rollout([], None)
