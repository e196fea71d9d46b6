"""CPU: the bindings of the mini-batch entry points (gm_trainer_begin, gm_train_step_accumulate, gm_train_rollout_accumulate,
gm_trainer_apply, gm_trainer_accum_record, gm_grad_sumsq and its workspace query): declared in include/gnn_manip_hip.h, bound in
_lib.py with the signatures the header states, exported by the built library -- an addition to ABI 7 -- and refusing null or absurd
arguments before any device call, with a message that starts with their name."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
import train_accum_cases as ac

NEW_SYMBOLS = ("gm_trainer_begin", "gm_train_step_accumulate", "gm_train_rollout_accumulate", "gm_trainer_apply", "gm_trainer_accum_record",
               "gm_grad_sumsq_workspace_bytes", "gm_grad_sumsq")
FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the two descriptors are typed, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        if decl.startswith("const gm_model_desc"):
            return _lib._MD
        if decl.startswith("const gm_feature_desc"):
            return _lib._FD
        return C.c_void_p
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}[decl.rsplit(" ", 1)[0]]


def _declared(name):
    return re.search(r"\b(int|size_t|void)\s+%s\s*\(([^)]*)\)\s*;" % name, _header()).groups()


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
    ret, params = _declared(name)
    want = [_ctype(p) for p in params.split(",")]
    res, args = _lib.PROTOTYPES[name]
    assert res is {"int": C.c_int, "size_t": C.c_size_t, "void": None}[ret]
    assert args == want, (name, args, want)


def test_accumulate_calls_take_their_parents_arguments():
    """gm_train_step's without lr; gm_train_rollout_step's without lr and update -- names and types, in order."""
    norm = lambda params: [" ".join(p.split()) for p in params.split(",")]
    step, acc = norm(_declared("gm_train_step")[1]), norm(_declared("gm_train_step_accumulate")[1])
    assert acc == [p for p in step if p != "double lr"] and len(acc) == len(step) - 1
    step, acc = norm(_declared("gm_train_rollout_step")[1]), norm(_declared("gm_train_rollout_accumulate")[1])
    assert acc == [p for p in step if p not in ("double lr", "int update")] and len(acc) == len(step) - 2
    # the records: the trainer's stays at 32 bytes, the mini-batch's has 48
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    assert "record_host /* 32 bytes */" in text and "record_host /* 48 bytes */" in text


def test_null_trainer_and_null_pointers_are_refused_before_any_device_call():
    from gnn_manip_amd import _lib
    from gnn_manip_amd.graph import make_feature_desc
    from conftest import BOUNDS, CART, CTRL, MAT, STATS
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    assert L.gm_trainer_begin(None, None) == -1 and err() == "gm_trainer_begin: null trainer"
    assert L.gm_trainer_apply(None, 1e-3, 0.0, None, None, None) == -1 and err() == "gm_trainer_apply: null trainer"
    assert L.gm_trainer_accum_record(None, FAKE, None) == -1 and err() == "gm_trainer_accum_record: null trainer"
    assert L.gm_train_step_accumulate(None, FAKE, 10, FAKE, FAKE, 20, FAKE, -1, None, FAKE, 1 << 40, None) == -1
    assert err() == "gm_train_step_accumulate: null trainer"
    fd = make_feature_desc(0.015, STATS, BOUNDS, CART, MAT, CTRL, 6, 8)
    assert L.gm_train_rollout_accumulate(None, FAKE, 400, C.byref(fd), 20, FAKE, 40, FAKE, 8, 3, -1, None, None, FAKE, 1 << 40, None) == -1
    assert err() == "gm_train_rollout_accumulate: null trainer"


def test_grad_sumsq_refuses_its_arguments_and_sizes_its_workspace():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    need = L.gm_grad_sumsq_workspace_bytes(1000)
    assert need == 8 * ac.SUMSQ_GRID_MAX == L.gm_grad_sumsq_workspace_bytes(1) == L.gm_grad_sumsq_workspace_bytes(1 << 33)
    for count in (0, -1):
        assert L.gm_grad_sumsq_workspace_bytes(count) == 0
        assert L.gm_grad_sumsq(FAKE, count, FAKE, FAKE, need, None) == -1 and err() == "gm_grad_sumsq: count=%d out of range" % count
    for kw in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert L.gm_grad_sumsq(kw[0], 1000, kw[1], kw[2], need, None) == -1 and err() == "gm_grad_sumsq: null pointer"
    assert L.gm_grad_sumsq(C.c_void_p(4100), 1000, FAKE, FAKE, need, None) == -1 and err() == "gm_grad_sumsq: x must lie on 16 bytes, ws on 8"
    assert L.gm_grad_sumsq(FAKE, 1000, FAKE, FAKE, need - 1, None) == -4 and err() == "gm_grad_sumsq: workspace %d < %d" % (need - 1, need)
