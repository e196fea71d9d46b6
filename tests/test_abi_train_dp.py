"""CPU: the bindings of the data-parallel entry points (gm_rank_sum, gm_trainer_contribution_bytes, gm_trainer_contribution,
gm_trainer_reduce): declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the
built library -- an addition to ABI 7 -- and refusing null or absurd arguments before any device call, with a message that starts
with their name.  The refusals that need a trainer (a short buffer, no mini-batch begun, ...) are in tests/test_gpu_train_dp.py."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("gm_rank_sum", "gm_trainer_contribution_bytes", "gm_trainer_contribution", "gm_trainer_reduce")
FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL or looked at for its alignment: never read
FAKE2 = C.c_void_p(8192)


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    decl = " ".join(decl.split())
    if "*" in decl:
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


def test_the_header_states_the_layout_and_the_order():
    text = " ".join(open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read().split())
    assert "{ int64 samples, int64 bad, double loss_sum, int64 steps_applied }" in text
    assert "strictly in rank order" in text and "world == 1 copies the bits" in text
    norm = [" ".join(p.split()) for p in _declared("gm_rank_sum")[1].split(",")]
    assert norm == ["const float* src", "int64_t count", "int world", "int64_t stride_floats", "float* dst", "void* stream"]


def test_rank_sum_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    for src, dst in ((None, FAKE2), (FAKE, None), (None, None)):
        assert L.gm_rank_sum(src, 100, 2, 100, dst, None) == -1 and err() == "gm_rank_sum: null pointer"
    for count in (0, -1):
        assert L.gm_rank_sum(FAKE, count, 2, 100, FAKE2, None) == -1 and err() == "gm_rank_sum: count=%d out of range" % count
    for world in (0, -1, 65):
        assert L.gm_rank_sum(FAKE, 100, world, 100, FAKE2, None) == -1 and err() == "gm_rank_sum: world=%d outside 1..64" % world
    for stride in (99, 96, 0, 101, 102, 103):                                 # below the count; no multiple of 4
        assert L.gm_rank_sum(FAKE, 100, 2, stride, FAKE2, None) == -1
        assert err() == "gm_rank_sum: stride_floats=%d below count=100 or no multiple of 4" % stride
    for src, dst in ((C.c_void_p(4100), FAKE2), (FAKE, C.c_void_p(8200)), (C.c_void_p(4104), C.c_void_p(8196))):
        assert L.gm_rank_sum(src, 100, 2, 100, dst, None) == -1 and err() == "gm_rank_sum: src and dst must lie on 16 bytes"


def test_a_null_trainer_is_refused_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    assert L.gm_trainer_contribution_bytes(None) == 0
    for poisoned in (0, 1):
        assert L.gm_trainer_contribution(None, FAKE, 1 << 20, poisoned, None) == -1 and err() == "gm_trainer_contribution: null trainer"
    assert L.gm_trainer_reduce(None, FAKE, 2, 1 << 20, 3, None) == -1 and err() == "gm_trainer_reduce: null trainer"
