"""CPU: the bindings of the weighted Sinkhorn entry points: declared in include/gnn_manip_hip.h, bound in _lib.py with the
signatures the header states, exported by the built library -- an addition to ABI 7 -- with a workspace query that grows with the
weights it has to hold, and refusing their arguments before any device call."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

NEW_SYMBOLS = ("gm_sinkhorn_weighted_workspace_bytes", "gm_sinkhorn_divergence_weighted", "gm_sinkhorn_divergence_weighted_backward")
CTYPES = {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t, "float": C.c_float}


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    decl = " ".join(decl.split())
    return C.c_void_p if "*" in decl else CTYPES[decl.rsplit(" ", 1)[0]]


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


@pytest.mark.parametrize("batch,n,m", [(1, 1, 1), (1, 17, 63), (6, 150, 130), (64, 4500, 4500)])
def test_workspace_query_is_monotone_in_the_weights(batch, n, m):
    """Without weights it is the unweighted query (the same layout: the backward of either reads either); each side's logarithms add
    at least their own bytes -- b's once when y is shared, per pair otherwise."""
    from gnn_manip_amd import _lib
    L = _lib.lib()
    q = L.gm_sinkhorn_weighted_workspace_bytes
    base = L.gm_sinkhorn_batched_workspace_bytes(batch, n, m)
    for shared in (0, 1):
        assert q(batch, n, m, 0, 0, shared) == base
        assert q(batch, n, m, 1, 0, shared) >= base + 4 * batch * n
        assert q(batch, n, m, 0, 1, shared) >= base + 4 * (m if shared else batch * m)
        assert q(batch, n, m, 1, 1, shared) >= max(q(batch, n, m, 1, 0, shared), q(batch, n, m, 0, 1, shared)) + 4 * min(n, m)
    assert q(batch, n, m, 0, 1, 1) <= q(batch, n, m, 0, 1, 0)
    assert q(-1, n, m, 1, 1, 0) == 0


def test_arguments_are_checked_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fwd = [None if t is C.c_void_p else 0 for t in _lib.PROTOTYPES["gm_sinkhorn_divergence_weighted"][1]]
    assert L.gm_sinkhorn_divergence_weighted(*fwd) == -1
    assert L.gm_last_error() == b"gm_sinkhorn_divergence_weighted: null pointer"
    bwd = [None if t is C.c_void_p else 0 for t in _lib.PROTOTYPES["gm_sinkhorn_divergence_weighted_backward"][1]]
    assert L.gm_sinkhorn_divergence_weighted_backward(*bwd) == -1
    assert L.gm_last_error() == b"gm_sinkhorn_divergence_weighted_backward: null pointer"


def test_python_surface():
    import inspect
    from gnn_manip_amd.losses import SamplesLoss
    from gnn_manip_amd.planner import InterpolatedCMAsolver, TrajectoryCMAsolver, density_target
    assert callable(density_target) and callable(TrajectoryCMAsolver.set_density_target)
    assert InterpolatedCMAsolver.set_density_target is TrajectoryCMAsolver.set_density_target
    assert list(inspect.signature(SamplesLoss.batched).parameters) == ["self", "x", "y", "a", "b"]
    for args in ((), (1,), (1, 2, 3), (1, 2, 3, 4, 5)):
        with pytest.raises(TypeError, match="loss\\(a, x, b, y\\)"):
            SamplesLoss()(*args)
    with pytest.raises(NotImplementedError):
        SamplesLoss(loss="energy")
