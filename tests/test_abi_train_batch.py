"""CPU: the bindings of the training-batch entry points (gm_train_batch_workspace_bytes / _build / _edges / _num_edges /
_status): declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the built
library -- an addition to ABI 7 -- and refusing their arguments before any device call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import BOUNDS, ROOT, STATS
import train_batch_cases as tc

NEW_SYMBOLS = ("gm_train_batch_workspace_bytes", "gm_train_batch_build", "gm_train_batch_edges", "gm_train_batch_num_edges",
               "gm_train_batch_status")


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the descriptor is typed, an int64_t* that returns a host count
    is a typed pointer, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        if decl.startswith("const gm_feature_desc"):
            return _lib._FD
        if decl == "int64_t* n_edges_host":
            return C.POINTER(C.c_int64)
        return C.c_void_p
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t, "double": C.c_double, "uint64_t": C.c_uint64}[decl.rsplit(" ", 1)[0]]


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


def test_header_constant_is_the_cases():
    assert re.search(r"#define\s+GM_TRAIN_BATCH_MAX\s+%d\b" % tc.GM_TRAIN_BATCH_MAX, _header())


def _fdesc(control=True, k=6, rec_dim=tc.REC_DIM):
    from gnn_manip_amd.graph import make_feature_desc
    return make_feature_desc(tc.R, STATS, BOUNDS, tc.CART, [tc.MAT], [rec_dim, rec_dim + 1, rec_dim + 2] if control else None, k,
                             rec_dim + (3 if control else 0))


FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read


def _build(L, fd, batch=2, n=10, rec_dim=tc.REC_DIM, k_nb=20, frames="fake", nodes=FAKE, target=FAKE, ws=FAKE, ws_bytes=None):
    if frames == "fake":
        frames = (C.c_void_p * max(batch, 1))(*([4096] * max(batch, 1)))
    if ws_bytes is None:
        ws_bytes = L.gm_train_batch_workspace_bytes(C.byref(fd), batch, n, k_nb) if fd is not None else 0
    return L.gm_train_batch_build(frames, batch, n, rec_dim, None if fd is None else C.byref(fd), k_nb, 0.0, 0, 0, None, nodes, target, None,
                                  ws, ws_bytes, None)


def test_build_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    err = lambda: L.gm_last_error().decode()
    assert _build(L, None) == -1 and err() == "gm_train_batch_build: null feature descriptor"
    for kw in (dict(frames=None), dict(nodes=None), dict(target=None), dict(ws=None, ws_bytes=1 << 30)):
        assert _build(L, fd, **kw) == -1 and err() == "gm_train_batch_build: null pointer", kw
    holes = (C.c_void_p * 2)(4096, None)
    assert _build(L, fd, frames=holes) == -1 and err() == "gm_train_batch_build: null pointer (first_frames[1])"
    assert _build(L, _fdesc(k=1)) == -1 and err() == "gm_train_batch_build: k_steps=1 out of range"
    for batch in (0, tc.GM_TRAIN_BATCH_MAX + 1, -3):
        assert _build(L, fd, batch=batch, ws_bytes=1 << 30) == -1 and err().startswith("gm_train_batch_build: batch=%d outside 1..64" % batch)
    assert _build(L, fd, n=0, ws_bytes=1 << 30) == -1 and err().startswith("gm_train_batch_build: nodes_per_graph=0")
    # the window is the recording's columns, or those and three control columns AT rec_dim
    wrong = _fdesc()
    wrong.control_col = 4
    for bad, rec_dim in ((wrong, 5), (fd, 6), (_fdesc(control=False), 6), (_fdesc(control=False), 4)):
        assert _build(L, bad, rec_dim=rec_dim, ws_bytes=1 << 30) == -1, (bad.control_col, bad.data_dim, rec_dim)
        assert err().startswith("gm_train_batch_build: data_dim=") and "control_col == rec_dim" in err()
    # the graph builder's limits, as this call's refusal
    for kw in (dict(k_nb=0), dict(k_nb=161), dict(n=1 << 29, batch=2), dict(n=1 << 27, k_nb=20)):
        assert _build(L, fd, ws_bytes=1 << 40, **kw) == -1 and err().startswith("gm_train_batch_build: gm_radius_graph_build"), (kw, err())
    need = L.gm_train_batch_workspace_bytes(C.byref(fd), 2, 10, 20)
    assert _build(L, fd, ws_bytes=need - 1) == -1 and err() == "gm_train_batch_build: workspace %d < %d" % (need - 1, need)
    # beyond the register-resident window: unsupported, not invalid
    assert _build(L, _fdesc(k=9), ws_bytes=1 << 30) == -2 and "k_steps=9 unsupported (2..8" in err()


def test_edges_and_status_refuse_their_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    err = lambda: L.gm_last_error().decode()
    assert L.gm_train_batch_edges(FAKE, 2, 10, None, 20, 5, FAKE, FAKE, None) == -1 and err() == "gm_train_batch_edges: null feature descriptor"
    assert L.gm_train_batch_edges(None, 2, 10, C.byref(fd), 20, 5, FAKE, FAKE, None) == -1 and err() == "gm_train_batch_edges: null pointer"
    assert L.gm_train_batch_edges(FAKE, 2, 10, C.byref(fd), 20, 5, None, FAKE, None) == -1 and err() == "gm_train_batch_edges: null pointer"
    assert L.gm_train_batch_edges(FAKE, 0, 10, C.byref(fd), 20, 5, FAKE, FAKE, None) == -1 and "batch=0" in err()
    for e in (-1, 2 * 10 * 20 + 1):
        assert L.gm_train_batch_edges(FAKE, 2, 10, C.byref(fd), 20, e, FAKE, FAKE, None) == -1 and "n_edges=%d" % e in err()
    assert L.gm_train_batch_edges(FAKE, 2, 10, C.byref(fd), 20, 0, None, None, None) == 0          # no edges: nothing to write
    e = C.c_int64(-1)
    assert L.gm_train_batch_num_edges(None, C.byref(e), None) == -1 and err() == "gm_train_batch_num_edges: null pointer"
    assert L.gm_train_batch_status(None, C.byref(e)) == -1 and err() == "gm_train_batch_status: null pointer"
    rec = np.array([123, 0, 0, 0], np.int32)
    assert L.gm_train_batch_status(rec.ctypes.data_as(C.c_void_p), C.byref(e)) == 0 and e.value == 123
    rec[1] = 1                                                   # the non-finite flag
    assert L.gm_train_batch_status(rec.ctypes.data_as(C.c_void_p), C.byref(e)) == -5 and "non-finite position" in err()
    assert L.gm_train_batch_status(rec.ctypes.data_as(C.c_void_p), None) == -5


def test_workspace_query():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    q = lambda batch, n=97, k_nb=20, d=fd: L.gm_train_batch_workspace_bytes(None if d is None else C.byref(d), batch, n, k_nb)
    sizes = [q(b) for b in range(1, tc.GM_TRAIN_BATCH_MAX + 1)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert q(2) >= L.gm_graph_workspace_bytes(2 * 97, 20) + 16 + 2 * 97 * 12
    for bad in (q(0), q(65), q(-1), q(2, n=0), q(2, k_nb=0), q(2, k_nb=161), q(2, d=None), q(2, n=1 << 29), q(2, n=1 << 27)):
        assert bad == 0


def test_python_surface():
    import inspect
    import gnn_manip_amd
    from gnn_manip_amd.dataset import CoffeeDataset, GraphLoader
    assert gnn_manip_amd.GraphLoader is GraphLoader and gnn_manip_amd.CoffeeDataset is CoffeeDataset
    sig = inspect.signature(GraphLoader.__init__).parameters
    assert (sig["fused"].default, sig["prefetch"].default, sig["batch_size"].default, sig["shuffle"].default, sig["seed"].default) \
        == (False, 1, 2, False, None)
    sig = inspect.signature(CoffeeDataset.batch).parameters
    assert list(sig) == ["self", "indices", "seed", "first_stream"] and (sig["seed"].default, sig["first_stream"].default) == (0, 0)
    assert "generator" in GraphLoader.__doc__
    with pytest.raises(ValueError, match="prefetch"):
        GraphLoader([], fused=True, prefetch=2)
