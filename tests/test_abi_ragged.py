"""CPU: the bindings of the ragged entry points (gm_graph_ragged_workspace_bytes, gm_radius_graph_build_ragged,
gm_train_batch_ragged_workspace_bytes, gm_train_batch_build_ragged, gm_train_batch_edges_ragged): declared in
include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported by the built library -- an addition to
ABI 7 -- refusing their arguments before any device call, and leaving the existing workspace layouts as they were."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import BOUNDS, ROOT, STATS
import ragged_cases as rc
import train_batch_cases as tc

NEW_SYMBOLS = ("gm_graph_ragged_workspace_bytes", "gm_radius_graph_build_ragged", "gm_train_batch_ragged_workspace_bytes",
               "gm_train_batch_build_ragged", "gm_train_batch_edges_ragged")
INVALID = -1


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the descriptor is typed, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        return _lib._FD if decl.startswith("const gm_feature_desc") else C.c_void_p
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


def test_header_constant():
    h = _header()
    ragged = int(re.search(r"#define\s+GM_RAGGED_MAX_GRAPHS\s+(\d+)\b", h).group(1))
    batch = int(re.search(r"#define\s+GM_TRAIN_BATCH_MAX\s+(\d+)\b", h).group(1))
    assert ragged == batch == rc.GM_RAGGED_MAX_GRAPHS == tc.GM_TRAIN_BATCH_MAX


def _fdesc(control=True, k=6, rec_dim=tc.REC_DIM):
    from gnn_manip_amd.graph import make_feature_desc
    return make_feature_desc(tc.R, STATS, BOUNDS, tc.CART, [tc.MAT], [rec_dim, rec_dim + 1, rec_dim + 2] if control else None, k,
                             rec_dim + (3 if control else 0))


FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read
BIG = 1 << 40


def _i64(values):
    return (C.c_int64 * len(values))(*values)


def _graph(L, offsets=(0, 3, 10), n_graphs=None, pos=FAKE, stride=3, r=0.015, cap=20, ws=FAKE, ws_bytes=BIG):
    off = None if offsets is None else _i64(offsets)
    n_graphs = len(offsets) - 1 if n_graphs is None else n_graphs
    return L.gm_radius_graph_build_ragged(pos, stride, off, n_graphs, r, cap, ws, ws_bytes, None)


def test_graph_build_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    who = "gm_radius_graph_build_ragged: "
    many = list(range(0, 67))
    for n_graphs in (0, 65, -1):
        assert _graph(L, many, n_graphs=n_graphs) == INVALID and err().startswith(who + "n_graphs=%d outside 1..64" % n_graphs)
    assert _graph(L, (1, 3, 10)) == INVALID and err().startswith(who + "graph_offsets[0]=1")
    for off in ((0, 0, 10), (0, 5, 5), (0, 5, 4)):
        assert _graph(L, off) == INVALID and err().startswith(who + "graph ") and "rows (< 1)" in err(), off
    for kw in (dict(offsets=None, n_graphs=2), dict(pos=None), dict(ws=None)):
        assert _graph(L, **kw) == INVALID and err() == who + "null pointer", kw
    assert _graph(L, (0, 5, 1 << 30)) == INVALID and err().startswith(who + "n_nodes=")
    for cap in (0, 161, -4):
        assert _graph(L, cap=cap) == INVALID and err().startswith(who + "max_neighbours=%d" % cap)
    assert _graph(L, (0, 1 << 26, 1 << 27), cap=20) == INVALID and "overflows int32" in err() and err().startswith(who)
    for r in (0.0, -1.0, float("nan")):
        assert _graph(L, r=r) == INVALID and err() == who + "conn_r must be > 0"
    assert _graph(L, stride=2) == INVALID and err() == who + "pos_stride < 3"
    need = L.gm_graph_ragged_workspace_bytes(10, 2, 20)
    assert need > 0 and _graph(L, ws_bytes=need - 1) == INVALID and err() == who + "workspace %d < %d" % (need - 1, need)


def test_graph_workspace_query():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    q = L.gm_graph_ragged_workspace_bytes
    for bad in (q(10, 0, 20), q(10, 65, 20), q(10, -1, 20), q(1, 2, 20), q(0, 1, 20), q(1 << 30, 2, 20), q(10, 2, 0), q(10, 2, 161), q(1 << 27, 2, 20)):
        assert bad == 0
    sizes = [q(n, 7, 20) for n in (7, 562, 1177, 4099, 20000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]       # grows with the total rows
    # how the total is split plays no part (the offsets travel in the kernel arguments); an existing workspace carve serves it
    assert len({q(1177, g, 20) for g in (1, 2, 7, 64)}) == 1
    for (n, cap), want in rc.GRAPH_WS_BYTES.items():
        assert q(n, 1, cap) == want, (n, cap)


def test_existing_queries_return_what_they_returned():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    for (n, cap), want in rc.GRAPH_WS_BYTES.items():
        assert L.gm_graph_workspace_bytes(n, cap) == want, (n, cap)
    fd = _fdesc()
    for (batch, n, cap), want in rc.TRAIN_BATCH_WS_BYTES.items():
        assert L.gm_train_batch_workspace_bytes(C.byref(fd), batch, n, cap) == want, (batch, n, cap)
        assert L.gm_train_batch_ragged_workspace_bytes(C.byref(fd), batch * n, batch, cap) == want       # equal sizes: the same layout


def _build(L, fd, sizes=(10, 7), batch=None, rec_dim=tc.REC_DIM, k_nb=20, frames="fake", nodes=FAKE, target=FAKE, ws=FAKE, ws_bytes=BIG):
    batch = len(sizes) if batch is None else batch
    if frames == "fake":
        frames = (C.c_void_p * max(batch, 1))(*([4096] * max(batch, 1)))
    return L.gm_train_batch_build_ragged(frames, None if sizes is None else _i64(sizes), batch, rec_dim, None if fd is None else C.byref(fd),
                                         k_nb, 0.0, 0, 0, None, nodes, target, None, ws, ws_bytes, None)


def test_batch_build_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    err = lambda: L.gm_last_error().decode()
    who = "gm_train_batch_build_ragged: "
    assert _build(L, None) == INVALID and err() == who + "null feature descriptor"
    for kw in (dict(frames=None), dict(nodes=None), dict(target=None), dict(ws=None), dict(sizes=None, batch=2)):
        assert _build(L, fd, **kw) == INVALID and err() == who + "null pointer", kw
    holes = (C.c_void_p * 2)(4096, None)
    assert _build(L, fd, frames=holes) == INVALID and err() == who + "null pointer (first_frames[1])"
    assert _build(L, _fdesc(k=1)) == INVALID and err() == who + "k_steps=1 out of range"
    for batch in (0, tc.GM_TRAIN_BATCH_MAX + 1, -3):
        assert _build(L, fd, sizes=[5] * 70, batch=batch) == INVALID and err().startswith(who + "batch=%d outside 1..64" % batch)
    for sizes in ((10, 0), (0, 10), (10, -2)):
        assert _build(L, fd, sizes=sizes) == INVALID and err().startswith(who + "sizes[%d]=%d < 1" % (int(sizes[0] >= 1), min(sizes))), sizes
    wrong = _fdesc()
    wrong.control_col = 4
    for bad, rec_dim in ((wrong, 5), (fd, 6), (_fdesc(control=False), 6), (_fdesc(control=False), 4)):
        assert _build(L, bad, rec_dim=rec_dim) == INVALID and err().startswith(who + "data_dim=") and "control_col == rec_dim" in err()
    # the graph builder's limits on the TOTAL of the sizes
    for kw in (dict(k_nb=0), dict(k_nb=161), dict(sizes=(1 << 29, 1 << 29)), dict(sizes=(1 << 26, 1 << 26), k_nb=20)):
        assert _build(L, fd, **kw) == INVALID and err().startswith(who), (kw, err())
    need = L.gm_train_batch_ragged_workspace_bytes(C.byref(fd), 17, 2, 20)
    assert need > 0 and _build(L, fd, ws_bytes=need - 1) == INVALID and err() == who + "workspace %d < %d" % (need - 1, need)
    assert _build(L, _fdesc(k=9)) == -2 and "k_steps=9 unsupported (2..8" in err()


def test_batch_edges_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    err = lambda: L.gm_last_error().decode()
    who = "gm_train_batch_edges_ragged: "
    edges = lambda ws=FAKE, sizes=(10, 7), batch=2, d=fd, cap=20, e=5, ei=FAKE, ea=FAKE: L.gm_train_batch_edges_ragged(
        ws, None if sizes is None else _i64(sizes), batch, None if d is None else C.byref(d), cap, e, ei, ea, None)
    assert edges(d=None) == INVALID and err() == who + "null feature descriptor"
    for kw in (dict(ws=None), dict(sizes=None), dict(ei=None), dict(ea=None)):
        assert edges(**kw) == INVALID and err() == who + "null pointer", kw
    assert edges(batch=0) == INVALID and "batch=0" in err()
    assert edges(sizes=(10, 0)) == INVALID and err().startswith(who + "sizes[1]=0 < 1")
    for e in (-1, 17 * 20 + 1):
        assert edges(e=e) == INVALID and "n_edges=%d" % e in err() and err().startswith(who)
    assert edges(cap=161) == INVALID and err().startswith(who + "max_neighbours=161")
    assert edges(e=0, ei=None, ea=None) == 0                      # no edges: nothing to write


def test_batch_workspace_query():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    fd = _fdesc()
    q = lambda rows, batch=3, k_nb=20, d=fd: L.gm_train_batch_ragged_workspace_bytes(None if d is None else C.byref(d), rows, batch, k_nb)
    for bad in (q(100, 0), q(100, 65), q(100, -1), q(2, 3), q(0, 1), q(100, k_nb=0), q(100, k_nb=161), q(100, d=None), q(1 << 30), q(1 << 27)):
        assert bad == 0
    sizes = [q(rows) for rows in (3, 97, 461, 4099, 20000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert len({q(461, b) for b in (1, 2, 4, 64)}) == 1              # 64 + 97 + 300, however it is split
    assert q(461) >= L.gm_graph_ragged_workspace_bytes(461, 3, 20) + 16 + 461 * 12


def test_python_surface():
    import inspect
    from gnn_manip_amd.graph import RadiusGraph, get_connectivity
    for fn in (RadiusGraph.__init__, get_connectivity):
        sig = inspect.signature(fn).parameters
        assert sig["graph_sizes"].default is None and sig["nodes_per_graph"].default is None
        assert list(sig)[-2:] == ["nodes_per_graph", "graph_sizes"]
    assert np.array_equal(rc.offsets((1, 15, 17)), [0, 1, 16, 33])
