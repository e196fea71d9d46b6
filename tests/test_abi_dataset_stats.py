"""CPU: the bindings of the dataset entry points (gm_recording_stats_workspace_bytes, gm_recording_stats,
gm_neighbour_census_workspace_bytes, gm_neighbour_census): declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures
the header states, exported by the built library -- an addition to ABI 7 -- and refusing their arguments before any device call."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT
import dataset_stats_cases as dc
import ragged_cases as rc

NEW_SYMBOLS = ("gm_recording_stats_workspace_bytes", "gm_recording_stats", "gm_neighbour_census_workspace_bytes", "gm_neighbour_census")
INVALID = -1
FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read
BIG = 1 << 40


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    decl = " ".join(decl.split())
    if "*" in decl:
        return C.c_void_p
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t, "double": C.c_double, "float": C.c_float}[decl.rsplit(" ", 1)[0]]


def test_declared_entry_points_are_the_exported_ones():
    """Every gm_ function the header declares is bound and exported, and the library exports no gm_ symbol the header lacks."""
    import subprocess
    from gnn_manip_amd import _lib
    declared = set(re.findall(r"\b(gm_[a-z0-9_]+)\s*\(", _header()))
    assert set(NEW_SYMBOLS) <= declared
    assert declared == set(_lib.PROTOTYPES)
    L = _lib.lib()
    assert all(hasattr(L, name) for name in declared)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.split() and line.split()[-1].startswith("gm_")}
    assert exported == declared, (sorted(exported - declared), sorted(declared - exported))
    assert L.gm_abi_version() == 7


@pytest.mark.parametrize("name", NEW_SYMBOLS)
def test_binding_has_the_headers_signature(name):
    from gnn_manip_amd import _lib
    ret, params = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, _header()).groups()
    res, args = _lib.PROTOTYPES[name]
    assert res is (C.c_int if ret == "int" else C.c_size_t)
    assert args == [_ctype(p) for p in params.split(",")], (name, args)


def _stats(L, rec=FAKE, t=5, n=10, d=8, cart0=2, dim=3, mcol=-1, mval=0.0, out=FAKE, ws=FAKE, ws_bytes=BIG):
    return L.gm_recording_stats(rec, t, n, d, cart0, dim, mcol, mval, out, ws, ws_bytes, None)


def test_recording_stats_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    who = "gm_recording_stats: "
    for kw in (dict(rec=None), dict(out=None), dict(ws=None)):
        assert _stats(L, **kw) == INVALID and err() == who + "null pointer", kw
    for t in (2, 1, 0, -7):
        assert _stats(L, t=t) == INVALID and err().startswith(who + "n_frames=%d < 3" % t)
    for n in (0, -1):
        assert _stats(L, n=n) == INVALID and err().startswith(who + "n_nodes=%d < 1" % n)
    for dim in (0, 4, -1):
        assert _stats(L, dim=dim) == INVALID and err() == who + "dim=%d outside 1..3" % dim
    for cart0, dim in ((-1, 3), (6, 3), (8, 1), (7, 2)):
        assert _stats(L, cart0=cart0, dim=dim) == INVALID and err().startswith(who + "columns cart0=%d" % cart0), (cart0, dim)
    assert _stats(L, cart0=5, dim=3, ws_bytes=0) == INVALID and "workspace" in err()          # the last admissible column passes the column check
    for mcol in (8, 9):
        assert _stats(L, mcol=mcol) == INVALID and err().startswith(who + "material_col=%d" % mcol)
    need = L.gm_recording_stats_workspace_bytes(5, 10)
    assert need > 0 and _stats(L, ws_bytes=need - 1) == INVALID and err() == who + "workspace %d < %d" % (need - 1, need)


def test_recording_stats_workspace_query():
    from gnn_manip_amd import _lib
    q = _lib.lib().gm_recording_stats_workspace_bytes
    for bad in (q(2, 10), q(0, 10), q(-1, 10), q(3, 0), q(3, -5), q(1 << 40, 1 << 40)):
        assert bad == 0
    rec = dc.RECORD_DOUBLES * 8
    # one record per workgroup behind the shifts: a workgroup per THREADS nodes up to MAX_WORKGROUPS, the same from there on
    assert q(3, 1) == q(9, dc.THREADS) == 256 + rec and q(3, dc.THREADS + 1) == 256 + 2 * rec
    assert q(3, dc.ONE_PASS) - q(3, dc.ONE_PASS - dc.THREADS) == rec
    assert q(3, dc.ONE_PASS) == q(3, dc.N_PAST_ONE_PASS) == q(400, 10 ** 7) == 256 + dc.MAX_WORKGROUPS * rec


def _census(L, pos=FAKE, stride=8, n=100, r=0.015, counts=FAKE, ws=FAKE, ws_bytes=BIG):
    return L.gm_neighbour_census(pos, stride, n, r, counts, ws, ws_bytes, None)


def test_neighbour_census_refuses_its_arguments_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    who = "gm_neighbour_census: "
    for kw in (dict(pos=None), dict(counts=None), dict(ws=None)):
        assert _census(L, **kw) == INVALID and err() == who + "null pointer", kw
    for n in (0, -3, 1 << 30):
        assert _census(L, n=n) == INVALID and err().startswith(who + "n_nodes=%d out of range" % n)
    for r in (0.0, -1.0, float("nan")):
        assert _census(L, r=r) == INVALID and err() == who + "conn_r must be > 0"
    assert _census(L, stride=2) == INVALID and err() == who + "pos_stride < 3"
    need = L.gm_neighbour_census_workspace_bytes(100)
    assert need > 0 and _census(L, ws_bytes=need - 1) == INVALID and err() == who + "workspace %d < %d" % (need - 1, need)


def test_neighbour_census_workspace_query():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    q = L.gm_neighbour_census_workspace_bytes
    assert q(0) == q(-1) == q(1 << 30) == 0
    sizes = [q(n) for n in (1, 562, 4099, 20000, 100000)]
    assert sizes[0] > 0 and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(q(n) == L.gm_graph_workspace_bytes(n, 1) for n in (1, 17, 1000, 100000))      # the build's own carve at the smallest cap
    for (n, cap), want in rc.GRAPH_WS_BYTES.items():                                          # ... which stays what it was
        assert L.gm_graph_workspace_bytes(n, cap) == want, (n, cap)


def test_python_surface():
    import inspect
    import gnn_manip_amd as g
    sig = inspect.signature(g.recording_statistics).parameters
    assert list(sig) == ["sims", "cartesian_idx", "material_id", "material"] and sig["cartesian_idx"].default == (2, 3, 4)
    assert sig["material_id"].default is None and sig["material"].default is None
    assert list(inspect.signature(g.write_metadata).parameters) == ["path", "sims", "bounds", "cartesian_idx", "control_idx", "material_id"]
    sig = inspect.signature(g.neighbour_census).parameters
    assert list(sig) == ["sims", "conn_r", "max_neighbours", "cartesian_idx", "frames"]
    assert sig["max_neighbours"].default == 20 and sig["frames"].default is None
    assert "stats" in inspect.signature(g.CoffeeDataset.from_recordings).parameters
    with pytest.raises(RuntimeError, match="recording_statistics: float32"):
        g.recording_statistics([])
