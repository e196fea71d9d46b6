"""CPU: the bindings of the ragged rollout entry points (gm_rollout_step_ragged, gm_rollout_ragged, gm_rollout_recorded_ragged,
gm_rollout_errors_ragged, the two ragged training sweeps, gm_rollout_l1_loss_ragged and gm_train_rollout_accumulate_ragged with
their workspace queries): declared in include/gnn_manip_hip.h, bound in _lib.py with the signatures the header states, exported
by the built library -- an addition to ABI 7, whose existing declarations and struct layouts stay as they were -- and refusing a
descriptor of equal-sized graphs or a bad table before any device call."""
import ctypes as C
import inspect
import os
import re

import pytest

from conftest import BOUNDS, ROOT, STATS
import ragged_cases as rc
import ragged_rollout_cases as rrc

FORWARD_SYMBOLS = ("gm_rollout_step_ragged", "gm_rollout_ragged", "gm_rollout_recorded_ragged", "gm_rollout_errors_ragged")
NEW_SYMBOLS = FORWARD_SYMBOLS + ("gm_rollout_step_backward_train_ragged", "gm_rollout_backward_train_ragged",
                                 "gm_rollout_l1_loss_ragged_workspace_bytes", "gm_rollout_l1_loss_ragged",
                                 "gm_train_rollout_ragged_workspace_bytes", "gm_train_rollout_accumulate_ragged")
INVALID = -1
FAKE = C.c_void_p(4096)          # a pointer that is only ever compared with NULL: every call below is refused before it is read
BIG = 1 << 40


def _header():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration: the descriptor is typed, every other pointer is void*."""
    from gnn_manip_amd import _lib
    decl = " ".join(decl.split())
    if "*" in decl:
        return _lib._FD if decl.startswith("const gm_feature_desc") else (_lib._MD if decl.startswith("const gm_model_desc") else C.c_void_p)
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}[decl.rsplit(" ", 1)[0]]


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
    assert res is (C.c_int if ret == "int" else C.c_size_t) and args == want, (name, args, want)
    # the graphs travel as in gm_radius_graph_build_ragged: a host table and its length, in this order, and no renumbering
    names = [" ".join(p.split()).rsplit(" ", 1)[1].lstrip("*") for p in params.split(",")]
    if ret == "int":
        assert names[names.index("graph_offsets_host") + 1] == "n_graphs"
    assert not any(n.startswith("renumber") for n in names)


def test_the_single_scene_declarations_are_untouched():
    from gnn_manip_amd import _lib
    h = _header()
    for name in ("gm_rollout_step", "gm_rollout", "gm_rollout_recorded", "gm_rollout_errors", "gm_rollout_workspace_bytes", "gm_rollout_status"):
        ret, params = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, h).groups()
        assert "graph_offsets_host" not in params
    assert C.sizeof(_lib.FeatureDesc) == 104 and _lib.FeatureDesc.nodes_per_graph.offset == 28     # gm_feature_desc keeps its layout
    assert int(re.search(r"#define\s+GM_RAGGED_MAX_GRAPHS\s+(\d+)\b", h).group(1)) == rc.GM_RAGGED_MAX_GRAPHS == 64


def _fdesc(n_per=0):
    from gnn_manip_amd.graph import make_feature_desc
    L = rrc.L
    d = make_feature_desc(rrc.R, STATS, BOUNDS, L.cart_idx, [L.mat], L.ctrl_idx, L.k, L.D)
    d.nodes_per_graph = n_per
    return d


def _i64(values):
    return (C.c_int64 * len(values))(*values)


def _calls(L, offsets, fd, n_graphs=None, ws=FAKE):
    """name -> status of every new entry point on this table and descriptor (fake pointers elsewhere)."""
    off = None if offsets is None else _i64(offsets)
    g = (len(offsets) - 1) if n_graphs is None else n_graphs
    d = None if fd is None else C.byref(fd)
    out = {}
    out["gm_rollout_step_ragged"] = L.gm_rollout_step_ragged(FAKE, FAKE, off, g, d, 20, FAKE, None, None, ws, BIG, None)
    msg = {"gm_rollout_step_ragged": L.gm_last_error().decode()}
    out["gm_rollout_ragged"] = L.gm_rollout_ragged(FAKE, FAKE, off, g, d, 20, FAKE, None, 0, 0, 1, None, ws, BIG, None)
    msg["gm_rollout_ragged"] = L.gm_last_error().decode()
    out["gm_rollout_recorded_ragged"] = L.gm_rollout_recorded_ragged(FAKE, FAKE, off, g, d, 20, FAKE, FAKE, 1, None, None, ws, BIG, None)
    msg["gm_rollout_recorded_ragged"] = L.gm_last_error().decode()
    out["gm_rollout_errors_ragged"] = L.gm_rollout_errors_ragged(FAKE, None, FAKE, 9, 0, 1, off, g, d, ws, None)
    msg["gm_rollout_errors_ragged"] = L.gm_last_error().decode()
    return out, msg


def test_refusals_before_any_device_call():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    good = [0, 3, 10]
    cases = [(good, _fdesc(3), None, FAKE, "nodes_per_graph=3, must be 0"),
             ([1, 3, 10], _fdesc(), None, FAKE, "graph_offsets[0]=1"),
             ([0, 3, 3, 10], _fdesc(), None, FAKE, "graph 1 has 0 rows (< 1)"),
             (list(range(67)), _fdesc(), 65, FAKE, "n_graphs=65 outside 1..64"),
             (list(range(67)), _fdesc(), 0, FAKE, "n_graphs=0 outside 1..64"),
             (None, _fdesc(), 2, FAKE, "null pointer"),
             (good, _fdesc(), None, None, "null pointer"),
             ([0, 5, 1 << 30], _fdesc(), None, FAKE, "n_nodes=")]
    for offsets, fd, n_graphs, ws, text in cases:
        status, msg = _calls(L, offsets, fd, n_graphs, ws)
        for name in FORWARD_SYMBOLS:
            assert status[name] == INVALID and msg[name].startswith(name + ": ") and text in msg[name], (name, text, status[name], msg[name])
    # the error sums' own frame range, with a good table
    for first, steps in ((9, 1), (-1, 1), (0, 10)):
        rc_ = L.gm_rollout_errors_ragged(FAKE, None, FAKE, 9, first, steps, _i64(good), 2, C.byref(_fdesc()), FAKE, None)
        assert rc_ == INVALID and L.gm_last_error().decode().startswith("gm_rollout_errors_ragged: frames ["), (first, steps)
    assert L.gm_rollout_errors_ragged(FAKE, None, FAKE, 9, 0, 0, _i64(good), 2, C.byref(_fdesc()), FAKE, None) == 0     # no step: nothing to do


def test_workspace_query_is_the_single_scene_one():
    """The table adds nothing to the workspace: a ragged batch of N rows takes gm_rollout_workspace_bytes(desc, N, K)."""
    from gnn_manip_amd import _lib
    L = _lib.lib()
    assert not any(name.endswith("workspace_bytes") for name in FORWARD_SYMBOLS)
    dims, _, _, _ = rrc.model("h64")
    md = _lib.ModelDesc(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], 1e-5, 0, 0, 0, 0, 0)
    sizes = [L.gm_rollout_workspace_bytes(C.byref(md), n, 20) for n in (1, 353, 653)]
    assert 0 < sizes[0] <= sizes[1] <= sizes[2]


def test_training_entry_points_refuse_before_any_device_call_and_size_their_workspaces():
    from gnn_manip_amd import _lib
    L = _lib.lib()
    err = lambda: L.gm_last_error().decode()
    good, frames = _i64([0, 3, 10]), (C.c_void_p * 2)(4096, 4096)
    for fd, off, g, text in ((_fdesc(3), good, 2, "nodes_per_graph=3, must be 0"), (_fdesc(), _i64([1, 3, 10]), 2, "graph_offsets[0]=1"),
                             (_fdesc(), _i64([0, 3, 3, 10]), 3, "graph 1 has 0 rows (< 1)"), (_fdesc(), _i64(list(range(67))), 65, "n_graphs=65")):
        d = C.byref(fd)
        rc_ = L.gm_rollout_step_backward_train_ragged(FAKE, FAKE, 1, FAKE, off, g, d, 20, None, None, FAKE, None, None, FAKE, None, None, FAKE, BIG, None)
        assert rc_ == INVALID and err().startswith("gm_rollout_step_backward_train_ragged: ") and text in err(), err()
        rc_ = L.gm_rollout_backward_train_ragged(FAKE, FAKE, 1, FAKE, off, g, d, 20, None, None, 0, 0, 1, FAKE, None, None, FAKE, None, FAKE, BIG, None)
        assert rc_ == INVALID and err().startswith("gm_rollout_backward_train_ragged: ") and text in err(), err()
        rc_ = L.gm_rollout_l1_loss_ragged(FAKE, FAKE, frames, rrc.L.D, 1, off, g, d, None, -1, None, FAKE, None, None, None, FAKE, BIG, None)
        assert rc_ == INVALID and err().startswith("gm_rollout_l1_loss_ragged: ") and text in err(), err()
    d = C.byref(_fdesc())
    holes = (C.c_void_p * 2)(4096, None)
    assert L.gm_rollout_l1_loss_ragged(FAKE, FAKE, holes, rrc.L.D, 1, good, 2, d, None, -1, None, FAKE, None, None, None, FAKE, BIG, None) == INVALID
    assert err() == "gm_rollout_l1_loss_ragged: null pointer (frames[1])"
    assert L.gm_rollout_l1_loss_ragged(FAKE, FAKE, frames, rrc.L.D - 1, 1, good, 2, d, None, -1, None, FAKE, None, None, None, FAKE, BIG, None) == INVALID
    assert "frame_dim=" in err()
    need = L.gm_rollout_l1_loss_ragged_workspace_bytes(2)
    assert need > 0 and [L.gm_rollout_l1_loss_ragged_workspace_bytes(g) for g in (0, 65, -1)] == [0, 0, 0]
    assert L.gm_rollout_l1_loss_ragged_workspace_bytes(64) > need
    assert L.gm_rollout_l1_loss_ragged(FAKE, FAKE, frames, rrc.L.D, 1, good, 2, d, None, -1, None, FAKE, None, None, None, FAKE, need - 1, None) == -4
    assert L.gm_train_rollout_accumulate_ragged(None, FAKE, good, 2, d, 20, None, 0, frames, rrc.L.D, 1, -1, None, 1, FAKE, FAKE, BIG, None) == INVALID
    assert err() == "gm_train_rollout_accumulate_ragged: null trainer"
    dims, _, _, _ = rrc.model("h64")
    md = _lib.ModelDesc(dims[0], dims[1], dims[2], dims[3], dims[4], dims[5], 1e-5, 0, 0, 0, 0, 0)
    q = lambda n, nr, g, steps=2: L.gm_train_rollout_ragged_workspace_bytes(C.byref(md), d, n, nr, g, 20, steps)
    assert [q(10, 1, 0), q(10, 1, 65), q(1, 0, 2), q(10, 11, 2), q(10, 1, 2, 0)] == [0] * 5
    one = L.gm_train_rollout_step_workspace_bytes(C.byref(md), d, 353, 30, 20, 2)
    # the plain step is the batch of one graph (one set of loss kernels); the table adds the per-graph partials only
    assert 0 < one == q(353, 30, 1) < q(353, 30, 3) and q(353, 30, 3) - one < 1 << 20


def test_python_surface():
    from gnn_manip_amd import RolloutEngine, evaluate_rollout
    sig = inspect.signature(RolloutEngine.__init__).parameters
    assert list(sig)[:4] == ["self", "model", "graph_attr", "n_nodes"] and sig["n_nodes"].default is None     # positional n_nodes still works
    assert list(sig)[-1] == "sizes" and sig["sizes"].default is None
    assert sig["candidates"].default == 1 and sig["renumber"].default == "auto"
    ev = inspect.signature(evaluate_rollout).parameters
    assert list(ev)[-1] == "ragged" and ev["ragged"].default is False
    assert hasattr(RolloutEngine, "rows") and isinstance(RolloutEngine.ragged, property)
