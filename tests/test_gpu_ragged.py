"""GPU: the ragged builds (cases: ragged_cases.py; their CPU side: test_ragged_cases.py, test_abi_ragged.py).

gm_radius_graph_build_ragged is held, bit for bit, to gm_radius_graph_build on each graph alone plus the graph's row offset;
gm_train_batch_build_ragged / gm_train_batch_edges_ragged to the collate of single-sample gm_train_batch_build / _edges builds on
streams first_stream + b; the loader to collate_graphs over single-sample batches.  Everything but the downstream forward is an
integer or a bit pattern and is compared for equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import BOUNDS, STATS
from gpu_support import dev, to_dev
import ragged_cases as rc
import train_batch_cases as tc
import yardstick

pytestmark = pytest.mark.gpu


def assert_same_bits(got, want, what=""):
    g, w = (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a) for a in (got, want))
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if g.dtype == np.float32:
        g, w = np.ascontiguousarray(g).view(np.uint32), np.ascontiguousarray(w).view(np.uint32)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


# ================================================================== the graph
_WANT = {}


def _per_graph_edges(c, pos_t):
    """get_connectivity on each graph's rows plus the graph's offset, once per case: [2, E] int64 on the host."""
    from gnn_manip_amd import get_connectivity
    if c.name not in _WANT:
        parts = []
        for o, n in zip(rc.offsets(c.sizes)[:-1], c.sizes):
            s, r = get_connectivity(pos_t[o:o + n], c.r, c.cap)
            parts.append(torch.stack((s, r)) + int(o))
        _WANT[c.name] = torch.cat(parts, dim=1).cpu().numpy()
        _WANT[c.name].setflags(write=False)
    return _WANT[c.name]


def _build_in(ws, pos_t, sizes, r, cap, dev):
    """The ragged build and its edge list through ctypes, in the caller's workspace."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    n = int(pos_t.shape[0])
    off = (C.c_int64 * (len(sizes) + 1))(*rc.offsets(sizes).tolist())
    assert 0 < L.gm_graph_ragged_workspace_bytes(n, len(sizes), cap) <= ws.numel()
    check(L.gm_radius_graph_build_ragged(ptr(pos_t), 3, off, len(sizes), r, cap, ptr(ws), ws.numel(), current_stream(dev)))
    e = C.c_int64(-1)
    check(L.gm_radius_graph_num_edges(ptr(ws), C.byref(e), current_stream(dev)))
    ei = torch.full((2, e.value), -7, dtype=torch.int64, device=dev)
    check(L.gm_radius_graph_edges(ptr(ws), n, cap, ptr(ei[0]), ptr(ei[1]), e.value, current_stream(dev)))
    return ei.cpu().numpy()


@pytest.mark.parametrize("name", list(rc.GRAPHS))
def test_ragged_graph_is_the_graphs_one_by_one(dev, name):
    from gnn_manip_amd import get_connectivity
    c = rc.graph_case(name)
    c.check()
    pos_t = to_dev(c.pos, dev)
    want = _per_graph_edges(c, pos_t)
    graph = rc.graph_of_rows(c.sizes)
    assert (graph[want[0]] == graph[want[1]]).all() and want.shape[1] > 0
    s, r = get_connectivity(pos_t, c.r, c.cap, graph_sizes=c.sizes)
    assert s.dtype == torch.int64 and r.dtype == torch.int64
    np.testing.assert_array_equal(torch.stack((s, r)).cpu().numpy(), want)
    # the xyz columns of an [N, 8] state
    state = torch.full((c.pos.shape[0], 8), float("nan"), device=dev)
    state[:, 2:5] = pos_t
    s, r = get_connectivity(state[:, 2:5], c.r, c.cap, graph_sizes=list(c.sizes))
    np.testing.assert_array_equal(torch.stack((s, r)).cpu().numpy(), want)
    if name == "equal":
        s, r = get_connectivity(pos_t, c.r, c.cap, nodes_per_graph=c.sizes[0])
        np.testing.assert_array_equal(torch.stack((s, r)).cpu().numpy(), want)
    if name == "copies":
        one = want[:, want[0] < 97]
        for g in (1, 2):
            np.testing.assert_array_equal(want[:, (want[0] >= 97 * g) & (want[0] < 97 * (g + 1))], one + 97 * g)


@pytest.mark.parametrize("name", list(rc.GRAPHS))
def test_ragged_graph_does_not_depend_on_what_the_workspace_held(dev, name):
    from gnn_manip_amd._lib import lib
    c = rc.graph_case(name)
    other = rc.graph_case("copies" if name != "copies" else "full_table")
    pos_t, other_t = to_dev(c.pos, dev), to_dev(other.pos, dev)
    want = _per_graph_edges(c, pos_t)
    need = max(lib().gm_graph_ragged_workspace_bytes(x.pos.shape[0], len(x.sizes), x.cap) for x in (c, other))
    ws = torch.full((need,), 0xff, dtype=torch.uint8, device=dev)
    np.testing.assert_array_equal(_build_in(ws, pos_t, c.sizes, c.r, c.cap, dev), want)
    np.testing.assert_array_equal(_build_in(ws, other_t, other.sizes, other.r, other.cap, dev), _per_graph_edges(other, other_t))
    np.testing.assert_array_equal(_build_in(ws, pos_t, c.sizes, c.r, c.cap, dev), want)      # again, behind a build of another shape


def test_python_refusals(dev):
    from gnn_manip_amd import get_connectivity
    from gnn_manip_amd._lib import GMError
    from gnn_manip_amd.graph import RadiusGraph
    c = rc.graph_case("full_table")
    pos_t = to_dev(c.pos, dev)
    with pytest.raises(ValueError, match="exclude"):
        get_connectivity(pos_t, c.r, c.cap, nodes_per_graph=4, graph_sizes=c.sizes)
    with pytest.raises(ValueError, match="add up"):
        RadiusGraph(pos_t, c.r, c.cap, graph_sizes=c.sizes[:-1])
    more = torch.cat((pos_t, pos_t[:1]))
    with pytest.raises(GMError, match="gm_radius_graph_build_ragged: n_graphs=65"):                # a 65th graph
        get_connectivity(more, c.r, c.cap, graph_sizes=c.sizes + (1,))
    with pytest.raises(GMError, match="gm_radius_graph_build_ragged: graph 1 has 0 rows"):
        get_connectivity(pos_t[:10], c.r, c.cap, graph_sizes=(4, 0, 6))


# ================================================================== downstream of a ragged workspace
def _csr_arrays(raw, n, cap):
    """in_ptr, dst, src, eid of a csr workspace (carve_csr: 256-byte aligned arrays behind a 16-byte header)."""
    ints = raw[:raw.shape[0] // 4 * 4].view(np.int32)
    off, out = 16, {}
    for key, count in (("in_ptr", n + 1), ("cursor", n + 1), ("dst", cap), ("src", cap), ("eid", cap)):
        o = (off + 255) // 256 * 256
        off = o + 4 * count
        out[key] = ints[o // 4:o // 4 + count]
    return out


def test_destination_sort_and_forward_on_a_ragged_workspace(dev):
    """gm_csr_from_graph on the ragged workspace lays out ONE graph of n rows -- what the collated edge_index gets from
    gm_csr_from_edge_index -- so gm_edge_features_csr and gm_epd_forward on it agree with EncProcDecGNN.forward on the emitted
    edge_index: within 2e-4 of the output's maximum (yardstick.GRAD_TOL, the float32 bar), and bit for bit where the ragged sort's
    order is the stable sort by receiver that the edge_index path produces."""
    from gnn_manip_amd import EncProcDecGNN, get_edges_displacement
    from gnn_manip_amd._lib import ModelDesc, check, current_stream, lib, ptr
    from gnn_manip_amd.graph import RadiusGraph
    c = rc.graph_case("edges_of_blocks")
    L, n, cap = lib(), c.pos.shape[0], c.pos.shape[0] * c.cap
    pos_t = to_dev(c.pos, dev)
    rg = RadiusGraph(pos_t, c.r, c.cap, graph_sizes=c.sizes)
    s, r = rg.edges()
    e = int(s.shape[0])
    u8 = lambda nb: torch.empty(max(int(nb), 256), dtype=torch.uint8, device=dev)
    cws = u8(L.gm_csr_workspace_bytes(n, cap))
    check(L.gm_csr_from_graph(ptr(rg.ws), n, c.cap, ptr(cws), cws.numel(), current_stream(dev)))
    got_e = C.c_int64(-1)
    check(L.gm_csr_num_edges(ptr(cws), C.byref(got_e), current_stream(dev)))
    assert got_e.value == e
    w = _csr_arrays(cws.cpu().numpy(), n, cap)
    rn, sn = r.cpu().numpy(), s.cpu().numpy()
    order = np.argsort(rn, kind="stable")
    alike = np.array_equal(w["eid"][:e], order) and np.array_equal(w["dst"][:e], rn[order]) and np.array_equal(w["src"][:e], sn[order])
    assert np.array_equal(w["in_ptr"], np.r_[0, np.cumsum(np.bincount(rn, minlength=n))])
    ea_sorted = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
    check(L.gm_edge_features_csr(ptr(pos_t), 3, ptr(cws), n, cap, c.r, ptr(ea_sorted), current_stream(dev)))
    ea = get_edges_displacement(pos_t, s, r, c.r)
    assert_same_bits(ea_sorted[:e], ea[to_dev(w["eid"][:e].astype(np.int64), dev)], "edge features")
    torch.manual_seed(77)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 2).to(dev)
    x = torch.randn((n, 25), generator=torch.Generator().manual_seed(78)).to(dev)
    md = ModelDesc(*m.model_desc())
    fws = u8(L.gm_forward_workspace_bytes(C.byref(md), n, cap))
    out = torch.full((n, 3), float("nan"), device=dev)
    check(L.gm_epd_forward(m.device_handle(dev), ptr(x), n, ptr(ea_sorted), 1, ptr(cws), cap, ptr(out), ptr(fws), fws.numel(),
                           current_stream(dev)))
    ei = torch.stack((s, r)).contiguous()
    with torch.no_grad():
        ref = m.forward(x, ea, ei)
    # the same chain on the destination sort of the emitted edge_index (same kernels: features in sorted order both times)
    ews = u8(L.gm_csr_workspace_bytes(n, e))
    check(L.gm_csr_from_edge_index(ptr(ei), n, e, ptr(ews), ews.numel(), current_stream(dev)))
    ea_ei = torch.zeros((e, 4), dtype=torch.float32, device=dev)
    check(L.gm_edge_features_csr(ptr(pos_t), 3, ptr(ews), n, e, c.r, ptr(ea_ei), current_stream(dev)))
    fws2 = u8(L.gm_forward_workspace_bytes(C.byref(md), n, e))
    out_ei = torch.full((n, 3), float("nan"), device=dev)
    check(L.gm_epd_forward(m.device_handle(dev), ptr(x), n, ptr(ea_ei), 1, ptr(ews), e, ptr(out_ei), ptr(fws2), fws2.numel(),
                           current_stream(dev)))
    err, scale = float((out - ref).abs().max()), float(ref.abs().max())
    print(f"\n[ragged] forward on the ragged csr against EncProcDecGNN.forward on edge_index: max err {err:.3e}, max |ref| {scale:.3e} "
          f"(same bits: {yardstick.same_bits(out, ref)}); orders alike: {alike}; against the chain on csr_from_edge_index: "
          f"max err {float((out - out_ei).abs().max()):.3e}")
    assert torch.isfinite(out).all() and scale > 0 and err <= yardstick.GRAD_TOL * scale
    if alike:
        assert_same_bits(ea_sorted[:e], ea_ei, "sorted edge features")
        assert yardstick.same_bits(out, out_ei)


# ================================================================== the training batch
def fdesc(k, control):
    from gnn_manip_amd.graph import make_feature_desc
    return make_feature_desc(tc.R, STATS, BOUNDS, tc.CART, [tc.MAT], tc.CTRL if control else None, k, tc.REC_DIM + (3 if control else 0))


class Build:
    """The two phases through ctypes, outputs pre-filled with NaN / -7.  frames: [(recording tensor [T, N_b, 5], first frame)];
    ragged: gm_train_batch_build_ragged / _edges_ragged, else the equal-sized entry points (all frames of one size).
    noise_sample: the samples' [k - 1, N_b, 3] blocks."""

    def __init__(self, dev, frames, k, control, max_nb, ragged, ws=None, noise_std=0.0, seed=0, first_stream=0, noise_sample=None):
        from gnn_manip_amd._lib import check, current_stream, lib, ptr
        self.L, self.dev, self.b, self.k_nb, self.ragged = lib(), dev, len(frames), max_nb, ragged
        self.sizes = [int(r.shape[1]) for r, _ in frames]
        self.fd = fdesc(k, control)
        d, f, rows = tc.REC_DIM + (3 if control else 0), 3 * (k - 1) + 7 + (3 if control else 0), sum(self.sizes)
        self.csizes = (C.c_int64 * self.b)(*self.sizes)
        if ragged:
            need = self.L.gm_train_batch_ragged_workspace_bytes(C.byref(self.fd), rows, self.b, max_nb)
        else:
            assert len(set(self.sizes)) == 1
            need = self.L.gm_train_batch_workspace_bytes(C.byref(self.fd), self.b, self.sizes[0], max_nb)
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev) if ws is None else ws
        assert self.ws.numel() >= need
        self.keep = [r for r, _ in frames]
        ptrs = (C.c_void_p * self.b)(*[r.data_ptr() + t * r.shape[1] * r.shape[2] * 4 for r, t in frames])
        nan = float("nan")
        self.nodes = torch.full((rows, f), nan, device=dev)
        self.target = torch.full((rows, 3), nan, device=dev)
        self.windows = torch.full((rows * k * d,), nan, device=dev)          # the samples' [k, N_b, D] blocks back to back
        ns = None if noise_sample is None else torch.cat([to_dev(a, dev).reshape(-1) for a in noise_sample])
        tail = (C.byref(self.fd), max_nb, float(noise_std), seed, first_stream, ptr(ns), ptr(self.nodes), ptr(self.target), ptr(self.windows),
                ptr(self.ws), need, current_stream(dev))
        if ragged:
            check(self.L.gm_train_batch_build_ragged(ptrs, self.csizes, self.b, tc.REC_DIM, *tail))
        else:
            check(self.L.gm_train_batch_build(ptrs, self.b, self.sizes[0], tc.REC_DIM, *tail))

    def record(self, pinned_row):
        """Asynchronous copy of the 16-byte record, and the event behind it."""
        pinned_row.copy_(self.ws[:16].view(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        return ev

    def status(self, pinned_row):
        e = C.c_int64(-1)
        return self.L.gm_train_batch_status(C.c_void_p(pinned_row.data_ptr()), C.byref(e)), int(e.value)

    def edges(self, e):
        from gnn_manip_amd._lib import check, current_stream, ptr
        self.edge_index = torch.full((2, e), -7, dtype=torch.int64, device=self.dev)
        self.edge_attr = torch.full((e, 4), float("nan"), device=self.dev)
        if self.ragged:
            check(self.L.gm_train_batch_edges_ragged(ptr(self.ws), self.csizes, self.b, C.byref(self.fd), self.k_nb, e, ptr(self.edge_index),
                                                     ptr(self.edge_attr), current_stream(self.dev)))
        else:
            check(self.L.gm_train_batch_edges(ptr(self.ws), self.b, self.sizes[0], C.byref(self.fd), self.k_nb, e, ptr(self.edge_index),
                                              ptr(self.edge_attr), current_stream(self.dev)))
        return self

    def finish(self):
        """E through gm_train_batch_status on an asynchronously copied record, then phase 2."""
        pinned = torch.zeros((1, 4), dtype=torch.int32).pin_memory()
        self.record(pinned[0]).synchronize()
        rc_, e = self.status(pinned[0])
        assert rc_ == 0 and 0 < e <= sum(self.sizes) * self.k_nb, (rc_, e)
        return self.edges(e)

    def outputs(self):
        return dict(nodes=self.nodes, target=self.target, windows=self.windows, edge_index=self.edge_index, edge_attr=self.edge_attr)


_REC = {}


def case_frames(name, dev):
    c = rc.BATCHES[name]
    if name not in _REC:
        _REC[name] = [to_dev(r, dev) for r in c.recordings()]
    return c, list(zip(_REC[name], c.first_frames))


def collate_singles(dev, c, frames, noise_sample=None, **kw):
    """Single-sample gm_train_batch_build / _edges builds on streams first_stream + b, collated with the running row offset."""
    first = kw.pop("first_stream", 0)
    outs, off = [], 0
    for b, fr in enumerate(frames):
        ns = None if noise_sample is None else [noise_sample[b]]
        o = Build(dev, [fr], c.k, c.control, c.max_nb, False, first_stream=first + b, noise_sample=ns, **kw).finish().outputs()
        o["edge_index"] = o["edge_index"] + off
        off += o["nodes"].shape[0]
        outs.append(o)
    return {key: torch.cat([o[key] for o in outs], dim=1 if key == "edge_index" else 0) for key in outs[0]}


MODES = {"no_noise": dict(), "injected": dict(injected=True), "drawn": dict(noise_std=tc.NOISE_STD, seed=(0x77 << 32) | 5, first_stream=(1 << 32) - 2)}
_SINGLES = {}


def _mode_kw(c, mode):
    kw = dict(MODES[mode])
    if kw.pop("injected", False):
        kw["noise_sample"] = [tc.noise_sample32(77, 5 + b, n, c.k, tc.NOISE_STD) for b, n in enumerate(c.sizes)]
    return kw


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(rc.BATCHES))
def test_ragged_batch_is_the_collate_of_single_builds(dev, name, mode):
    c, frames = case_frames(name, dev)
    kw = _mode_kw(c, mode)
    want = _SINGLES[(name, mode)] = collate_singles(dev, c, frames, **kw)
    got = Build(dev, frames, c.k, c.control, c.max_nb, True, **kw).finish().outputs()
    for key in want:
        assert_same_bits(got[key], want[key], f"{name} {mode} {key}")
    assert torch.isfinite(got["nodes"]).all() and torch.isfinite(got["windows"]).all() and int(got["edge_index"].min()) >= 0
    off = rc.offsets(c.sizes)
    graph = np.searchsorted(off, got["edge_index"].cpu().numpy(), side="right") - 1
    assert (graph[0] == graph[1]).all() and set(graph[0]) == set(range(c.B))
    if mode != "no_noise":
        clean = _SINGLES.get((name, "no_noise"))
        assert clean is None or not np.array_equal(clean["windows"].cpu().numpy(), got["windows"].cpu().numpy())
    if name == "same97":
        one = Build(dev, frames, c.k, c.control, c.max_nb, False, **kw).finish().outputs()
        for key in want:
            assert_same_bits(got[key], one[key], f"same97 {mode} against the equal-sized build: {key}")


def test_non_finite_position_in_the_last_sample_is_reported(dev):
    c, frames = case_frames("mixed6", dev)
    rec, t = frames[-1]
    bad = rec.clone()
    bad[t + c.k, rec.shape[1] - 1, 3] = float("nan")                 # the frame after the window, the batch's last row
    b = Build(dev, frames[:-1] + [(bad, t)], c.k, c.control, c.max_nb, True)
    pinned = torch.zeros((1, 4), dtype=torch.int32).pin_memory()
    b.record(pinned[0]).synchronize()
    assert b.status(pinned[0])[0] == -5 and b"non-finite position" in b.L.gm_last_error()
    good = Build(dev, frames, c.k, c.control, c.max_nb, True, ws=b.ws)    # the flag does not outlive its build
    good.record(pinned[0]).synchronize()
    assert good.status(pinned[0])[0] == 0


def test_two_ragged_batches_in_flight(dev):
    ca, fa = case_frames("mixed6", dev)
    cb, fb = case_frames("mixed_cap5", dev)
    kwa = dict(noise_std=tc.NOISE_STD, seed=3, first_stream=0)
    kwb = dict(noise_std=tc.NOISE_STD, seed=3, first_stream=ca.B)
    alone_a = Build(dev, fa, ca.k, ca.control, ca.max_nb, True, **kwa).finish()
    alone_b = Build(dev, fb, cb.k, cb.control, cb.max_nb, True, **kwb).finish()
    pinned = torch.zeros((2, 4), dtype=torch.int32).pin_memory()
    a = Build(dev, fa, ca.k, ca.control, ca.max_nb, True, **kwa)                 # phase 1 of A into workspace 0
    ev_a = a.record(pinned[0])
    b = Build(dev, fb, cb.k, cb.control, cb.max_nb, True, **kwb)                 # phase 1 of B into workspace 1, A's phase 2 still to come
    ev_b = b.record(pinned[1])
    counts = []
    for x, ev, row in ((a, ev_a, pinned[0]), (b, ev_b, pinned[1])):
        ev.synchronize()
        rc_, e = x.status(row)
        assert rc_ == 0
        counts.append(e)
    a.edges(counts[0])
    b.edges(counts[1])
    assert counts == [alone_a.edge_index.shape[1], alone_b.edge_index.shape[1]] and counts[0] != counts[1]
    for got, want in ((a, alone_a), (b, alone_b)):
        for key, v in want.outputs().items():
            assert_same_bits(got.outputs()[key], v, "in flight " + key)


# ================================================================== the loader
@pytest.fixture(scope="module")
def mixed_dataset(dev):
    from gnn_manip_amd import CoffeeDataset
    recs = [to_dev(tc.Case("loader", n, 6, [(0, 1)], seed=40 + n).recordings()[0], dev) for n in rc.LOADER_N]
    assert [tuple(r.shape) for r in recs] == [(8, n, tc.REC_DIM) for n in rc.LOADER_N]
    ds = CoffeeDataset.from_recordings(recs, 6, tc.R, STATS, BOUNDS, tc.CART, tc.MAT, tc.CTRL, noise=tc.NOISE_STD, use_control=True,
                                       max_neighbours=12)
    assert len(ds) == 6                                                  # T = 8: two windows per recording
    return ds


def assert_same_batches(got, want, what):
    assert len(got) == len(want) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        for key in ("x", "edge_attr", "edge_index", "y"):
            assert_same_bits(getattr(a, key), getattr(b, key), f"{what} batch {i} {key}")


def _want_batches(ds, seed):
    from gnn_manip_amd.dataset import collate_graphs
    return [collate_graphs([ds.batch([i], seed=seed, first_stream=i) for i in idx]) for idx in ((0, 1, 2), (3, 4, 5))]


def test_loader_over_three_sizes(dev, mixed_dataset):
    from gnn_manip_amd import GraphLoader
    ds = mixed_dataset
    want = _want_batches(ds, 21)
    assert [b.num_nodes for b in want] == [64 + 64 + 97, 97 + 300 + 300]
    assert_same_batches([ds.batch([0, 1, 2], seed=21, first_stream=0), ds.batch([3, 4, 5], seed=21, first_stream=3)], want, "CoffeeDataset.batch")
    for prefetch in (0, 1):
        got = list(GraphLoader(ds, batch_size=3, shuffle=False, seed=21, fused=True, prefetch=prefetch))
        assert_same_batches(got, want, f"prefetch={prefetch}")
    ei = want[1].edge_index.cpu().numpy()
    graph = np.searchsorted([97, 397, 697], ei, side="right")
    assert (graph[0] == graph[1]).all() and set(graph[0]) == {0, 1, 2}


def test_loader_makes_one_build_per_batch_and_does_not_synchronise(dev, mixed_dataset, monkeypatch):
    from gnn_manip_amd import GraphLoader, _lib
    ds = mixed_dataset
    want = _want_batches(ds, 21)
    calls = []
    L = _lib.lib()

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped

    watched = [name for name in _lib.PROTOTYPES if name.endswith("_num_edges")]
    watched += ["gm_train_batch_build", "gm_train_batch_build_ragged", "gm_train_batch_edges", "gm_train_batch_edges_ragged"]
    for name in watched:
        monkeypatch.setattr(L, name, spy(name, getattr(L, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", spy("torch.cuda.synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("Stream.synchronize", torch.cuda.Stream.synchronize))
    for prefetch in (0, 1):
        del calls[:]
        got = []
        for batch in GraphLoader(ds, batch_size=3, shuffle=False, seed=21, fused=True, prefetch=prefetch):
            got.append((batch, list(calls)))
        builds = [c for c in calls if "_build" in c]
        edges = [c for c in calls if "_edges" in c]
        assert builds == ["gm_train_batch_build_ragged"] * 2 and edges == ["gm_train_batch_edges_ragged"] * 2, calls
        assert sorted(calls) == sorted(builds + edges), calls            # nothing else: no synchronise, no *_num_edges
        if prefetch:                                                      # batch 1 was built before batch 0 was handed out
            assert got[0][1].count("gm_train_batch_build_ragged") == 2 and got[0][1].count("gm_train_batch_edges_ragged") == 1
        assert_same_batches([b for b, _ in got], want, f"under the spies, prefetch={prefetch}")
