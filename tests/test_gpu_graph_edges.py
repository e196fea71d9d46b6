"""The graph front end on ties and degenerate geometry (cases: graph_cases.py; their CPU side: test_graph_cases.py).

The front end returns integers -- which particles are neighbours, in what order, where each edge sits in the destination-sorted
list and in the 32-edge block tables -- so almost everything here is compared bit for bit: the radius graph with the float64
oracle (contract: include/gnn_manip_hip.h, "ties broken on the smaller index"), the destination sort with numpy's stable argsort,
the block tables with their restatement in graph_cases.block_tables.  The float comparisons (Parts B and C) use the bars the
existing rollout / forward tests use, unchanged.  Every case asserts its own regime before the GPU is touched."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_cases as gc
from conftest import BOUNDS, CART, CTRL, MAT, STATS, assert_forward_close
from oracle import epd_oracle as orc
from gpu_support import dev, graph_attr, load_model as _model, to_dev as _t

pytestmark = pytest.mark.gpu

GM_ERR_INVALID_ARGUMENT, GM_ERR_UNSUPPORTED = -1, -2


# ------------------------------------------------------------------ reading a csr workspace back
def _parse_csr(raw, n, cap):
    """The arrays of a csr workspace, carved the way the library does (carve_csr, carve_edge_blocks: 256-byte aligned arrays
    behind a 16-byte header; the block tables are one array of ints).  raw: the workspace as uint8."""
    ints = raw[:raw.shape[0] // 4 * 4].view(np.int32)
    off = [16]

    def take(count):
        o = (off[0] + 255) // 256 * 256
        off[0] = o + 4 * count
        return ints[o // 4:o // 4 + count], o

    out = dict(header=ints[:4].copy())
    out["in_ptr"], _ = take(n + 1)
    take(n + 1)                                  # cursor
    for k in ("dst", "src", "eid"):
        out[k], _ = take(cap)
    take(2 * ((max(n + 1, 1) + 2047) // 2048) + 4)   # scan state
    take(2 * cap)                                # sort_tmp
    nblk = (cap + 31) // 32 + 4 * n + 4          # capacity of the tables
    tab, o = take(8 + (n + 2) + 1 + 4 * nblk + (nblk // 4 + 2) + 2 * n)
    p = 8 + n + 2
    p += 1 if (o + 4 * p) & 4 else 0             # int2 alignment
    out.update(n_blocks=int(tab[0]), n_groups=int(tab[1]), n_graphs=int(tab[2]), n_stitch=int(tab[4]),
               blk=tab[p:p + 2 * nblk].reshape(-1, 2), seg=tab[p + 2 * nblk:p + 4 * nblk].reshape(-1, 2),
               head=tab[p + 4 * nblk:p + 4 * nblk + nblk // 4 + 2])
    q = p + 4 * nblk + nblk // 4 + 2
    out.update(stitch=tab[q:q + n], stitch_list=tab[q + n:q + 2 * n])
    return out


def _check_sorted_structure(w, n, agg, other, single_graph=True):
    """w: a parsed workspace; agg / other: the aggregation row and the other row of the edge list it was built from."""
    e = agg.shape[0]
    assert int(w["header"][0]) == e and int(w["header"][1]) == 0
    order = np.argsort(agg, kind="stable")
    assert np.array_equal(w["in_ptr"], np.r_[0, np.cumsum(np.bincount(agg, minlength=n))])
    assert np.array_equal(w["eid"][:e], order)
    assert np.array_equal(w["dst"][:e], agg[order]) and np.array_equal(w["src"][:e], other[order])
    if not single_graph:
        return
    t = gc.block_tables(agg[order], n)
    nb = t["n_blocks"]
    assert (w["n_blocks"], w["n_groups"], w["n_graphs"]) == (nb, nb // 4, 1)
    assert np.array_equal(w["blk"][:nb], t["blk"])
    assert np.array_equal(w["seg"][:nb].astype(np.int64) & 0xffffffff, t["seg"])
    assert np.array_equal(w["head"][:nb // 4], t["head"]), (np.flatnonzero(w["head"][:nb // 4] != t["head"])[:8],)
    assert np.array_equal(w["stitch"], t["stitch"])
    want = np.flatnonzero(t["stitch"] >= 0)
    assert w["n_stitch"] == want.shape[0] and np.array_equal(np.sort(w["stitch_list"][:w["n_stitch"]]), want)


# ================================================================== Part A: radius graph and its destination sort
def _oracle_edges(c):
    """orc.get_connectivity per graph of the batch, indices offset by the graph's first row (collate_utils.py:76)."""
    n = c.props["n"]
    n_per = c.n_per or n
    if n_per < n and n_per == 1728:      # G copies of one lattice: the single-graph result, once
        s1, r1 = orc.get_connectivity(c.pos[:n_per], c.r, c.cap)
        assert all(np.array_equal(c.pos[g:g + n_per], c.pos[:n_per]) for g in range(0, n, n_per))
        return (np.concatenate([s1 + g for g in range(0, n, n_per)]), np.concatenate([r1 + g for g in range(0, n, n_per)]))
    ss, rr = [], []
    for g in range(0, n, n_per):
        s, r = orc.get_connectivity(c.pos[g:g + n_per], c.r, c.cap)
        ss.append(s + g)
        rr.append(r + g)
    return np.concatenate(ss), np.concatenate(rr)


def _destination_sort_of_graph(rg, pos_t, s, r, c, dev):
    """gm_csr_from_graph_flow over the radius graph's workspace at both flows: a stable sort by aggregation node (bit exact, block
    tables included), and gm_edge_features_csr == gm_edge_features row for row through eid."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    n, k = rg.n, rg.max_neighbours
    cap, e = n * k, s.shape[0]
    ts, tr = _t(s, dev), _t(r, dev)
    ref = torch.empty((e, 4), dtype=torch.float32, device=dev)
    check(L.gm_edge_features(ptr(pos_t), 3, ptr(ts), ptr(tr), e, c.r, ptr(ref), current_stream(dev)))
    ref = ref.cpu().numpy()
    np.testing.assert_allclose(ref, orc.get_edges_displacement(c.pos, s, r, c.r), rtol=2e-7, atol=0)
    for flow in (0, 1):
        ws = torch.empty(max(int(L.gm_csr_workspace_bytes(n, cap)), 256), dtype=torch.uint8, device=dev)
        check(L.gm_csr_from_graph_flow(ptr(rg.ws), n, k, flow, ptr(ws), ws.numel(), current_stream(dev)))
        got = C.c_int64(-1)
        check(L.gm_csr_num_edges(ptr(ws), C.byref(got), current_stream(dev)))
        assert got.value == e
        out = torch.empty((cap, 4), dtype=torch.float32, device=dev)
        check(L.gm_edge_features_csr(ptr(pos_t), 3, ptr(ws), n, cap, c.r, ptr(out), current_stream(dev)))
        w = _parse_csr(ws.cpu().numpy(), n, cap)
        assert int(w["header"][2]) == flow
        agg, other = (r, s) if flow == 0 else (s, r)
        _check_sorted_structure(w, n, agg, other, single_graph=not (c.n_per and c.n_per < n))
        np.testing.assert_array_equal(out.cpu().numpy()[:e], ref[w["eid"][:e]])
    return np.bincount(r, minlength=n).max()


@pytest.mark.parametrize("name", list(gc.GEOMETRY))
def test_radius_graph_and_destination_sort_bit_exact(dev, name):
    from gnn_manip_amd.graph import RadiusGraph
    c = gc.geometry(name)
    c.check()
    so, ro = _oracle_edges(c)
    pos_t = _t(c.pos, dev)
    rg = RadiusGraph(pos_t, c.r, c.cap, c.n_per)
    s, r = (x.cpu().numpy() for x in rg.edges())
    assert s.dtype == np.int64 and rg.num_edges() == so.shape[0]
    assert np.array_equal(s, so), name
    bad = np.flatnonzero(r != ro) if r.shape == ro.shape else None
    assert np.array_equal(r, ro), (name, None if bad is None else (bad[:5], s[bad[:5]], r[bad[:5]], ro[bad[:5]]))
    if c.n_per:
        assert np.array_equal(s // c.n_per, r // c.n_per)         # no edge crosses graphs
    max_indeg = _destination_sort_of_graph(rg, pos_t, s, r, c, dev)
    if name == "a3_cluster150":
        assert max_indeg > gc.SEG_CAP                               # the long-segment path of the sort, from a radius graph


def test_radius_graph_argument_errors_are_status_codes(dev):
    """max_neighbours outside 1 .. 160 is GM_ERR_UNSUPPORTED, a batch whose size is not a multiple of nodes_per_graph
    GM_ERR_INVALID_ARGUMENT -- before any launch; the next build is unaffected."""
    from gnn_manip_amd import get_connectivity
    from gnn_manip_amd._lib import GMError
    c = gc.geometry("a7_over160_cap160")
    pos = _t(c.pos, dev)
    for cap in (161, 0, -3):
        with pytest.raises(GMError) as ei:
            get_connectivity(pos, c.r, cap)
        assert ei.value.code == GM_ERR_UNSUPPORTED, cap
    with pytest.raises(GMError) as ei:
        get_connectivity(pos[:10], c.r, 20, nodes_per_graph=3)
    assert ei.value.code == GM_ERR_INVALID_ARGUMENT
    s, r = get_connectivity(pos[:10], c.r, 20, nodes_per_graph=5)
    so, ro = orc.get_connectivity(c.pos[:5], c.r, 20)
    so2, ro2 = orc.get_connectivity(c.pos[5:10], c.r, 20)
    assert np.array_equal(s.cpu().numpy(), np.r_[so, so2 + 5]) and np.array_equal(r.cpu().numpy(), np.r_[ro, ro2 + 5])


# ================================================================== Part B: the fused rollout path on the same inputs
KW = dict(stats=STATS, bounds=BOUNDS, conn_r=0.015, cartesian_idx=CART, material_idx=MAT, control_idx=CTRL)


def _scene(name):
    from gnn_manip_amd import scene
    sc = gc.scene_case(name)
    sc.geo.check()
    assert sc.geo.r == 0.015 and sc.geo.cap == 20
    obs = sc.obs
    trajs = np.stack([scene.rigid_drift_trajectory(obs, 1, seed=100 + k, step_size=3e-4) for k in range(3)])
    e_ref = orc.get_connectivity(obs[-1][:, 2:5], 0.015, 20)[0].shape[0]
    return obs, trajs, e_ref


@pytest.mark.parametrize("name", ["lattice9", "cluster200"])
def test_one_rollout_step_on_ties_and_coincident_rows(dev, name):
    """ONE step of RolloutEngine (radius_graph_build_fused / csr_from_graph_fused: the counting pass rides in the neighbour kernels,
    the block tables and the edge features in the segment sort) from a last frame with ties: the oracle's edge count exactly, its
    positions at the rollout tests' bar, candidate c of a batch == its stand-alone run bit for bit -- with each processor kernel.
    One step only: after it the tied particles sit a rounding error apart, and the neighbour order is then legitimately
    undecidable between float32 implementations."""
    from gnn_manip_amd import RolloutEngine
    obs, trajs, e_ref = _scene(name)
    n = obs.shape[1]
    params = orc.init_params(25, 4, 3, 128, 2, 10, 96)
    m = _model(params, (25, 4, 3, 128, 2, 10), dev)
    ref = orc.rollout(params, obs, trajs[0], 1, STATS, BOUNDS, 0.015, CART, MAT, CTRL)
    for kernel in ("auto", "hm", "sys_all"):
        m.set_edge_kernel(kernel)
        with torch.no_grad():
            eng_1 = RolloutEngine(m, graph_attr(0.015), n, device=dev)
            singles = []
            for k in range(3):
                singles.append(eng_1.rollout(_t(obs, dev), _t(trajs[k], dev), horizon=1).cpu().numpy())
                assert eng_1.status() == e_ref, (kernel, k)
            eng_b = RolloutEngine(m, graph_attr(0.015), n, device=dev, candidates=3)
            out = eng_b.rollout_candidates(_t(obs, dev), _t(trajs, dev)).cpu().numpy()
            assert eng_b.status() == 3 * e_ref, kernel
        for k in range(3):
            assert np.array_equal(out[k], singles[k]), (kernel, k, np.abs(out[k] - singles[k]).max())
        err = np.abs(singles[0][:, :, 2:5] - ref[:, :, 2:5]).max()
        print(f"{name} {kernel}: E = {e_ref}, max |pos - oracle| = {err:.3e}")
        np.testing.assert_allclose(singles[0][:, :, 2:5], ref[:, :, 2:5], rtol=0, atol=5e-6)
        np.testing.assert_array_equal(singles[0][:, :, :2], ref[:, :, :2])


@pytest.mark.parametrize("name", ["cluster1100", "cluster200"])
def test_renumbered_step_with_and_without_an_overfull_cell(dev, name):
    """The renumbered loop (renumber_every = 1) against the plain one, under the bound of
    test_renumbered_rollout_matches_the_plain_one_and_the_oracle: on a scene with a cell of more than 1024 rows
    (cell_order_kernel raises order_skip and the rows stay where they are) and on one without."""
    from gnn_manip_amd import RolloutEngine
    obs, trajs, e_ref = _scene(name)
    n = obs.shape[1]
    assert (gc.scene_case(name).geo.props["fullest_cell"] > gc.CELL_ORDER_CAP) == (name == "cluster1100")
    params = orc.init_params(25, 4, 3, 128, 2, 10, 314)
    # Damped messages: 1100 coincident rows send 1100 IDENTICAL messages to each of the cluster's first 20 rows, and with
    # init_params' LayerNorm weights (about 1) that sum drives the node MLP's hidden activations past the fp16 split range of the
    # inference kernels (measured: the step is flagged GM_ERR_DATA, as include/gnn_manip_hip.h documents).  This test is about the row
    # order, so the processor's edge LayerNorms are scaled by 1/32 -- in the oracle's parameters and the engine's alike.
    for k in range(10):
        for leaf in ("weight", "bias"):
            params[f"processor.{k}.phi_edge.5.{leaf}"] = params[f"processor.{k}.phi_edge.5.{leaf}"] * np.float32(1.0 / 32.0)
    m = _model(params, (25, 4, 3, 128, 2, 10), dev)
    with torch.no_grad():
        plain = RolloutEngine(m, graph_attr(0.015), n, device=dev, renumber=False)
        f0, r0 = plain.rollout(_t(obs, dev), _t(trajs[0], dev), horizon=1, record=True)
        e0 = plain.status()
        ren = RolloutEngine(m, graph_attr(0.015), n, device=dev, renumber=True)
        ren.RENUMBER_EVERY = 1
        f1, r1 = ren.rollout(_t(obs, dev), _t(trajs[0], dev), horizon=1, record=True)
        e1 = ren.status()
        f2, r2 = ren.rollout(_t(obs, dev), _t(trajs[0], dev), horizon=1, record=True)
    assert ren.renumber and not plain.renumber and e0 == e1 == e_ref
    assert torch.equal(f1, f2) and torch.equal(r1, r2)
    f0, r0, f1, r1 = (x.cpu().numpy() for x in (f0, r0, f1, r1))
    np.testing.assert_array_equal(f1[:, :, :2], obs[:, :, :2])
    print(f"{name}: E = {e_ref}, max |renumbered - plain| = {np.abs(f1[:, :, 2:8] - f0[:, :, 2:8]).max():.3e}")
    np.testing.assert_allclose(f1[:, :, 2:8], f0[:, :, 2:8], rtol=0, atol=2e-6)
    np.testing.assert_allclose(r1[:, :, 2:8], r0[:, :, 2:8], rtol=0, atol=2e-6)
    ref = orc.rollout(params, obs, trajs[0], 1, STATS, BOUNDS, 0.015, CART, MAT, CTRL)
    np.testing.assert_allclose(f1[:, :, 2:8], ref[:, :, 2:8], rtol=0, atol=5e-6)
    np.testing.assert_allclose(f0[:, :, 2:8], ref[:, :, 2:8], rtol=0, atol=5e-6)


# ================================================================== Part C: block-boundary degree structures
def _inputs(c, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.standard_normal((c.n, 25)).astype(np.float32), rng.standard_normal((c.props["e"], 4)).astype(np.float32)


@pytest.mark.parametrize("name", list(gc.DEGREES))
def test_destination_sort_and_block_tables_of_an_edge_index(dev, name):
    """gm_csr_from_edge_index_flow + build_edge_blocks on segments placed on purpose: eid, dst, src, in_ptr against numpy's stable
    argsort and blk / seg / head / stitch against their restatement, at both flows, with the columns as built and permuted again."""
    from gnn_manip_amd.epd_gnn import DstCsr
    c = gc.degree_case(name)
    c.check()
    e = c.props["e"]
    perm = np.random.Generator(np.random.PCG64(7)).permutation(e)
    for ei in (c.edge_index, np.ascontiguousarray(c.edge_index[:, perm])):
        for flow in (0, 1):
            csr = DstCsr(_t(ei, dev), c.n, flow=flow)
            assert csr.validate() == e
            w = _parse_csr(csr.ws.cpu().numpy(), c.n, e)
            _check_sorted_structure(w, c.n, ei[1 - flow], ei[flow])


@pytest.mark.parametrize("name", list(gc.DEGREES))
def test_forward_on_block_boundary_degrees(dev, name):
    """EncProcDecGNN.forward (hidden 128 / 2 layers) over the same graphs with each processor kernel: the oracle's result at the
    forward bar, two runs bit for bit; the standalone processor block at the bar of test_scatter_add_is_deterministic_with_hub_nodes."""
    c = gc.degree_case(name)
    c.check()
    ei, e = c.edge_index, c.props["e"]
    nodes, ea = _inputs(c, 160)
    params = orc.init_params(25, 4, 3, 128, 2, 3, 74)
    m = _model(params, (25, 4, 3, 128, 2, 3), dev)
    ref = orc.epd_forward(params, nodes, ea, ei, 2, 3)
    h0, e0 = orc.graph_independent(params, "encoder", nodes, ea, 2)
    h1o, e1o = orc.interaction_network(params, "processor.0", h0, e0, ei, 2)
    for kernel in ("auto", "hm", "sys_all"):
        m.set_edge_kernel(kernel)
        with torch.no_grad():
            outs = [m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy() for _ in range(2)]
            assert m.status() == e
            h1, e1, _ = m.processor[0](_t(h0, dev), _t(e0, dev), _t(ei, dev))
        assert np.array_equal(outs[0], outs[1]), kernel
        assert_forward_close(outs[0], ref, floor=1e-3, what=f"{name} {kernel}")
        np.testing.assert_allclose(h1.cpu().numpy(), h1o, rtol=1e-5, atol=2e-5)
        np.testing.assert_allclose(e1.cpu().numpy(), e1o, rtol=1e-5, atol=2e-5)


@pytest.mark.parametrize("hidden", [64, 256])
@pytest.mark.parametrize("name", ["c_hub384_at_group_plus_1", "c_degrees_31_to_129", "c_hub_is_node0"])
def test_forward_on_block_boundary_degrees_other_widths(dev, name, hidden):
    c = gc.degree_case(name)
    c.check()
    nodes, ea = _inputs(c, 161)
    params = orc.init_params(25, 4, 3, hidden, 2, 3, 75)
    m = _model(params, (25, 4, 3, hidden, 2, 3), dev)
    m.set_edge_kernel("hm")
    with torch.no_grad():
        outs = [m.forward(_t(nodes, dev), _t(ea, dev), _t(c.edge_index, dev)).cpu().numpy() for _ in range(2)]
    assert np.array_equal(outs[0], outs[1])
    assert_forward_close(outs[0], orc.epd_forward(params, nodes, ea, c.edge_index, 2, 3), floor=1e-3, what=f"{name} h{hidden}")
