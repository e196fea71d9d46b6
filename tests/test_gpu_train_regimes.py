"""Training path on the MI355X in the regimes tests/test_gpu_train.py does not reach (same yardstick: forward and loss 1e-5; every
parameter gradient by the rule of tests/yardstick.py against the float64 gradient of oracle/torch_epd.py, relu_flip_allowance as the
only fallback).

A. More than one tile per workgroup.  train_bwd_kernel with a LayerNorm is launched with at most CUs x (2 at hidden <= 128, else 1)
   workgroups of 128 rows (csrc/train.hip: launch_train_bwd); train_fwd_kernel and the other backward kinds with at most 2048
   (grid_tiles).  Past that a workgroup walks several tiles: it restarts the weight-stream ring, re-uses its LDS turn and keeps
   adding into its LayerNorm parameter sums.  Every case asserts from the device's CU count that it is past the limit it is there
   for, so it cannot pass without entering its regime.  At these sizes the weight-gradient chunk length (wgrad_flush) is hundreds
   of rows instead of its floor of 64.
B. Graphs that are not radius graphs: a seeded random multigraph with hub destinations and hub sources (segments of 700 and 300
   rows in segment_sum_kernel, with and without its perm indirection, at all three rows-per-wave-step widths), duplicate edges,
   self loops, send-only / receive-only / isolated nodes, and edges in random order -- through the full model and through the
   standalone InteractionNetwork, whose input gradients dh_in / de_in (de_in row for row in the caller's edge order) are compared
   with float64 autograd here.

The block-level comparisons use the same rule, with relu_flip_allowance restated for one block as their only fallback: de_in is a
per-row quantity, so a single unit whose sign differs between two float32-accurate evaluations shows undiluted in its row."""
import functools

import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
from oracle import torch_epd
import yardstick
from gpu_support import check_training_step as _check, cus as _cus, dev, l1_step, load_model as _model, tiles as _tiles, to_dev as _t
from train_cases import HUB_E, HUB_N, benchmark_graph as _benchmark_graph, graph as _graph, hub_graph as _hub_graph

pytestmark = pytest.mark.gpu

FWD_GRID_TILES = 2048  # grid_tiles(): workgroups of train_fwd_kernel and of the backward kinds without a LayerNorm


def _report(case, res):
    """The worst err / tol of the case (printed before anything else can fail), and whether the relu-flip fallback ran."""
    worst, after = res
    print(f"\n[regimes] {case}: worst err/tol {worst[1]:.3f} at {worst[0]!r}" + (f" (err {worst[2]:.3e}, tol {worst[3]:.3e})" if len(worst) > 2 else "")
          + (f"; relu_flip_allowance fallback ran: worst with allowance {after[1]:.3f} at {after[0]!r}" if after is not None else "; no fallback"))


def _assert_every_parameter_is_compared(m, params, num_layers):
    """gpu_support.compare_parameter_gradients walks m.named_parameters(): those are all of the oracle's tensors, the LayerNorm weight / bias of every
    normed MLP (the tensors that depend on a workgroup's sums surviving from tile to tile) among them, and each has a gradient."""
    names = [k for k, _ in m.named_parameters()]
    assert sorted(names) == sorted(params.keys())
    k = 2 * num_layers + 1
    ln = [n for n in names if n.endswith(f".{k}.weight") or n.endswith(f".{k}.bias")]
    assert len(ln) == 2 * (2 + 2 * len(m.processor))          # decoder: no LayerNorm
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters()}


def _step(m, nodes, ea, ei, target, dev):
    out, _ = l1_step(m, nodes, ea, ei, target, dev)
    return out.detach(), _grads(m)


# ------------------------------------------------------------------ A: more than one tile per workgroup
def test_benchmark_shape_backward_walks_three_tiles_per_workgroup(dev):
    """The configuration the published training number is measured on (two collated 5000-node scenes, hidden 128), at two
    message-passing steps: TB_EDGE, and TB_ENC on the edges, run several tiles per workgroup."""
    nodes, ea, ei = _benchmark_graph()
    assert _tiles(ea.shape[0]) > 2 * _cus(dev), (ea.shape[0], _cus(dev))
    dims = (25, 4, 3, 128, 2, 2)
    params = orc.init_params(*dims, 150)
    m = _model(params, dims, dev)
    res = _check(m, params, nodes, ea, ei, dims, dev, 150)
    _report(f"benchmark shape, N={nodes.shape[0]} E={ea.shape[0]} hidden 128", res)
    _assert_every_parameter_is_compared(m, params, dims[4])


def test_benchmark_shape_gradients_are_bit_identical_across_runs(dev):
    """No atomics in the weight-gradient reduce, the LayerNorm parameter reduce or the segment sums: the same step on two fresh
    copies of the model gives the same bits, also when a workgroup's sums run over several tiles."""
    nodes, ea, ei = _benchmark_graph()
    assert _tiles(ea.shape[0]) > 2 * _cus(dev), (ea.shape[0], _cus(dev))
    dims = (25, 4, 3, 128, 2, 2)
    params = orc.init_params(*dims, 150)
    target = np.random.default_rng(150).standard_normal((nodes.shape[0], 3)).astype(np.float32)
    out_a, g_a = _step(_model(params, dims, dev), nodes, ea, ei, target, dev)
    out_b, g_b = _step(_model(params, dims, dev), nodes, ea, ei, target, dev)
    assert torch.equal(out_a, out_b)
    assert sorted(g_a) == sorted(params.keys())
    for k in g_a:
        assert torch.equal(g_a[k], g_b[k]), k


def test_forward_kernels_walk_tiles_past_their_grid(dev):
    """More edge tiles than train_fwd_kernel's grid: TK_ENC_EDGE / TK_PROC_EDGE (and the backward kinds without a LayerNorm
    limit) stride over tiles."""
    nodes, ea, ei = _graph(15000, 0.18, 151)
    assert _tiles(ea.shape[0]) > FWD_GRID_TILES, ea.shape[0]
    assert _tiles(ea.shape[0]) > 2 * _cus(dev), (ea.shape[0], _cus(dev))
    dims = (25, 4, 3, 128, 2, 1)
    params = orc.init_params(*dims, 151)
    m = _model(params, dims, dev)
    res = _check(m, params, nodes, ea, ei, dims, dev, 151)
    _report(f"forward grid-stride, N={nodes.shape[0]} E={ea.shape[0]} hidden 128", res)
    _assert_every_parameter_is_compared(m, params, dims[4])


def test_many_nodes_sparse_graph_walks_node_tiles(dev):
    """More node tiles than backward workgroups: TB_NODE, and TB_ENC on the nodes, carry the node-side LayerNorm sums across
    tiles."""
    nodes, ea, ei = _graph(70000, 0.7, 152)
    assert _tiles(nodes.shape[0]) > 2 * _cus(dev), (nodes.shape[0], _cus(dev))
    assert _tiles(ea.shape[0]) > FWD_GRID_TILES, ea.shape[0]
    dims = (25, 4, 3, 128, 2, 1)
    params = orc.init_params(*dims, 152)
    m = _model(params, dims, dev)
    res = _check(m, params, nodes, ea, ei, dims, dev, 152)
    _report(f"many nodes, N={nodes.shape[0]} E={ea.shape[0]} hidden 128", res)
    _assert_every_parameter_is_compared(m, params, dims[4])


def test_hidden_256_backward_walks_tiles(dev):
    """Hidden 256 runs one backward workgroup per CU."""
    nodes, ea, ei = _graph(2500, 0.1, 153)
    assert _tiles(ea.shape[0]) > _cus(dev), (ea.shape[0], _cus(dev))
    dims = (25, 4, 3, 256, 2, 1)
    params = orc.init_params(*dims, 153)
    m = _model(params, dims, dev)
    res = _check(m, params, nodes, ea, ei, dims, dev, 153)
    _report(f"hidden 256, N={nodes.shape[0]} E={ea.shape[0]}", res)
    _assert_every_parameter_is_compared(m, params, dims[4])


def test_hidden_64_three_layers_backward_walks_tiles(dev):
    """The third width, and the run-time loop over the hidden Linears (num_layers 3) across tiles."""
    nodes, ea, ei = _benchmark_graph()
    assert _tiles(ea.shape[0]) > 2 * _cus(dev), (ea.shape[0], _cus(dev))
    dims = (25, 4, 3, 64, 3, 1)
    params = orc.init_params(*dims, 154)
    m = _model(params, dims, dev)
    res = _check(m, params, nodes, ea, ei, dims, dev, 154)
    _report(f"hidden 64 x 3 layers, N={nodes.shape[0]} E={ea.shape[0]}", res)
    _assert_every_parameter_is_compared(m, params, dims[4])


# ------------------------------------------------------------------ B: graphs that are not radius graphs
@pytest.mark.parametrize("hidden,seed", [(64, 160), (128, 161), (256, 162)])
def test_hub_graph_full_model(dev, hidden, seed):
    """EncProcDecGNN under autograd on the hub graph: the source-sorted CSR, segment sums of 700 and 300 rows with and without
    the perm indirection, 4 / 2 / 1 rows per wave step."""
    ei = _hub_graph()
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes = rng.standard_normal((HUB_N, 25)).astype(np.float32)
    ea = rng.standard_normal((HUB_E, 4)).astype(np.float32)
    dims = (25, 4, 3, hidden, 2, 2)
    params = orc.init_params(*dims, seed)
    m = _model(params, dims, dev)
    res = _check(m, params, nodes, ea, ei, dims, dev, seed)
    _report(f"hub graph, full model, hidden {hidden}", res)
    _assert_every_parameter_is_compared(m, params, dims[4])
    # bit-stable: the same step on a fresh copy of the model
    target = np.random.default_rng(seed).standard_normal((HUB_N, 3)).astype(np.float32)   # _check's target
    _, g2 = _step(_model(params, dims, dev), nodes, ea, ei, target, dev)
    for k, p in m.named_parameters():
        assert torch.equal(p.grad, g2[k]), k


DEFAULT_CONV = dict(flow="source_to_target", concat=("i", "j", "e"), node_concat=("h", "agg"))
OTHER_CONV = dict(flow="target_to_source", concat=("e", "j", "i"), node_concat=("agg", "h"))


def _block_forward(p, h_t, e_t, idx, conv, mlp):
    """One InteractionNetwork block wired from `mlp` (torch_epd.mlp's signature after the parameters) in the given convention."""
    nl = (len([k for k in p if k.startswith("phi_edge.")]) - 4) // 2
    j, i = (idx[0], idx[1]) if conv["flow"] == "source_to_target" else (idx[1], idx[0])
    parts = {"i": h_t[i], "j": h_t[j], "e": e_t}
    e_new = mlp(p, "phi_edge", torch.cat([parts[c] for c in conv["concat"]], dim=1), nl, True)
    nparts = {"h": h_t, "agg": torch.zeros_like(h_t).index_add_(0, i, e_new)}
    h_new = mlp(p, "phi_node", torch.cat([nparts[c] for c in conv["node_concat"]], dim=1), nl, True)
    return h_new, e_new


def _block_leaves(params, h, e, dtype):
    p = {k[len("processor.0."):]: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in params.items() if k.startswith("processor.0.")}
    return p, torch.tensor(h, dtype=dtype, requires_grad=True), torch.tensor(e, dtype=dtype, requires_grad=True)


def _block_reference(params, h, e, ei, wh, we, conv, dtype):
    """The block (processor.0) through torch_epd.mlp in `dtype` on the CPU, with the cotangents wh / we on its two outputs:
    {"dh_in", "de_in", parameter name within the block: gradient}."""
    p, h_t, e_t = _block_leaves(params, h, e, dtype)
    h_new, e_new = _block_forward(p, h_t, e_t, torch.tensor(ei, dtype=torch.int64), conv, torch_epd.mlp)
    ((h_new * torch.tensor(wh, dtype=dtype)).sum() + (e_new * torch.tensor(we, dtype=dtype)).sum()).backward()
    return dict({k: v.grad.numpy() for k, v in p.items()}, dh_in=h_t.grad.numpy(), de_in=e_t.grad.numpy())


def _block_flip_allowance(params, h, e, ei, wh, we, conv, tau=1e-5, max_units=256):
    """torch_epd.relu_flip_allowance restated for one block and its two inputs, with the same tau and the same cap: per tensor,
    the largest change that toggling the ReLU derivative of the hidden units whose float64 pre-activation lies within tau x rms
    of zero explains (absolute values summed over those units) -- element by element, so a row of de_in that no such unit
    touches gets none.  Returns ({name: allowance array}, number of units)."""
    dtype = torch.float64
    p, h_t, e_t = _block_leaves(params, h, e, dtype)
    tape = []
    h_new, e_new = _block_forward(p, h_t, e_t, torch.tensor(ei, dtype=torch.int64), conv,
                                  lambda pp, prefix, x, nl, norm: torch_epd._mlp_taped(pp, prefix, x, nl, norm, tape))
    ((h_new * torch.tensor(wh, dtype=dtype)).sum() + (e_new * torch.tensor(we, dtype=dtype)).sum()).backward(retain_graph=True)
    units = torch_epd.near_zero_units(tape, tau, max_units)
    leaves = dict(p, dh_in=h_t, de_in=e_t)
    bounds = torch_epd.flip_bounds(tape, units, list(leaves.values()))
    return {k: v.numpy() for k, v in zip(leaves, bounds)}, len(units)


def _block_step(blk, h, e, ei, wh, we, dev):
    """The standalone block under autograd with h and e requiring grad: the same dictionary as device tensors."""
    blk.zero_grad(set_to_none=True)
    x = _t(h, dev).requires_grad_(True)
    a = _t(e, dev).requires_grad_(True)
    h_new, e_new, _ = blk(x, a, _t(ei, dev))
    ((h_new * _t(wh, dev)).sum() + (e_new * _t(we, dev)).sum()).backward()
    return dict({k: p.grad.detach().clone() for k, p in blk.named_parameters()}, dh_in=x.grad.detach().clone(), de_in=a.grad.detach().clone())


def _assert_within(case, got, ref64, ref32, allowance):
    """Every tensor of `got` within the rule of float64; one beyond it is allowed only what `allowance()` (the relu-flip bound of the
    same inputs, per element, computed when needed) adds."""
    assert sorted(got) == sorted(ref64)
    yardstick.compare({k: v.cpu().numpy() for k, v in got.items()}, ref64, ref32, allowance, tag="[regimes]", what=case)


@pytest.mark.parametrize("hidden,conv,seed", [(128, DEFAULT_CONV, 170), (64, DEFAULT_CONV, 171), (256, DEFAULT_CONV, 172), (128, OTHER_CONV, 173)])
def test_hub_graph_standalone_interaction_network(dev, hidden, conv, seed):
    """InteractionNetwork alone with both inputs requiring grad and random cotangents on both outputs (as
    test_graph_independent_input_gradients): dh_in, de_in and the block's parameter gradients against float64 autograd.  de_in
    is compared row for row in the caller's edge order, which the destination sort must undo (rowidx / dyidx / dxidx).  With
    flow='target_to_source' the roles of the two edge_index rows swap, so the hub segments land on the other sum.
      * a random permutation of the edge columns leaves parameter gradients and dh_in within the yardstick, and gives the plain
        call's de_in rows, permuted, within the same bound (not the same bits: the order of additions in a segment changes);
      * the same call twice gives the same bits for every gradient."""
    from gnn_manip_amd import InteractionNetwork
    ei = _hub_graph()
    rng = np.random.Generator(np.random.PCG64(seed))
    h = rng.standard_normal((HUB_N, hidden)).astype(np.float32)
    e = rng.standard_normal((HUB_E, hidden)).astype(np.float32)
    wh = rng.standard_normal((HUB_N, hidden)).astype(np.float32)
    we = rng.standard_normal((HUB_E, hidden)).astype(np.float32)
    dims = (25, 4, 3, hidden, 2, 1)
    params = orc.init_params(*dims, seed)
    src = _model(params, dims, dev).processor[0]
    blk = InteractionNetwork(src.phi_edge, src.phi_node, **conv).to(dev)
    assert sorted(k for k, _ in blk.named_parameters()) == sorted(k[len("processor.0."):] for k in params if k.startswith("processor.0."))

    ref64 = _block_reference(params, h, e, ei, wh, we, conv, torch.float64)
    ref32 = _block_reference(params, h, e, ei, wh, we, conv, torch.float32)
    allowance = functools.lru_cache(maxsize=None)(lambda: _block_flip_allowance(params, h, e, ei, wh, we, conv))
    got = _block_step(blk, h, e, ei, wh, we, dev)
    what = f"hub graph, standalone block, hidden {hidden}, {conv['flow']}"
    _assert_within(what, got, ref64, ref32, allowance)

    # the same call again: identical bits
    again = _block_step(blk, h, e, ei, wh, we, dev)
    for k in got:
        assert torch.equal(got[k], again[k]), k

    # edge order is immaterial
    perm = rng.permutation(HUB_E)
    ei_p, e_p, we_p = np.ascontiguousarray(ei[:, perm]), e[perm], we[perm]
    ref64_p = _block_reference(params, h, e_p, ei_p, wh, we_p, conv, torch.float64)
    ref32_p = _block_reference(params, h, e_p, ei_p, wh, we_p, conv, torch.float32)
    got_p = _block_step(blk, h, e_p, ei_p, wh, we_p, dev)
    _assert_within(what + ", edges permuted", got_p, ref64_p, ref32_p,
                   functools.lru_cache(maxsize=None)(lambda: _block_flip_allowance(params, h, e_p, ei_p, wh, we_p, conv)))
    err = np.abs(got_p["de_in"].cpu().numpy() - got["de_in"].cpu().numpy()[perm])
    tol, scale, _ = yardstick.tolerance(ref64["de_in"], ref32["de_in"])
    tol_p, scale_p, _ = yardstick.tolerance(ref64_p["de_in"], ref32_p["de_in"])
    bound = min(tol * scale, tol_p * scale_p)
    print(f"[regimes] {what}: de_in of the permuted call against de_in[perm]: err/tol {err.max() / bound:.3f}")
    if err.max() > bound:     # two evaluations may disagree on the sign of the same near-zero units (the same set in either edge order)
        assert (err <= bound + allowance()[0]["de_in"][perm]).all(), (float(err.max()), bound)
