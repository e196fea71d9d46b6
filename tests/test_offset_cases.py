"""The tiled-copy helper of tests/offset_cases.py on the CPU: a tiling is what it claims to be (the oracle on the tiled graph equals
the class references, the assembled gradients equal float64 autograd on the tiled graph), the wrap-safety and regime assertions
reject cases built wrong, and every case of tests/test_gpu_offsets.py is in the regime it exists for."""
import numpy as np
import pytest
import torch

import offset_cases as oc
import yardstick
from oracle import epd_oracle as orc
from oracle import torch_epd

DIMS = (25, 4, 3, 32, 2, 1)   # a narrow model: the tiling is what is under test here, not the width


@pytest.fixture(scope="module")
def params():
    return orc.init_params(*DIMS, 61)


@pytest.fixture(scope="module", params=["dense", "sparse"])
def fam(request):
    return oc.dense_family() if request.param == "dense" else oc.sparse_family()


def test_families_are_wrap_safe_and_as_described():
    d, s = oc.dense_family(), oc.sparse_family()
    assert d.node_period == s.node_period == 5 * 1021 and d.node_period % 2 == 1
    assert d.edge_period % 2 == 1 and s.edge_period % 2 == 1
    assert 100_000 < d.edge_period < 104_000 and all(20_000 < e < 20_800 for e in d.e0)
    mean_in, isolated, send_only = s.degrees()
    assert 1.0 <= mean_in <= 2.0 and isolated > 0 and send_only > 0
    assert d.degrees()[1] == 0   # the dense family keeps every self edge


@pytest.mark.parametrize("t", [3, 7])
def test_device_tiling_is_the_copy_by_copy_layout(fam, t):
    """tile_device (torch operations, here on the CPU device) against the plain concatenation."""
    nodes, ea, ei = oc.tile_host(fam, t)
    dn, da, di = oc.tile_device(fam, t, torch.device("cpu"))
    assert (nodes.shape[0], ei.shape[1]) == fam.sizes(t)
    np.testing.assert_array_equal(dn.numpy(), nodes)
    np.testing.assert_array_equal(da.numpy(), ea)
    np.testing.assert_array_equal(di.numpy(), ei)
    assert di.dtype == torch.int64 and di.is_contiguous()
    for c in range(t):   # block-diagonal: copy c's edges stay inside its rows
        lo = sum(fam.e0[i % oc.K] for i in range(c))
        blk = ei[:, lo:lo + fam.e0[c % oc.K]]
        assert blk.size == 0 or (blk.min() >= c * fam.n0 and blk.max() < (c + 1) * fam.n0)


@pytest.mark.parametrize("t", [3, 7])
def test_tiled_forward_and_gradients_are_the_class_references(fam, params, t):
    nl, ms = DIMS[4], DIMS[5]
    targets = oc.class_targets(fam)
    refs = oc.class_grad_refs(fam, params, targets, nl, ms, inputs=True)
    nodes, ea, ei = oc.tile_host(fam, t)
    target = np.concatenate([targets[i % oc.K] for i in range(t)])
    # float64 autograd on the whole tiled graph
    p = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    x = torch.tensor(nodes, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(ea, dtype=torch.float64, requires_grad=True)
    out = torch_epd.epd_forward(p, x, a, torch.tensor(ei), nl, ms)
    loss = torch.nn.functional.l1_loss(out, torch.tensor(target, dtype=torch.float64), reduction="sum") / out.shape[0]
    loss.backward()
    # forward: every copy is its class's reference (the same float64 arithmetic row by row: to the last few bits)
    fr = [torch.tensor(r["out"]) for r in refs]
    assert max(oc.worst_copy_error(out.detach(), fr, fam, t)) <= 1e-12
    assert abs(float(loss.detach()) - oc.assemble_loss(refs, t)) <= 1e-12 * abs(float(loss.detach()))
    # parameter gradients: the multiplicity-weighted sum
    g = oc.assemble_param_grads(refs, t)
    for name, v in p.items():
        scale = max(float(v.grad.abs().max()), 1e-30)
        assert np.abs(v.grad.numpy() - g[name]).max() <= 1e-11 * scale, name
    # input gradients: copy t's are its class's, scaled by n0 / N
    s = oc.input_grad_scale(t)
    dn = [torch.tensor(r["d_nodes"]) * s for r in refs]
    de = [torch.tensor(r["d_edge_attr"]) * s for r in refs]
    assert max(oc.worst_copy_error(x.grad, dn, fam, t)) <= 1e-12 * float(x.grad.abs().max())
    assert oc.edge_rows_error(a.grad, de, fam, t) <= 1e-12 * max(float(a.grad.abs().max()), 1e-30)
    # ... and a comparison against the wrong class does fail: the classes differ
    assert oc.worst_copy_error(out.detach(), fr[1:] + fr[:1], fam, t)[0] > 1e-3
    # the float32 yardstick assembles the same way
    refs32 = oc.class_grad_refs(fam, params, targets, nl, ms, dtype=torch.float32)
    g32 = oc.assemble_param_grads(refs32, t)
    worst, _ = yardstick.compare({k: v.grad.numpy() for k, v in p.items()}, g, g32, tag="[offsets]")
    assert worst[1] < 1e-6


def test_compare_gradients_rejects_a_wrong_tensor(params):
    fam = oc.sparse_family()
    targets = oc.class_targets(fam)
    refs = oc.class_grad_refs(fam, params, targets, DIMS[4], DIMS[5])
    g = oc.assemble_param_grads(refs, 6)
    g32 = {k: v.astype(np.float32).astype(np.float64) for k, v in g.items()}
    bad = {k: v.copy() for k, v in g.items()}
    name = "processor.0.phi_edge.0.weight"
    bad[name][3, 5] += 1e-3 * np.abs(g[name]).max()
    with pytest.raises(AssertionError):
        yardstick.compare(bad, g, g32, tag="[offsets]")
    with pytest.raises(AssertionError):
        yardstick.compare(bad, g, g32, allowance=lambda: ({k: 0.0 for k in g}, None), tag="[offsets]")


def test_wrap_safety_rejects_an_even_node_period():
    """n0 = 1024: an address that wraps by 2^k rows would land on the same row of another copy."""
    d = oc.dense_family()
    bad = oc.Family("n0_1024", [np.pad(x, ((0, 3), (0, 0))) for x in d.nodes[:4]] + [np.pad(d.nodes[4], ((0, 3), (0, 0)))],
                    d.edge_attr, d.edge_index, n0=1024)
    assert bad.edge_period % 2 == 1
    with pytest.raises(AssertionError, match="node period must be odd"):
        bad.check()
    with pytest.raises(AssertionError, match="node period must be odd"):
        oc.make_case("bad", bad, 7, 128, edge_rows="<2GiB").check()


def test_wrap_safety_rejects_an_even_edge_period():
    d = oc.dense_family()
    ea, ei = list(d.edge_attr), list(d.edge_index)
    ea[2], ei[2] = ea[2][:-1], ei[2][:, :-1]
    bad = oc.Family("even_edges", d.nodes, ea, ei)
    assert bad.edge_period % 2 == 0
    with pytest.raises(AssertionError, match="edge period must be odd"):
        bad.check()


def test_regime_check_rejects_a_case_outside_its_regime():
    d = oc.dense_family()
    small = oc.make_case("too_small", d, 50, 256, edge_rows="[2,4)GiB")
    assert small.regime["edge_rows"] == "<2GiB"
    with pytest.raises(AssertionError, match="edge_rows"):
        small.check()
    with pytest.raises(AssertionError):   # a case that names nothing it is there for
        oc.make_case("no_regime", d, 50, 256).check()
    route = oc.make_case("wrong_route", oc.sparse_family(), 4109, 128, edge_sys_fits=True)
    with pytest.raises(AssertionError, match="edge_sys_fits"):
        route.check()


def test_restated_guards_at_their_boundaries():
    # P table: n * 2 * 128 * 4 < 2^32  <=>  n < 2^22
    assert oc.edge_sys_fits(1 << 20, 1 << 20) and not oc.edge_sys_fits(1 << 22, 0)
    # agg + side buffer: binds first on a sparse graph (one side-buffer row per node in the worst case)
    n, e = oc.sparse_family().sizes(4108)
    assert n * 2 * 128 * 4 < oc.GIB4 and (n + oc.edge_groups_max(n, e)) * 128 * 4 >= oc.GIB4 and not oc.edge_sys_fits(n, e)
    assert oc.wgrad_guard_ok(4_194_303, 256) and not oc.wgrad_guard_ok(4_194_304, 256)
    assert oc.side_of(oc.GIB2 - 1) == "<2GiB" and oc.side_of(oc.GIB2) == "[2,4)GiB" and oc.side_of(oc.GIB4) == ">=4GiB"


def test_every_gpu_case_is_in_its_regime():
    """The table of tests/test_gpu_offsets.py, checked here too: a case that drifts out of its regime fails without a GPU."""
    cases = oc.gpu_cases()
    assert set(cases) == {"F1", "F1s2", "F2", "F2c", "F3", "F3s2", "F4", "F5", "F5b", "F6", "B1", "T0", "T1", "T2", "T2g", "T1g", "R1"}
    for c in cases.values():
        c.check()
        print(c.describe())
    # F5 is the LAST tiling the systolic route takes, F5b / F6 lie beyond it on the two clauses of edge_sys_fits
    s = oc.sparse_family()
    t5 = cases["F5"].copies
    assert oc.edge_sys_fits(*s.sizes(t5)) and not oc.edge_sys_fits(*s.sizes(t5 + 1))
    assert cases["F5b"].copies == 4108 and cases["F6"].copies == 4109
    assert cases["F5b"].regime["bytes"]["p_table"] < oc.GIB4 <= cases["F6"].regime["bytes"]["p_table"]
    # T1 just under, T2 / T2g at the 4 GiB of edge rows the indexed weight-gradient operand is guarded at
    assert cases["T1"].regime["e"] < 4_194_304 <= cases["T2"].regime["e"]
    assert cases["T1"].regime["bytes"]["edge_rows"] > 0.98 * oc.GIB4
