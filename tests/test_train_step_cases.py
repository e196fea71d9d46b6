"""CPU: the numpy restatements of the library's training step (tests/train_step_cases.py) against torch, and the case table's own
regime -- what tests/test_gpu_train_step.py holds the kernels to, bit for bit, is checked here first.

Bounds.  The loss gradient: bit equality with what ``l1_loss(reduction='sum') / count`` back-propagates (counts below 2^24).  The
loss: 1e-12 relative against float64 numpy (two float64 summation orders of at most 15 000 terms differ by ~1e-14).  Adam: per
tensor, the restatement's error against float64 ``torch.optim.Adam`` is at most 4 x float32 ``torch.optim.Adam``'s own -- the
factor of tests/yardstick.py."""
import numpy as np
import pytest
import torch

import train_step_cases as sc
import yardstick


def test_table_sits_on_the_loss_kernels_edges():
    wg, cap = sc.LOSS_WG, sc.LOSS_GRID_MAX
    regimes = {n: sc.loss_regime(n) for n in sc.LOSS_ROWS}
    assert regimes[1] == (1, 1) and regimes[wg - 1] == (1, 1) and regimes[wg] == (1, 1)       # one partial workgroup, full or not
    assert regimes[wg + 1] == (2, 1) and regimes[300] == (2, 1)                                # a second, nearly empty workgroup
    big = max(sc.LOSS_ROWS)
    assert big > wg * cap and regimes[big] == (cap, 2)                                         # past one pass of the capped grid
    assert big % wg != 0 and (big - wg * cap) % wg != 0                                        # ... whose last workgroup is ragged
    assert {wg - 1, wg, wg + 1} <= set(sc.LOSS_ROWS)
    assert set(sc.LOSS_OUT_DIMS) == {2, 3}
    assert sc.LOSS_MASKS["middle"] not in (None, sc.LOSS_NODE_DIM - 1)                         # a mask column that is not the last


def test_loss_cases_hold_what_they_are_for():
    for n in sc.LOSS_ROWS:
        for od in sc.LOSS_OUT_DIMS:
            for mask in sc.LOSS_MASKS:
                pred, target, nodes, col = sc.loss_case(n, od, mask)
                loss, count, grad = sc.l1_restated(pred, target, nodes, col)
                if mask == "empty":
                    assert count == 0 and np.isnan(loss) and not grad.any()
                    continue
                assert count >= 1 and np.isfinite(loss)
                assert (pred == target).sum() == 1 and grad[n // 2, od - 1] == 0 and np.abs(grad[n // 2]).sum() > 0   # on a counted row
                if mask == "plain":
                    assert count == n and col == -1
                elif n > 1:
                    assert 0 < count < n and (grad[count_rows(nodes, col) == 0] == 0).all()


def count_rows(nodes, col):
    return (nodes[:, col] < 0.5).astype(np.int64)


@pytest.mark.parametrize("count", [7, 300, 5000])
@pytest.mark.parametrize("masked", [False, True])
def test_loss_restatement_is_torchs_gradient_bit_for_bit(count, masked):
    """Plain: every row counts.  Masked, as train_dyn.py:58-62 writes it: a boolean index on the material column, the sum over
    the selected rows divided by their number."""
    rng = np.random.default_rng(count)
    n = count if not masked else 2 * count + 3
    pred = rng.standard_normal((n, 3)).astype(np.float32)
    target = rng.standard_normal((n, 3)).astype(np.float32)
    nodes = rng.standard_normal((n, 25)).astype(np.float32)
    col = -1
    if masked:
        col = 25 + sc.MATERIAL_COL
        flag = np.ones(n, np.float32)
        flag[rng.permutation(n)[:count]] = 0.0
        nodes[:, col] = flag
    row = n // 2 if not masked else int(np.nonzero(nodes[:, col] < 0.5)[0][0])      # a counted row
    target[row, 1] = pred[row, 1]                                                    # one exactly equal element: sign 0
    loss, counted, grad = sc.l1_restated(pred, target, nodes, col)
    assert counted == count
    p = torch.tensor(pred, requires_grad=True)
    t, x = torch.tensor(target), torch.tensor(nodes)
    crit = torch.nn.L1Loss(reduction="sum")
    if masked:
        sand = x[:, sc.MATERIAL_COL] < 0.5
        l = crit(p[sand], t[sand]) / t[sand].shape[0]
    else:
        l = crit(p, t) / p.shape[0]
    l.backward()
    assert yardstick.same_bits(grad, p.grad)
    assert (grad == 0).sum() == (1 if not masked else 1 + 3 * (n - count))
    d64 = np.abs((pred - target).astype(np.float64))          # the float32 differences, summed in float64
    ref = d64.sum() / n if not masked else d64[nodes[:, col] < 0.5].sum() / count
    assert abs(loss - ref) <= 1e-12 * abs(ref)
    assert abs(loss - float(l.detach())) <= 1e-5 * abs(ref)   # torch's own float32 sum


def test_adam_restatement_against_float64_torch():
    grads, p0 = sc.adam_gradients()
    assert grads.shape == (20, 4099) and sc.ADAM_LR == 1e-3
    mag = np.abs(grads[grads != 0])
    assert mag.min() < 2e-6 and mag.max() > 5 and (grads == 0).all(axis=0).sum() >= 7 and (grads == 0).any(axis=0).sum() > 1000

    def torch_run(dtype):
        p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
        opt = torch.optim.Adam([p], lr=sc.ADAM_LR)
        for g in grads:
            p.grad = torch.tensor(g, dtype=dtype)
            opt.step()
        s = opt.state[p]
        return [a.detach().numpy().astype(np.float64) for a in (p, s["exp_avg"], s["exp_avg_sq"])]

    ref64, ref32 = torch_run(torch.float64), torch_run(torch.float32)
    state = sc.adam_state([p0])
    p = [p0]
    for g in grads:
        p = sc.adam_restated(p, [g], state, sc.ADAM_LR)
    assert state["steps"] == 20 and state["b1p"] == pytest.approx(0.9 ** 20, rel=1e-14)
    got = [p[0], state["m"][0], state["v"][0]]
    assert not (got[0][:7] != p0[:7]).any()                   # zero gradients from the start: the weight does not move
    for name, a, r64, r32 in zip(("weights", "exp_avg", "exp_avg_sq"), got, ref64, ref32):
        scale = np.abs(r64).max()
        err, e32 = np.abs(a.astype(np.float64) - r64).max() / scale, np.abs(r32 - r64).max() / scale
        print(f"\n[adam] {name}: err {err:.3e}, float32 torch {e32:.3e}, ratio {err / e32:.2f}")
        assert e32 > 0 and err <= 4.0 * e32, (name, err, e32)


def test_models_cover_a_flat_count_with_and_without_a_vector_tail():
    counts = {name: sc.flat_count(dims) for name, dims in sc.STEP_MODELS.items()}
    assert counts["h64"] % 4 == 3 and counts["h128"] % 4 == 3 and counts["h256"] % 4 == 3     # out_dim 3: a scalar tail of three
    assert counts["h64_out4"] % 4 == 0                                                          # none
    grid_pass = 2048 * 256 * 4                                                                  # floats of one pass of the flat Adam launch
    assert counts["h256_m3"] % 4 == 3 and counts["h256_m3"] > grid_pass > counts["h256"]        # a second trip of the grid-stride loop
    assert sc.flat_count((25, 4, 3, 128, 2, 10)) >= sum(int(np.prod(s)) for s in sc.tensor_shapes((25, 4, 3, 128, 2, 10)))
    from gnn_manip_amd import EncProcDecGNN
    for dims in sc.STEP_MODELS.values():
        assert [tuple(p.shape) for p in EncProcDecGNN(*dims).parameters()] == sc.tensor_shapes(dims)


def test_state_dict_layout_loads_into_torch_adam_and_back():
    from gnn_manip_amd.train import adam_state_dict, parse_adam_state_dict
    shapes = sc.tensor_shapes(sc.SMALL)
    rng = np.random.default_rng(3)
    m = [torch.tensor(rng.standard_normal(s).astype(np.float32)) for s in shapes]
    v = [torch.tensor(rng.random(s).astype(np.float32)) for s in shapes]
    sd = adam_state_dict(m, v, 17, 3e-4, (0.8, 0.99), 1e-7)
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes]
    opt = torch.optim.Adam(params, lr=1.0)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"]) == (3e-4, (0.8, 0.99), 1e-7)
    assert all(float(opt.state[p]["step"]) == 17 and torch.equal(opt.state[p]["exp_avg"], a) and torch.equal(opt.state[p]["exp_avg_sq"], b)
               for p, a, b in zip(params, m, v))
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()                                                 # a loaded optimiser steps: every hyper-parameter key is there
    m2, v2, step, group = parse_adam_state_dict(opt.state_dict(), shapes)
    assert step == 18 and group["lr"] == 3e-4 and len(m2) == len(v2) == len(shapes)
    assert parse_adam_state_dict(torch.optim.Adam(params).state_dict(), shapes)[:3] == (None, None, 0)     # never stepped
    with pytest.raises(ValueError, match="parameter group"):
        parse_adam_state_dict(opt.state_dict(), shapes[:-1])
    bad = opt.state_dict()
    bad["param_groups"][0]["weight_decay"] = 0.1
    with pytest.raises(ValueError, match="weight decay"):
        parse_adam_state_dict(bad, shapes)


def test_material_col_and_schedules():
    from gnn_manip_amd.train import normalise_material_col
    assert normalise_material_col(-1 - 3, 25) == 21 and normalise_material_col(-1, 22) == 21 and normalise_material_col(21, 25) == 21
    for bad in (25, -26):
        with pytest.raises(ValueError, match="material_col"):
            normalise_material_col(bad, 25)
    # the host formulas against torch's schedulers (train_dyn.py:100-107,143-144)
    p = [torch.nn.Parameter(torch.zeros(1))]
    opt = torch.optim.Adam(p, lr=1e-3)
    sched = torch.optim.swa_utils.SWALR(opt, anneal_strategy="linear", anneal_epochs=10, swa_lr=1e-4)
    for ep in range(1, 14):
        opt.step()
        sched.step()
        assert opt.param_groups[0]["lr"] == pytest.approx(sc.lr_linear(1e-3, 1e-4, ep, 10), rel=1e-12)
    opt = torch.optim.Adam(p, lr=1e-3)
    sched = torch.optim.lr_scheduler.ExponentialLR(opt, gamma=0.9)
    for ep in range(6):
        assert opt.param_groups[0]["lr"] == pytest.approx(sc.lr_exponential(1e-3, 0.9, ep, start=2), rel=1e-12)
        opt.step()
        if ep > 2:
            sched.step()
