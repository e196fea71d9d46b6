"""The library's training step on the MI355X (csrc/train_step.hip, gnn_manip_amd/train.py): gm_l1_loss, gm_train_step and the
Trainer around them against the numpy restatements of tests/train_step_cases.py -- bit for bit -- and against the existing path
(model.forward under autograd -> l1_loss / N -> backward), whose parameter gradients the library step must reproduce bit for bit.

Bounds.  Gradients, weights and moments: bit equality.  A loss: 1e-12 relative against the float64 numpy sum of the same float32
differences (two float64 summation orders of at most 150 000 terms).  Five steps against the float64 oracle/torch_epd.py +
torch.optim.Adam loop: 1e-3, per tensor against the tensor's largest element (the norm of tests/yardstick.py and of the 20-step
table this arithmetic was chosen by): an element-wise relative bound has no meaning for parameters that start at exactly zero
(the LayerNorm betas) and move by +-lr per step on the sign of their gradient.  The per-step losses are held to 1e-3 each, the bar
tests/test_gpu_train.py holds five Adam steps to.

Every test ends by reading the trainer's record and checking status()."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
from oracle import torch_epd
from gpu_support import dev, load_model, to_dev
from yardstick import same_bits
import train_step_cases as sc

pytestmark = pytest.mark.gpu

LR = 1e-3


def _setup(name, seed, dev, **kw):
    """(trainer, module, (x, edge_attr, edge_index, y) on the device, the numpy batch, the oracle's parameters)."""
    from gnn_manip_amd import Trainer
    dims = sc.STEP_MODELS[name]
    params = orc.init_params(*dims, seed)
    m = load_model(params, dims, dev)
    nodes, ea, ei = sc.scene_graph(seed)
    target = sc.step_target(nodes, dims[2], seed)
    batch = tuple(to_dev(a, dev) for a in (nodes, ea, ei, target))
    return Trainer(m, lr=LR, **kw), m, batch, (nodes, ea, ei, target), params


def _existing_path(m, batch, mask_col=-1):
    """train_dyn.py:49-66 on the module: (prediction, [p.grad]) of the L1 loss, plain or over the sand rows."""
    x, ea, ei, y = batch
    m.zero_grad()
    out = m.forward(x, ea, ei)
    crit = torch.nn.L1Loss(reduction="sum")
    if mask_col >= 0:
        sand = x[:, mask_col] < 0.5
        loss = crit(out[sand], y[sand]) / y[sand].shape[0]
    else:
        loss = crit(out, y) / out.shape[0]
    loss.backward()
    return out.detach(), [p.grad.detach().clone() for p in m.parameters()]


def _finish(t, applied=None, skipped=0):
    rec = t.record()
    t.status()
    if applied is not None:
        assert (rec["steps_applied"], rec["steps_skipped"]) == (applied, skipped), rec
    return rec


def _state(t):
    from gnn_manip_amd import train
    return [t.export(w) for w in (train.PARAMS, train.EXP_AVG, train.EXP_AVG_SQ)]


def _assert_same_state(a, b, what):
    for kind, ta, tb in zip(("weights", "exp_avg", "exp_avg_sq"), a, b):
        for i, (u, v) in enumerate(zip(ta, tb)):
            assert same_bits(u, v), (what, kind, i)


# ------------------------------------------------------------------------------------------ gm_l1_loss alone
@pytest.mark.parametrize("n", sc.LOSS_ROWS)
def test_l1_loss_is_the_restatement(dev, n):
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    for od in sc.LOSS_OUT_DIMS:
        for mask in sc.LOSS_MASKS:
            pred, target, nodes, col = sc.loss_case(n, od, mask)
            want_loss, want_count, want_grad = sc.l1_restated(pred, target, nodes, col)
            p, t, x = to_dev(pred, dev), to_dev(target, dev), to_dev(nodes, dev)
            need = L.gm_l1_loss_workspace_bytes(n, od)
            runs = []
            for _ in range(2):
                ws = torch.full((need // 4 + 1,), float("nan"), device=dev).view(torch.uint8)
                loss = torch.full((1,), 7.0, dtype=torch.float64, device=dev)
                rows = torch.full((1,), -1, dtype=torch.int64, device=dev)
                grad = torch.full_like(p, float("nan"))
                check(L.gm_l1_loss(ptr(p), ptr(t), n, od, ptr(x) if col >= 0 else None, sc.LOSS_NODE_DIM, col, ptr(loss), ptr(rows), ptr(grad),
                                   ptr(ws), need, current_stream(dev)))
                runs.append((loss.cpu().numpy(), int(rows), grad.cpu().numpy()))
            (l0, r0, g0), (l1, r1, g1) = runs
            what = (n, od, mask)
            assert l0.view(np.uint64) == l1.view(np.uint64) and r0 == r1 and same_bits(g0, g1), what      # a run repeats itself
            assert r0 == want_count and same_bits(g0, want_grad), what
            if want_count == 0:
                assert np.isnan(l0[0]) and not g0.any(), what
            else:
                assert abs(l0[0] - want_loss) <= 1e-12 * abs(want_loss), (what, l0[0], want_loss)
            # without the optional outputs: the same loss
            loss2 = torch.zeros(1, dtype=torch.float64, device=dev)
            ws = torch.full((need // 4 + 1,), float("nan"), device=dev).view(torch.uint8)
            check(L.gm_l1_loss(ptr(p), ptr(t), n, od, ptr(x), sc.LOSS_NODE_DIM, col, ptr(loss2), None, None, ptr(ws), need, current_stream(dev)))
            assert loss2.cpu().numpy().view(np.uint64) == l0.view(np.uint64), what
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ one step
@pytest.mark.parametrize("name,sand_only", [("h64", False), ("h64", True), ("h128", False), ("h256", True), ("h64_out4", False),
                                            ("h256_m3", False)])       # adam_flat_kernel<false> past one pass of its grid
def test_one_step_has_the_existing_paths_gradients(dev, name, sand_only):
    from gnn_manip_amd import train
    t, m, batch, (nodes, _, _, target), _ = _setup(name, 301, dev, sand_only=sand_only, material_col=sc.MATERIAL_COL if sand_only else None)
    assert t.mask_col == (21 if sand_only else -1)
    if sand_only:
        assert 0 < (nodes[:, 21] < 0.5).sum() < len(nodes)
    out, grads = _existing_path(m, batch, t.mask_col)
    w0 = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    t.step(*batch)
    got = t.export(train.GRADS)
    for i, (g, want) in enumerate(zip(got, grads)):
        assert same_bits(g, want), (name, "gradient", i, float((g - want).abs().max()))
    assert any(float(g.abs().max()) > 0 for g in got)
    want_loss = sc.l1_restated(out.cpu().numpy(), target, nodes, t.mask_col)[0]
    assert abs(float(t.last_loss) - want_loss) <= 1e-12 * abs(want_loss)
    # ... and the update is the restatement's on them
    state = sc.adam_state(w0)
    w1 = sc.adam_restated(w0, [g.cpu().numpy() for g in grads], state, LR)
    _assert_same_state(_state(t), (w1, state["m"], state["v"]), name)
    assert sum(int(np.prod(s)) for s in sc.tensor_shapes(sc.STEP_MODELS[name])) <= sc.flat_count(sc.STEP_MODELS[name])
    rec = _finish(t, applied=1)
    assert (rec["beta1_pow"], rec["beta2_pow"]) == (0.9, 0.999)


# ------------------------------------------------------------------------------------------ five steps
def _float64_loop(params, dims, nodes, ea, ei, target, mask_col, steps):
    """The float64 oracle with torch.optim.Adam: (per-step losses, final parameters)."""
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in params.items()}
    opt = torch.optim.Adam(list(p64.values()), lr=LR)
    x, a, i, y = (torch.tensor(nodes, dtype=torch.float64), torch.tensor(ea, dtype=torch.float64), torch.tensor(ei, dtype=torch.int64),
                  torch.tensor(target, dtype=torch.float64))
    sand = torch.tensor(nodes[:, mask_col] < 0.5) if mask_col >= 0 else torch.ones(len(nodes), dtype=torch.bool)
    losses = []
    for _ in range(steps):
        o = torch_epd.epd_forward(p64, x, a, i, dims[4], dims[5])
        l = torch.nn.functional.l1_loss(o[sand], y[sand], reduction="sum") / int(sand.sum())
        opt.zero_grad()
        l.backward()
        opt.step()
        losses.append(float(l.detach()))
    return losses, {k: v.detach().numpy() for k, v in p64.items()}


@pytest.mark.parametrize("name,sand_only", [("h64", True), ("h64_out4", False)])
def test_five_steps_are_the_restatement_bit_for_bit(dev, name, sand_only):
    """With (h64: out_dim 3) and without (h64_out4) a scalar tail of the flat Adam launch."""
    dims = sc.STEP_MODELS[name]
    assert (sc.flat_count(dims) % 4 != 0) == (name == "h64")
    t, m, batch, (nodes, ea, ei, target), params = _setup(name, 302, dev, sand_only=sand_only, material_col=sc.MATERIAL_COL if sand_only else None)
    w = [p.detach().cpu().numpy().copy() for p in m.parameters()]
    state = sc.adam_state(w)
    losses = torch.full((5,), float("nan"), dtype=torch.float64, device=dev)
    want_losses = []
    for k in range(5):
        out, grads = _existing_path(m, batch, t.mask_col)              # on the trainer's current weights (sync_module below)
        w = sc.adam_restated(w, [g.cpu().numpy() for g in grads], state, LR)
        want_losses.append(sc.l1_restated(out.cpu().numpy(), target, nodes, t.mask_col)[0])
        t.step(*batch, loss_out=losses[k:k + 1])
        _assert_same_state(_state(t), (w, state["m"], state["v"]), (name, "step", k))
        t.sync_module()
    got_losses = losses.cpu().numpy()
    np.testing.assert_allclose(got_losses, want_losses, rtol=1e-12, atol=0)
    rec = _finish(t, applied=5)
    assert (rec["beta1_pow"], rec["beta2_pow"]) == (state["b1p"], state["b2p"])
    # against float64 end to end
    ref_losses, ref = _float64_loop(params, dims, nodes, ea, ei, target, t.mask_col, 5)
    print(f"\n[train step] {name}: losses {got_losses} float64 {ref_losses}")
    assert ref_losses[-1] < ref_losses[0]
    np.testing.assert_allclose(got_losses, ref_losses, rtol=1e-3)
    worst = ("", 0.0)
    for key, g in zip([k for k, _ in m.named_parameters()], w):
        r = ref[key]
        err = float(np.abs(g.astype(np.float64) - r).max() / np.abs(r).max())
        worst = max(worst, (key, err), key=lambda kv: kv[1])
    print(f"[train step] {name}: worst tensor against float64 after five steps: {worst[0]} {worst[1]:.3e} of its maximum")
    assert worst[1] <= 1e-3, worst


# ------------------------------------------------------------------------------------------ skipped steps
@pytest.mark.parametrize("how", ["edge_index", "nan_target"])
def test_a_bad_batch_is_skipped_and_leaves_no_trace(dev, how):
    from gnn_manip_amd._lib import GMError
    t, m, batch, _, _ = _setup("h64", 303, dev)
    twin, _, _, _, _ = _setup("h64", 303, dev)
    x, ea, ei, y = batch
    y2 = torch.roll(y, 1, 0).contiguous()                               # a second good batch
    t.step(x, ea, ei, y)
    twin.step(x, ea, ei, y)
    before, rec0 = _state(t), t.record()
    if how == "edge_index":
        bad_ei = ei.clone()
        bad_ei[1, 17] = x.shape[0]                                      # one entry out of range
        bad = (x, ea, bad_ei, y)
    else:
        bad_y = y.clone()
        bad_y[5, 1] = float("nan")
        bad = (x, ea, ei, bad_y)
    slot = torch.zeros(1, dtype=torch.float64, device=dev)
    t.step(*bad, loss_out=slot)
    assert np.isnan(float(slot))
    _assert_same_state(_state(t), before, how)
    rec1 = t.record()
    assert rec1 == dict(rec0, steps_skipped=rec0["steps_skipped"] + 1), (rec0, rec1)
    if how == "edge_index":                                             # the flag still surfaces through the tape header
        with pytest.raises(GMError, match="edge_index"):
            t.status()
    t.step(x, ea, ei, y2)
    twin.step(x, ea, ei, y2)
    _assert_same_state(_state(t), _state(twin), (how, "the next good step"))
    assert float(t.last_loss) == float(twin.last_loss)
    _finish(twin, applied=2)
    _finish(t, applied=2, skipped=1)


# ------------------------------------------------------------------------------------------ after training
def test_trained_weights_reach_the_module_and_the_inference_path(dev):
    from gnn_manip_amd import EncProcDecGNN, train
    t, m, batch, (nodes, _, _, target), _ = _setup("h64", 304, dev)
    x, ea, ei, y = batch
    with torch.no_grad():
        stale = m.forward(x, ea, ei).clone()
    t.evaluate(*batch)
    want = sc.l1_restated(stale.cpu().numpy(), target)[0]               # the trainer's own model, inference images, before a step
    assert abs(float(t.last_loss) - want) <= 1e-12 * want
    for _ in range(3):
        t.step(*batch)
    t.sync_module()
    with torch.no_grad():
        out = m.forward(x, ea, ei)
    fresh = EncProcDecGNN(*sc.SMALL).to(dev)
    with torch.no_grad():
        for p, w in zip(fresh.parameters(), t.export(train.PARAMS)):
            p.copy_(w)
        out_fresh = fresh.forward(x, ea, ei)
    assert same_bits(out, out_fresh) and not same_bits(out, stale)
    t.evaluate(*batch)                                                  # the trainer's inference images re-packed after the steps
    want = sc.l1_restated(out.cpu().numpy(), target)[0]
    assert abs(float(t.last_loss) - want) <= 1e-12 * want
    assert float(t.last_loss) < sc.l1_restated(stale.cpu().numpy(), target)[0]       # and training did lower the loss
    fresh.status()
    _finish(t, applied=3)


# ------------------------------------------------------------------------------------------ checkpoints
def test_checkpoint_round_trip(dev):
    from gnn_manip_amd import Trainer
    t, m, batch, _, _ = _setup("h64", 305, dev, betas=(0.8, 0.99), eps=1e-7)
    for _ in range(2):
        t.step(*batch)
    sd = t.state_dict()
    t.sync_module()                                                     # the module now holds the checkpoint's weights
    opt = torch.optim.Adam(m.parameters(), lr=0.5)
    opt.load_state_dict(sd)                                             # train_dyn.py:33-37 with a torch optimiser
    assert opt.param_groups[0]["lr"] == LR and tuple(opt.param_groups[0]["betas"]) == (0.8, 0.99)
    assert all(float(opt.state[p]["step"]) == 2 for p in m.parameters())
    resumed = Trainer(m, lr=0.5, betas=(0.8, 0.99), eps=1e-7)
    resumed.load_state_dict(opt.state_dict())                           # ... and back
    assert resumed.lr == LR
    _assert_same_state(_state(resumed), _state(t), "after the import")
    assert resumed.record() == dict(t.record(), steps_skipped=0)
    t.step(*batch)
    resumed.step(*batch)
    _assert_same_state(_state(resumed), _state(t), "one step after the import")
    assert float(resumed.last_loss) == float(t.last_loss)
    with pytest.raises(ValueError, match="betas"):
        Trainer(m).load_state_dict(sd)
    _finish(resumed, applied=3)
    _finish(t, applied=3)


# ------------------------------------------------------------------------------------------ refusals that need a trainer
def test_step_export_and_import_refuse_their_arguments(dev):
    from gnn_manip_amd._lib import current_stream, lib, ptr
    t, m, batch, _, _ = _setup("h64", 306, dev)
    x, ea, ei, y = batch
    L = lib()
    err = lambda: L.gm_last_error().decode()
    n, e = x.shape[0], ea.shape[0]
    need = L.gm_train_step_workspace_bytes(C.byref(t.desc), n, e)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    s = current_stream(dev)
    step = lambda mask_col=-1, ws_bytes=need, nodes=x: L.gm_train_step(t._h, ptr(nodes), n, ptr(ea), ptr(ei), e, ptr(y), mask_col, LR, None, ptr(ws),
                                                                        ws_bytes, s)
    assert step(ws_bytes=need - 1) == -4 and err() == "gm_train_step: workspace %d < %d" % (need - 1, need)
    assert step(mask_col=25) == -1 and err() == "gm_train_step: mask_col=25 outside the 25 node columns"
    assert step(nodes=None) == -1 and err() == "gm_train_step: null pointer"
    tensors = t.export()
    arr = (C.c_void_p * len(tensors))(*[w.data_ptr() for w in tensors])
    for fn, extra in ((L.gm_trainer_export, ()), (L.gm_trainer_import, (0,))):
        name = "gm_trainer_export" if not extra else "gm_trainer_import"
        assert fn(t._h, 1, arr, len(tensors) - 1, *extra, s) == -1 and err() == "%s: expected %d tensors, got %d" % (name, len(tensors), len(tensors) - 1)
        for what in (0, 5, -1):
            assert fn(t._h, what, arr, len(tensors), *extra, s) == -1 and err() == "%s: unknown what=%d" % (name, what)
        assert fn(t._h, 1, None, len(tensors), *extra, s) == -1 and err() == "%s: null pointer" % name
    assert L.gm_trainer_import(t._h, 4, arr, len(tensors), 0, s) == -1 and err().startswith("gm_trainer_import: the gradients are an output")
    assert L.gm_trainer_import(t._h, 2, arr, len(tensors), -1, s) == -1 and err() == "gm_trainer_import: step_count=-1 out of range"
    _finish(t, applied=0)                                               # nothing above reached the device


# ------------------------------------------------------------------------------------------ an epoch
@pytest.fixture(scope="module")
def g9_root(golden, tmp_path_factory):
    """The synthetic recordings of tests/golden/g9_dataset.npz as a dataset directory."""
    g = golden("g9_dataset.npz")
    root = str(tmp_path_factory.mktemp("g9_train_step")) + "/"
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")
    return root


def test_fit_epoch_synchronises_once_and_is_step_by_step(dev, g9_root, monkeypatch):
    from gnn_manip_amd import CoffeeDataset, GraphLoader, Trainer
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=3e-4, device=dev, use_control=True)
    dims = (25, 4, 3, 64, 2, 2)
    params = orc.init_params(*dims, 307)
    loader = lambda: GraphLoader(ds, batch_size=2, seed=2, fused=True, prefetch=1)
    # batch by batch
    by_step = Trainer(load_model(params, dims, dev), lr=LR, sand_only=True, material_col=sc.MATERIAL_COL)
    slots = torch.zeros(len(loader()), dtype=torch.float64, device=dev)
    for i, batch in enumerate(loader()):
        by_step.step(batch, loss_out=slots[i:i + 1])
    want = slots.cpu().numpy()
    assert len(want) == 3 and np.isfinite(want).all()
    # fit_epoch, under the spies of test_loader_does_not_synchronise
    t = Trainer(load_model(params, dims, dev), lr=LR, sand_only=True, material_col=sc.MATERIAL_COL)
    epoch_loader = loader()
    calls = []

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(torch.cuda, "synchronize", spy("torch.cuda.synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("Stream.synchronize", torch.cuda.Stream.synchronize))
    got = t.fit_epoch(epoch_loader)
    assert calls == ["Stream.synchronize"], calls
    monkeypatch.undo()
    assert got.dtype == np.float64 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), (got, want)
    _assert_same_state(_state(t), _state(by_step), "fit_epoch against step by step")
    ev = t.eval_epoch(loader())
    assert ev.shape == (3,) and np.isfinite(ev).all()
    _assert_same_state(_state(t), _state(by_step), "eval_epoch changes nothing")
    _finish(by_step, applied=3)
    _finish(t, applied=3)
