"""Input gradients on the MI355X: EncProcDecGNN's d_nodes / d_edge_attr (gm_epd_backward_inputs), the backward kernels of the
per-step feature functions and the integrator, and RolloutEngine.differentiable_step, alone and unrolled into SamplesLoss.

Yardstick: the rule of tests/yardstick.py (`within`), the flip allowance per element; g64 the float64 reference (oracle/torch_epd.py
for the model, tests/grad_cases.py for the step, both checked on the CPU).  Losses are (out * w).sum() with seeded w.  Forward values: conftest.assert_forward_close (1e-5).  Every
figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

from conftest import STATS, assert_forward_close
from oracle import epd_oracle as orc
from oracle import torch_epd
import grad_cases as gc
import width_cases as wc
from gpu_support import cus as _cus, dev, graph_attr, load_model as _model, step_engine as _engine, tiles as _tiles, to_dev as _t
from grad_cases import L0, flip_allowance, split as _split, step_allowance as _step_allowance, step_reference as _step_reference
from sinkhorn_cases import sinkhorn_grad_ref
from train_cases import HUB_E, HUB_N, benchmark_graph as _benchmark_graph, graph as _graph, hub_graph as _hub_graph
from yardstick import lazy as _lazy, within as _within

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ the fused model
def _model_reference(params, nodes, ea, ei, w, num_layers, m_steps, dtype):
    p = {k: torch.tensor(v, dtype=dtype) for k, v in params.items()}
    x, a = gc.t64(nodes, True, dtype), gc.t64(ea, True, dtype)
    out = torch_epd.epd_forward(p, x, a, torch.tensor(ei, dtype=torch.int64), num_layers, m_steps)
    (out * gc.t64(w, dtype=dtype)).sum().backward()
    return out.detach().numpy(), x.grad.numpy(), a.grad.numpy()


def _run(m, nodes, ea, ei, w, dev, grad_inputs=True):
    x, a = _t(nodes, dev).requires_grad_(grad_inputs), _t(ea, dev).requires_grad_(grad_inputs)
    out = m.forward(x, a, _t(ei, dev))
    (out * _t(w, dev)).sum().backward()
    return out, x.grad, a.grad


def _check_inputs(what, params, dims, nodes, ea, ei, dev, seed, frozen=False, max_units=256):
    w = gc.weights((nodes.shape[0], dims[2]), seed)
    m = _model(params, dims, dev)
    if frozen:
        m.requires_grad_(False)
    out, dx, da = _run(m, nodes, ea, ei, w, dev)
    assert out.grad_fn is not None
    ref_out, rx, ra = _model_reference(params, nodes, ea, ei, w, dims[4], dims[5], torch.float64)
    _, x32, a32 = _model_reference(params, nodes, ea, ei, w, dims[4], dims[5], torch.float32)
    assert_forward_close(out.detach().cpu().numpy(), ref_out, floor=1e-3, what=what)

    def allowance():
        p = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
        x, a = gc.t64(nodes, True), gc.t64(ea, True)
        idx = torch.tensor(ei, dtype=torch.int64)
        return flip_allowance(lambda fwd: (fwd(p, x, a, idx, dims[4], dims[5]) * gc.t64(w)).sum(), [x, a], max_units=max_units)
    allowance = _lazy(allowance)
    _within(what + " d_nodes", dx.cpu().numpy(), rx, x32, lambda: (allowance()[0][0], allowance()[1]))
    if ea.shape[0]:
        _within(what + " d_edge_attr", da.cpu().numpy(), ra, a32, lambda: (allowance()[0][1], allowance()[1]))
    return m, w, dx, da


INPUT_CASES = [("default", (25, 4, 3, 128, 2, 2), 301), ("hidden 64", (25, 4, 3, 64, 2, 2), 302), ("hidden 256", (25, 4, 3, 256, 2, 2), 303),
               ("padded 96", (25, 4, 3, 96, 2, 2), 304), ("width 17 x 5", wc.WIDTHS["k_group_1_one_feature"][0] + (128, 2, 2), 305)]


@pytest.mark.parametrize("what,dims,seed", INPUT_CASES, ids=[c[0] for c in INPUT_CASES])
def test_fused_model_input_gradients(dev, what, dims, seed):
    """d_nodes / d_edge_attr against float64; the parameter gradients of the same run are bit-equal to those of a fresh model
    whose inputs do not require grad (gm_epd_backward): the input tail only adds stores."""
    params = orc.init_params(*dims, seed)
    _, _, ei = _graph(300, 0.06, seed)
    rng = np.random.default_rng(seed)
    if dims[:2] == (25, 4):
        nodes, ea, ei = _graph(300, 0.06, seed)
    else:
        nodes = rng.standard_normal((300, dims[0])).astype(np.float32)
        ea = rng.standard_normal((ei.shape[1], dims[1])).astype(np.float32)
    m, w, _, _ = _check_inputs(what, params, dims, nodes, ea, ei, dev, seed)
    m2 = _model(params, dims, dev)
    out2, dx2, _ = _run(m2, nodes, ea, ei, w, dev, grad_inputs=False)
    assert dx2 is None
    for (k, p), (_, p2) in zip(m.named_parameters(), m2.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, p2.grad), k


def test_frozen_model_still_carries_the_input_gradient(dev):
    """Every parameter requires_grad=False (a planning loop on a trained model): the output has a grad_fn and the input
    gradients are test 1's, bit for bit; no parameter gets a gradient."""
    what, dims, seed = INPUT_CASES[0]
    params = orc.init_params(*dims, seed)
    nodes, ea, ei = _graph(300, 0.06, seed)
    m, w, dx, da = _check_inputs("frozen", params, dims, nodes, ea, ei, dev, seed, frozen=True)
    assert all(p.grad is None for p in m.parameters())
    _, dx1, da1 = _run(_model(params, dims, dev), nodes, ea, ei, w, dev)
    assert torch.equal(dx, dx1) and torch.equal(da, da1)
    x = _t(nodes, dev).requires_grad_(True)                 # only one input requires grad
    out = m.forward(x, _t(ea, dev), _t(ei, dev))
    (out * _t(w, dev)).sum().backward()
    assert torch.equal(x.grad, dx)


@pytest.mark.parametrize("hidden,seed", [(128, 311), (64, 312)])
def test_hub_multigraph_in_random_edge_order(dev, hidden, seed):
    """Hubs, duplicates, self loops, isolated nodes, the columns in random order: d_edge_attr row for row in the caller's order
    (the destination sort's permutation undone by the indexed store)."""
    ei = _hub_graph()
    rng = np.random.Generator(np.random.PCG64(seed))
    nodes = rng.standard_normal((HUB_N, 25)).astype(np.float32)
    ea = rng.standard_normal((HUB_E, 4)).astype(np.float32)
    dims = (25, 4, 3, hidden, 2, 2)
    _check_inputs(f"hub graph hidden {hidden}", orc.init_params(*dims, seed), dims, nodes, ea, ei, dev, seed)


@pytest.mark.parametrize("n,with_edges", [(5, False), (1, True), (130, False)])
def test_degenerate_graphs(dev, n, with_edges):
    dims = (25, 4, 3, 128, 2, 2)
    nodes = np.random.default_rng(n).standard_normal((n, 25)).astype(np.float32)
    ei = np.stack((np.arange(n), np.arange(n))).astype(np.int64) if with_edges else np.zeros((2, 0), np.int64)
    ea = np.random.default_rng(n + 1).standard_normal((ei.shape[1], 4)).astype(np.float32)
    _, _, _, da = _check_inputs(f"n={n} e={ei.shape[1]}", orc.init_params(*dims, 99), dims, nodes, ea, ei, dev, 99)
    assert da.shape == (ei.shape[1], 4)


def test_benchmark_graph_walks_tiles_and_is_bit_stable(dev):
    """More edge tiles than two per CU: the indexed dx_in store runs across a workgroup's tile restarts.  Twice, same bits.
    About 5e7 hidden units see this graph, so some pre-activation always lies within float32 rounding of zero (plain PyTorch
    float32 is itself 2.5e-3 / 2.7e-2 of the maximum off on this input) and the flip allowance is what holds the one or two rows
    concerned.  Each unit of it costs a float64 backward over the whole graph: only the 24 units closest to zero are taken here
    (measured: d_nodes is 5.3 x the plain bound in one row, and 0.84 of bound + allowance from 16 units on) -- fewer units can
    only make the bound smaller."""
    nodes, ea, ei = _benchmark_graph()
    assert _tiles(ea.shape[0]) > 2 * _cus(dev), (ea.shape[0], _cus(dev))
    dims = (25, 4, 3, 128, 2, 1)
    params = orc.init_params(*dims, 321)
    _, w, dx, da = _check_inputs("benchmark graph", params, dims, nodes, ea, ei, dev, 321, max_units=24)
    _, dx2, da2 = _run(_model(params, dims, dev), nodes, ea, ei, w, dev)
    assert torch.equal(dx, dx2) and torch.equal(da, da2)


def test_flagged_edge_index_gives_zero_input_gradients(dev):
    from gnn_manip_amd import EncProcDecGNN
    from gnn_manip_amd._lib import GMError
    torch.manual_seed(3)
    n, e = 300, 4000
    m = EncProcDecGNN(25, 4, 3, 128, 2, 2).to(dev)
    x, ea = torch.randn(n, 25, device=dev).requires_grad_(), torch.randn(e, 4, device=dev).requires_grad_()
    bad = torch.randint(0, n, (2, e), device=dev)
    bad[1, 17] = n + 5
    out = m.forward(x, ea, bad)
    out.abs().sum().backward()
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    assert x.grad.shape == x.shape and float(x.grad.abs().max()) == 0.0
    assert ea.grad.shape == ea.shape and float(ea.grad.abs().max()) == 0.0
    assert all(float(p.grad.abs().max()) == 0.0 for p in m.parameters())
    with pytest.raises(GMError, match="out of range"):
        m.status()


# ------------------------------------------------------------------------------------------ the feature functions alone
def _edge_case(name):
    if name == "multigraph":
        return gc.multigraph()
    L = wc.LAYOUTS[name]
    obs = gc.state(name)
    return np.ascontiguousarray(obs[-1][:, L.cart:L.cart + 3]), gc.radius_edges(name)


@pytest.mark.parametrize("name", ["default", "moved", "multigraph"])
def test_edge_features_backward(dev, name):
    from gnn_manip_amd import get_edges_displacement
    pos, ei = _edge_case(name)
    w = gc.weights((ei.shape[1], 4), 41)
    s, r = _t(ei[0], dev), _t(ei[1], dev)
    refs = {}
    for dtype in (torch.float64, torch.float32):
        p = gc.t64(pos, True, dtype)
        out = gc.edge_features(p, torch.tensor(ei[0]), torch.tensor(ei[1]))
        (out * gc.t64(w, dtype=dtype)).sum().backward()
        refs[dtype] = (out.detach().numpy(), p.grad.numpy())
    got = []
    for stride in (3, 8, 3):     # dense rows, a stride-8 view (rows of a state), dense again: the same bits every time
        buf = torch.zeros((pos.shape[0], stride), device=dev)
        buf[:, :3] = _t(pos, dev)
        buf.requires_grad_(True)
        view = buf[:, :3]
        assert view.stride(0) == stride
        out = get_edges_displacement(view, s, r, gc.R)
        assert out.grad_fn is not None
        (out * _t(w, dev)).sum().backward()
        assert float(buf.grad[:, 3:].abs().max()) == 0.0 if stride > 3 else True
        got.append(buf.grad[:, :3].clone())
        assert torch.equal(out.detach(), get_edges_displacement(view.detach(), s, r, gc.R))     # the forward is the plain one
    assert_forward_close(out.detach().cpu().numpy(), refs[torch.float64][0], what=name)
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])
    _within(f"edge features {name}", got[0].cpu().numpy(), refs[torch.float64][1], refs[torch.float32][1])
    deg = np.bincount(ei[0], minlength=len(pos)) + np.bincount(ei[1], minlength=len(pos))
    assert float(got[0][torch.tensor(deg == 0)].abs().sum()) == 0.0      # a node in no edge: a zero row, written


def test_edge_features_backward_without_edges(dev):
    from gnn_manip_amd import get_edges_displacement
    pos = torch.rand(10, 3, device=dev).requires_grad_()
    none = torch.zeros(0, dtype=torch.int64, device=dev)
    get_edges_displacement(pos, none, none, gc.R).sum().backward()
    assert pos.grad.shape == (10, 3) and float(pos.grad.abs().max()) == 0.0


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_node_features_and_integrator_backward(dev, name):
    """Piecewise-linear functions with coefficients 1 / vel_std, 1 / r, acc_std, 2 and 1: every gradient entry is one or two
    float32 roundings of the reference's, so both are held to 1e-6 of the tensor's maximum (the integrator's bound)."""
    from gnn_manip_amd.rollout import get_position_from_prediction
    L = wc.LAYOUTS[name]
    obs_np = gc.state(name)
    n = obs_np.shape[1]
    w_n, w_p, pred_np = gc.weights((n, L.node_dim), 42), gc.weights((n, 3), 43), gc.weights((n, 3), 44)
    o64, p64 = gc.t64(obs_np, True), gc.t64(pred_np, True)
    ref_nodes = gc.node_features(o64, L)
    (ref_nodes * gc.t64(w_n)).sum().backward()
    g_nodes = o64.grad.clone()
    o64.grad = None
    ref_next = gc.integrate(p64, o64, L)
    (ref_next * gc.t64(w_p)).sum().backward()
    obs = _t(obs_np, dev).requires_grad_(True)
    nodes = graph_attr(gc.R, L).compute_nodes(obs)
    assert nodes.grad_fn is not None
    (nodes * _t(w_n, dev)).sum().backward()
    assert_forward_close(nodes.detach().cpu().numpy(), ref_nodes.detach().numpy(), what=name)
    got = obs.grad.cpu().numpy()
    err = np.abs(got - g_nodes.numpy()).max() / np.abs(g_nodes.numpy()).max()
    print(f"\n[input grads] node features {name}: err {err:.3e}")
    assert err <= 1e-6
    assert np.array_equal(got != 0, g_nodes.numpy() != 0)         # the clamp rule and the columns nothing reads, entry by entry
    obs.grad = None
    pred = _t(pred_np, dev).requires_grad_(True)
    nxt = get_position_from_prediction(STATS, L.cart_idx, pred, obs)
    (nxt * _t(w_p, dev)).sum().backward()
    assert_forward_close(nxt.detach().cpu().numpy(), ref_next.detach().numpy(), what=name)
    for what, g, r in (("d_pred", pred.grad, p64.grad), ("d_obs", obs.grad, o64.grad)):
        err = np.abs(g.cpu().numpy() - r.numpy()).max() / np.abs(r.numpy()).max()
        print(f"[input grads] integrator {name} {what}: err {err:.3e}")
        assert err <= 1e-6, what


# ------------------------------------------------------------------------------------------ the step
@pytest.mark.parametrize("with_target", [True, False])
def test_differentiable_step(dev, with_target):
    params = orc.init_params(*gc.STEP_DIMS, 841)
    m = _model(params, gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    target_np = gc.rigid_target(obs_np, L0, 3) if with_target else None
    obs0 = _t(obs_np, dev)
    assert eng.set_scene(obs0) == len(gc.rigid_rows(obs_np, L0)) > 0
    obs = obs0.clone().requires_grad_(True)
    tgt = _t(target_np, dev).requires_grad_(True) if with_target else None
    nxt, pred, ei = eng.differentiable_step(obs, tgt)
    assert torch.equal(obs.detach(), obs0)                                      # out of place
    w_o, w_p = gc.weights(obs_np.shape, 6), gc.weights((gc.STEP_N, 3), 7)
    ((nxt * _t(w_o, dev)).sum() + (pred * _t(w_p, dev)).sum()).backward()
    # ---- forward: engine.step on a clone is the same state, bit for bit, but for the prediction's own kernels (training / inference)
    stepped = obs0.clone()
    pred_inf = torch.empty_like(pred)
    eng.step(stepped, tgt.detach() if with_target else None, pred_out=pred_inf)
    assert eng.status() == ei.shape[1]
    ei_np = ei.cpu().numpy()
    ref_next, ref_preds, g_obs, g_tgt = _step_reference(params, obs_np, [target_np], [ei_np], w_o, w_p, torch.float64)
    _, _, g_obs32, g_tgt32 = _step_reference(params, obs_np, [target_np], [ei_np], w_o, w_p, torch.float32)
    assert_forward_close(pred.detach().cpu().numpy(), ref_preds[0], floor=1e-3, what="pred")
    from gnn_manip_amd.rollout import get_position_from_prediction
    c = slice(L0.cart, L0.cart + 3)
    rigid = torch.from_numpy(obs_np[-1][:, L0.mat] == 1).to(dev)
    # state_pre changes control columns only, which the integrator does not read: the pre-step window is obs0's for it
    pos = get_position_from_prediction(STATS, L0.cart_idx, pred.detach(), obs0, _desc=eng.fdesc)
    assert torch.equal(nxt.detach()[-1][~rigid][:, c], pos[~rigid])
    if with_target:
        assert torch.equal(nxt.detach()[-1][rigid][:, c], tgt.detach())
    else:
        assert torch.equal(nxt.detach()[-1][rigid][:, c], obs0[-1][rigid][:, c])
    others = [i for i in range(L0.D) if not (c.start <= i < c.stop)]
    assert torch.equal(nxt.detach()[:, :, others], stepped[:, :, others])
    assert torch.equal(nxt.detach()[:-1], stepped[:-1])
    assert_forward_close(nxt.detach()[-1][:, c].cpu().numpy(), ref_next[-1][:, c], what="next position")
    # ---- gradients
    allow = _step_allowance(params, obs_np, [target_np], [ei_np], w_o, w_p)
    _split("step" + (" with target" if with_target else ""), obs.grad.cpu().numpy(), g_obs, g_obs32, allow)
    if with_target:
        _within("step d_rigid_target", tgt.grad.cpu().numpy(), g_tgt[0], g_tgt32[0], lambda: (allow()[0][1], allow()[1]))


def test_differentiable_step_with_two_candidates(dev):
    """candidates = 2 (the batched radius graph): forward and gradients of each scene are those of a single-scene call, bit for
    bit."""
    params = orc.init_params(*gc.STEP_DIMS, 841)
    m = _model(params, gc.STEP_DIMS, dev)
    scenes = [gc.step_state("step_a"), gc.step_state("step_b")]
    targets = [gc.rigid_target(s, L0, 3 + i) for i, s in enumerate(scenes)]
    w_o, w_p = gc.weights(scenes[0].shape, 6), gc.weights((gc.STEP_N, 3), 7)
    single = []
    for s, t in zip(scenes, targets):
        eng = _engine(m, dev)
        eng.set_scene(_t(s, dev))
        obs, tgt = _t(s, dev).requires_grad_(True), _t(t, dev).requires_grad_(True)
        nxt, pred, ei = eng.differentiable_step(obs, tgt)
        ((nxt * _t(w_o, dev)).sum() + (pred * _t(w_p, dev)).sum()).backward()
        single.append((nxt.detach(), pred.detach(), ei, obs.grad, tgt.grad))
    eng2 = _engine(m, dev, candidates=2)
    both = _t(np.concatenate(scenes, axis=1), dev)
    eng2.set_scene(both)
    obs, tgt = both.clone().requires_grad_(True), _t(np.concatenate(targets), dev).requires_grad_(True)
    nxt, pred, ei = eng2.differentiable_step(obs, tgt)
    w_o2, w_p2 = _t(np.concatenate((w_o, w_o), axis=1), dev), _t(np.concatenate((w_p, w_p)), dev)
    ((nxt * w_o2).sum() + (pred * w_p2).sum()).backward()
    n, nr = gc.STEP_N, targets[0].shape[0]
    e0 = single[0][2].shape[1]
    assert torch.equal(ei[:, :e0], single[0][2]) and torch.equal(ei[:, e0:], single[1][2] + n)
    for b in range(2):
        rows = slice(b * n, (b + 1) * n)
        for what, got, ref in (("next_obs", nxt.detach()[:, rows], single[b][0]), ("pred", pred.detach()[rows], single[b][1]),
                               ("d_obs", obs.grad[:, rows], single[b][3]), ("d_target", tgt.grad[b * nr:(b + 1) * nr], single[b][4])):
            assert torch.equal(got, ref), (b, what)     # the same rows through the same kernels: row-wise work, fixed sum orders


def test_two_steps_unrolled_into_samples_loss(dev):
    """d SamplesLoss(end cloud, target cloud) / d (initial obs, both steps' rigid_target) through two differentiable steps,
    against the float64 two-step restatement on the edge lists the GPU returned and sinkhorn_cases' float64 Sinkhorn
    gradient at the restatement's own end cloud."""
    from gnn_manip_amd.losses import SamplesLoss
    params = orc.init_params(*gc.STEP_DIMS, 841)
    m = _model(params, gc.STEP_DIMS, dev)
    eng = _engine(m, dev)
    obs_np = gc.step_state("step_a")
    t1 = gc.rigid_target(obs_np, L0, 3)
    t2 = gc.rigid_target(obs_np, L0, 4, step_size=6e-4)
    eng.set_scene(_t(obs_np, dev))
    fluid = np.nonzero(obs_np[-1][:, L0.mat] != 1)[0]
    # the desired cloud: the fluid moved by (0.03, -0.02, 0.05) -- the displacement of test_gpu_planner.py's known answer, a loss of
    # about |t|^2 / 2 = 1.9e-3 that float32 carries to the forward bar (a cloud a fraction of the blur away leaves a loss of 1e-7,
    # the difference of terms of 1e-3: no float32 evaluation holds that to 1e-5) -- with a seeded per-particle offset
    shift = np.array([0.03, -0.02, 0.05], np.float32)
    cloud = (obs_np[-1][fluid][:, L0.cart:L0.cart + 3] + shift + np.float32(0.004) * gc.weights((len(fluid), 3), 8)).astype(np.float32)
    obs = _t(obs_np, dev).requires_grad_(True)
    tg = [_t(t1, dev).requires_grad_(True), _t(t2, dev).requires_grad_(True)]
    cur, eis = obs, []
    for t in tg:
        cur, _, ei = eng.differentiable_step(cur, t)
        eis.append(ei.cpu().numpy())
    fl = _t(fluid, dev)
    loss = SamplesLoss(loss="sinkhorn", p=2, blur=.05)(cur[-1][fl][:, L0.cart:L0.cart + 3], _t(cloud, dev))
    loss.backward()

    def end_loss(nxt):
        g = np.zeros_like(nxt)
        s, dx, _ = sinkhorn_grad_ref(nxt[-1][fluid][:, L0.cart:L0.cart + 3], cloud)
        g[-1][fluid, L0.cart:L0.cart + 3] = dx
        end_loss.value = s
        return g

    end64, _, g_obs, g_t = _step_reference(params, obs_np, [t1, t2], eis, None, None, torch.float64, end_loss)
    s64 = end_loss.value
    _, _, g_obs32, g_t32 = _step_reference(params, obs_np, [t1, t2], eis, None, None, torch.float32, end_loss)
    loss = float(loss.detach())
    print(f"\n[input grads] two steps: loss {loss:.6e} reference {s64:.6e}")
    assert abs(loss - s64) <= 1e-5 * abs(s64)      # the forward bar of tests/test_gpu_planner.py for this loss
    allow = _step_allowance(params, obs_np, [t1, t2], eis, None, None, end_grad=end_loss(end64))
    _split("two steps", obs.grad.cpu().numpy(), g_obs, g_obs32, allow)
    for i in range(2):
        _within(f"two steps d_rigid_target[{i}]", tg[i].grad.cpu().numpy(), g_t[i], g_t32[i], lambda i=i: (allow()[0][1 + i], allow()[1]))
