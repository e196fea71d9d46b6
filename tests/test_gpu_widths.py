"""Models and rollouts at widths and state layouts other than the default (cases: width_cases.py; their CPU side:
test_width_cases.py, which also shows that every forward case is well conditioned).

Part A -- models at (node_dim, edge_dim, out_dim) other than (25, 4, 3): the fused forward with every processor kernel and hidden
size, the standalone encoder, training and the GraphIndependent input gradients, each at the bar the suite already uses for it
(assert_forward_close; rtol 1e-5 / atol 3e-6 for the encoder's latents; the gradient yardstick of tests/yardstick.py through gpu_support.check_training_step).
Part B -- feature descriptors other than (k 6, D 8, cart 2, material 1, control 5): the stand-alone feature / integrator / state
kernels against the oracle and a numpy restatement, gm_rigid_rank against numpy.cumsum, one gm_rollout_step against the chain of
stand-alone entry points include/gnn_manip_hip.h documents it as (bit for bit), and rollouts against the oracle's."""
import ctypes as C

import numpy as np
import pytest
import torch

import graph_cases as gc
import width_cases as wc
from conftest import BOUNDS, STATS, assert_forward_close
from oracle import epd_oracle as orc
from gpu_support import check_training_step as _check, dev, feature_desc, graph_attr, load_model as _model, rollout_engine, to_dev as _t

pytestmark = pytest.mark.gpu

GM_ERR_INVALID_ARGUMENT = -1


def _dims(name, hidden=wc.HIDDEN, m_steps=wc.M_STEPS):
    return wc.WIDTHS[name][0] + (hidden, wc.NUM_LAYERS, m_steps)


# ================================================================== Part A: models
@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_fused_forward_with_every_processor_kernel(dev, name):
    """Hidden 128 / 2 layers: the oracle's result at the forward bar, two runs bit for bit, with each processor kernel."""
    wc.check_width_case(name)
    m = _model(wc.params(name), _dims(name), dev)
    for kind in ("dense", "ragged") if name in wc.RAGGED else ("dense",):
        nodes, ea, ei = wc.inputs(name, kind)
        ref = wc.forward_reference(name, wc.HIDDEN, kind)
        for kernel in ("auto", "hm", "sys_all"):
            m.set_edge_kernel(kernel)
            with torch.no_grad():
                outs = [m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy() for _ in range(2)]
                assert m.status() == ei.shape[1]
            assert outs[0].shape == (nodes.shape[0], wc.WIDTHS[name][0][2])
            assert np.array_equal(outs[0], outs[1]), (kind, kernel)
            assert_forward_close(outs[0], ref, floor=1e-3, what=f"{name} {kind} {kernel}")


@pytest.mark.parametrize("hidden", wc.OTHER_HIDDEN)
@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_fused_forward_at_other_hidden_sizes(dev, name, hidden):
    """The streamed kernels at hidden 64, 256 and a zero-padded 100."""
    nodes, ea, ei = wc.inputs(name)
    m = _model(wc.params(name, hidden), _dims(name, hidden), dev)
    m.set_edge_kernel("hm")
    with torch.no_grad():
        outs = [m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy() for _ in range(2)]
    assert np.array_equal(outs[0], outs[1])
    assert_forward_close(outs[0], wc.forward_reference(name, hidden), floor=1e-3, what=f"{name} h{hidden}")


@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_standalone_encoder_and_its_non_finite_rows(dev, name):
    """h0, e0 of gm_graph_independent_forward against the oracle; a non-finite input row comes out as a NaN row and every other row
    keeps its bits (include/gnn_manip_hip.h) -- at node_dim 1, 17 and 32 among the others."""
    nodes, ea, ei = wc.inputs(name)
    nd, ed, _ = wc.WIDTHS[name][0]
    p = wc.params(name)
    m = _model(p, _dims(name), dev)
    ho, eo = orc.graph_independent(p, "encoder", nodes, ea, wc.NUM_LAYERS)
    xb, eb = nodes.copy(), ea.copy()
    xb[7, nd - 1] = np.nan; xb[100, 0] = np.inf; xb[nodes.shape[0] - 1, (nd - 1) // 2] = -np.inf; xb[20, nd - 1] = 1e30
    eb[11, ed - 1] = np.inf; eb[ea.shape[0] - 1, 0] = np.nan; eb[64, ed - 1] = -1e30
    with torch.no_grad():
        h0, e0, _ = m.encoder(_t(nodes, dev), _t(ea, dev), _t(ei, dev))
        h1, e1, _ = m.encoder(_t(xb, dev), _t(eb, dev), _t(ei, dev))
    h0, e0, h1, e1 = (x.cpu().numpy() for x in (h0, e0, h1, e1))
    assert h0.shape == ho.shape and e0.shape == eo.shape
    np.testing.assert_allclose(h0, ho, rtol=1e-5, atol=3e-6)
    np.testing.assert_allclose(e0, eo, rtol=1e-5, atol=3e-6)
    bad_n, bad_e = [7, 100, nodes.shape[0] - 1], [11, ea.shape[0] - 1]
    assert np.isnan(h1[bad_n]).all() and np.isnan(e1[bad_e]).all()
    keep_n = np.ones(nodes.shape[0], bool); keep_n[bad_n + [20]] = False
    keep_e = np.ones(ea.shape[0], bool); keep_e[bad_e + [64]] = False
    assert np.array_equal(h1[keep_n], h0[keep_n]) and np.array_equal(e1[keep_e], e0[keep_e])
    assert np.isfinite(h1[20]).all() and np.isfinite(e1[64]).all()


@pytest.mark.parametrize("hidden", [128, 64])
@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_training_at_every_width(dev, name, hidden):
    """gpu_support.check_training_step as it stands (forward 1e-5, every parameter gradient against float64 autograd inside its
    yardstick); then, by name, the tensors whose shape follows the widths: the right shape, and a reference gradient that is not
    zero, so that passing the yardstick means something."""
    nd, ed, od = wc.WIDTHS[name][0]
    dims = _dims(name, hidden, 2)
    seed = wc.weight_seed(name, hidden)
    params = orc.init_params(*dims, seed)
    nodes, ea, ei = wc.inputs(name, "ragged" if (name in wc.RAGGED and hidden == 64) else "dense")
    m = _model(params, dims, dev)
    ref = {}
    _check(m, params, nodes, ea, ei, dims, dev, seed, ref=ref)
    last = 2 * wc.NUM_LAYERS
    shapes = {"encoder.phi_node.0.weight": (hidden, nd), "encoder.phi_edge.0.weight": (hidden, ed),
              f"decoder.{last}.weight": (od, hidden), f"decoder.{last}.bias": (od,)}
    got = dict(m.named_parameters())
    assert ref["target"].shape == (nodes.shape[0], od)
    for key, shape in shapes.items():
        assert tuple(got[key].grad.shape) == shape == ref["ref_g"][key].shape, key
        assert np.abs(ref["ref_g"][key]).max() > 0, key


@pytest.mark.parametrize("name", list(wc.WIDTHS))
def test_graph_independent_input_gradients_at_every_width(dev, name):
    """dx [N, node_dim] and dedge_attr [E, edge_dim] against float64 autograd, at the bar of test_graph_independent_input_gradients
    -- node_dim 1 and 32, edge_dim 1 and 8 among the cases.  No case has a ReLU within float32 rounding of a sign change
    (test_width_cases.py: test_input_gradient_case_is_well_conditioned), so the bar tests the kernel."""
    nodes, ea, ei = wc.inputs(name)
    m = _model(wc.params(name), _dims(name), dev)
    wh, we, dx64, dea64 = wc.input_gradient_reference(name)
    x = _t(nodes, dev).requires_grad_(True)
    a = _t(ea, dev).requires_grad_(True)
    h, e, _ = m.encoder(x, a, _t(ei, dev))
    ((h * _t(wh, dev)).sum() + (e * _t(we, dev)).sum()).backward()
    for got, ref, shape in ((x.grad, dx64, nodes.shape), (a.grad, dea64, ea.shape)):
        assert tuple(got.shape) == shape == ref.shape
        err = np.abs(got.cpu().numpy() - ref).max()
        print(f"{name} {shape}: max err = {err:.3e}, max |ref| = {np.abs(ref).max():.3e}")
        assert err <= 2e-4 * np.abs(ref).max()


# ================================================================== Part B: features and state
class _Abi:
    """The stand-alone entry points through ctypes: device tensors in, status codes checked."""

    def __init__(self, dev):
        from gnn_manip_amd._lib import check, current_stream, lib
        self.L, self.check, self.dev = lib(), check, dev
        self.stream = lambda: current_stream(dev)

    @staticmethod
    def p(t, offset=0):
        return None if t is None else C.c_void_p(t.data_ptr() + 4 * offset)

    def u8(self, nbytes):
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=self.dev)

    def rank(self, obs, fd):
        n = obs.shape[1]
        rank = torch.full((n,), -7, dtype=torch.int32, device=self.dev)
        cnt = torch.full((1,), -7, dtype=torch.int32, device=self.dev)
        self.check(self.L.gm_rigid_rank(self.p(obs), n, C.byref(fd), self.p(rank), self.p(cnt), self.stream()))
        return rank, int(cnt.item())

    def state_pre(self, obs, fd, rank, target):
        return self.L.gm_state_pre(self.p(obs), obs.shape[1], C.byref(fd), self.p(rank), self.p(target), self.stream())

    def state_post(self, obs, fd, next_pos, rank, target):
        self.check(self.L.gm_state_post(self.p(obs), obs.shape[1], C.byref(fd), self.p(next_pos), self.p(rank), self.p(target), self.stream()))

    def node_features(self, obs, fd, node_dim):
        out = torch.empty((obs.shape[1], node_dim), dtype=torch.float32, device=self.dev)
        self.check(self.L.gm_node_features(self.p(obs), obs.shape[1], C.byref(fd), self.p(out), self.stream()))
        return out

    def integrate(self, pred, obs, fd):
        out = torch.empty((obs.shape[1], 3), dtype=torch.float32, device=self.dev)
        self.check(self.L.gm_integrate(self.p(pred), self.p(obs), obs.shape[1], C.byref(fd), self.p(out), self.stream()))
        return out


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_node_features_and_integrator_per_layout(dev, name):
    L = wc.LAYOUTS[name]
    obs = wc.scene_in_layout(name)
    abi, fd = _Abi(dev), feature_desc(wc.R, L)
    tobs = _t(obs, dev)
    ref = orc.compute_nodes(obs, STATS, BOUNDS, wc.R, L.cart_idx, [L.mat], L.ctrl_idx)
    assert ref.shape[1] == L.node_dim
    for got in (abi.node_features(tobs, fd, L.node_dim), graph_attr(wc.R, L).compute_nodes(tobs)):
        got = got.cpu().numpy()
        np.testing.assert_allclose(got, ref, rtol=2e-7, atol=1e-7)
        mat_col = 3 * (L.k - 1) + 6
        assert np.array_equal(got[:, mat_col], obs[-1][:, L.mat]) and set(np.unique(got[:, mat_col])) == {0.0, 1.0, 2.0}
    pred = np.random.Generator(np.random.PCG64(801)).standard_normal((obs.shape[1], 3)).astype(np.float32)
    nxt = abi.integrate(_t(pred, dev), tobs, fd).cpu().numpy()
    assert np.array_equal(nxt, orc.get_position_from_prediction(STATS, L.cart_idx, pred, obs))
    assert torch.equal(tobs, _t(obs, dev))                                  # neither kernel writes the state


@pytest.mark.parametrize("with_target", [True, False])
@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_state_pre_and_post_per_layout(dev, name, with_target):
    """gm_state_pre / gm_state_post against the float32 numpy restatement of rollout_utils.py:40-47 / 53-61, bit for bit over the
    whole [k, N, D] state: payload columns ride through the window shift, non-rigid rows keep every column but xyz, and with
    target = NULL control takes the current xyz and post leaves rigid rows where they are.  A descriptor without control columns
    is rejected by the stand-alone gm_state_pre (documented), and leaves the state alone."""
    L = wc.LAYOUTS[name]
    obs = wc.scene_in_layout(name)
    abi, fd = _Abi(dev), feature_desc(wc.R, L)
    state = _t(obs, dev).clone()
    rank, n_rigid = abi.rank(state, fd)
    rigid = wc.rigid_rows(obs, L)
    assert n_rigid == rigid.sum()
    assert np.array_equal(rank.cpu().numpy(), np.where(rigid, np.cumsum(rigid) - 1, -1))
    target = wc.drift_trajectory(obs, L, 1, 802)[0] if with_target else None
    tt = None if target is None else _t(target, dev)
    rc = abi.state_pre(state, fd, rank, tt)
    if L.ctrl < 0:
        assert rc == GM_ERR_INVALID_ARGUMENT and torch.equal(state, _t(obs, dev))
        want = np.array(obs)
    else:
        assert rc == 0
        want = wc.state_pre(obs, L, target)
        assert not np.array_equal(want, obs)
    got = state.cpu().numpy()
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    nxt = np.random.Generator(np.random.PCG64(803)).random((obs.shape[1], 3)).astype(np.float32)
    abi.state_post(state, fd, _t(nxt, dev), rank, tt)
    got, want2 = state.cpu().numpy(), wc.state_post(want, L, nxt, target)
    assert np.array_equal(got, want2), np.argwhere(got != want2)[:5]
    # what the restatement implies, spelled out: payload of frame t is the input's frame t + 1; rigid xyz = target or unchanged
    for c in L.payload:
        assert np.array_equal(got[:-1, :, c], obs[1:, :, c]) and np.array_equal(got[-1, :, c], obs[-1, :, c])
    assert np.array_equal(got[-1][rigid][:, L.cart_idx], target if with_target else obs[-1][rigid][:, L.cart_idx])
    assert np.array_equal(got[-1][~rigid][:, L.cart_idx], nxt[~rigid])
    # without ranks every row is a free particle
    state2 = _t(obs, dev).clone()
    abi.state_post(state2, fd, _t(nxt, dev), None, None)
    free = np.array(obs); free[:-1] = obs[1:]; free[-1][:, L.cart_idx] = nxt
    assert np.array_equal(state2.cpu().numpy(), free)


@pytest.mark.parametrize("n", wc.RANK_SIZES)
def test_rigid_rank_is_a_cumsum(dev, n):
    """One block of 1024 threads with a running carry: sizes around the block, rigid rows on its edges, material 2.0 not rigid."""
    abi = _Abi(dev)
    for lname in ("default", "moved"):
        L = wc.LAYOUTS[lname]
        fd = feature_desc(wc.R, L)
        for pattern in ("placed", "none", "all"):
            mat = wc.rank_material(n, pattern)
            rigid = mat == 1
            if pattern == "placed":
                assert all(rigid[i] for i in (0, 1023, 1024, n - 1) if i < n) and ((mat == 2).any() or n == 1)
            obs = np.full((L.k, n, L.D), 1.0, np.float32)       # every other column, and the material of earlier frames, reads 1.0
            obs[-1, :, L.mat] = mat
            rank, n_rigid = abi.rank(_t(obs, dev), fd)
            assert n_rigid == rigid.sum() == {"none": 0, "all": n}.get(pattern, rigid.sum()), (lname, pattern)
            assert np.array_equal(rank.cpu().numpy(), np.where(rigid, np.cumsum(rigid) - 1, -1)), (lname, pattern)


def _step_and_chain(dev, name, kernel, obs=None, K=20, flow=0):
    """obs: a state in the layout `name` (default: wc.scene_in_layout's); flow 1: a model of the flow="target_to_source" convention,
    the chain's sort through gm_csr_from_graph_flow.  Returns the longest segment of the destination sort, by the oracle's edges."""
    from gnn_manip_amd._lib import ModelDesc
    L = wc.LAYOUTS[name]
    obs = wc.scene_in_layout(name) if obs is None else obs
    n = obs.shape[1]
    cap = n * K
    dims = (L.node_dim, 4, 3, wc.HIDDEN, wc.NUM_LAYERS, wc.M_STEPS)
    params = orc.init_params(*dims, 810 + list(wc.LAYOUTS).index(name))
    m = _model(params, dims, dev, **(dict(flow="target_to_source") if flow else {}))
    m.set_edge_kernel(kernel)
    handle = m.device_handle(dev)
    abi, fd, md = _Abi(dev), feature_desc(wc.R, L), ModelDesc(*m.model_desc())
    lib, p, check = abi.L, abi.p, abi.check
    target = _t(wc.drift_trajectory(obs, L, 1, 811)[0], dev)
    # --- one fused step
    a = _t(obs, dev).clone()
    rank, _ = abi.rank(a, fd)
    ws = abi.u8(lib.gm_rollout_workspace_bytes(C.byref(md), n, K))
    pred_a = torch.empty((n, 3), dtype=torch.float32, device=dev)
    check(lib.gm_rollout_step(handle, p(a), n, C.byref(fd), K, p(rank), p(target), p(pred_a), p(ws), ws.numel(), abi.stream()))
    e_a = C.c_int64(-1)
    check(lib.gm_rollout_status(p(ws), C.byref(md), n, K, C.byref(e_a), abi.stream()))
    # --- the chain the header documents, through the stand-alone entry points
    b = _t(obs, dev).clone()
    if L.ctrl >= 0:
        assert abi.state_pre(b, fd, rank, target) == 0
    x = abi.node_features(b, fd, L.node_dim)
    last = (L.k - 1) * n * L.D + L.cart
    gws = abi.u8(lib.gm_graph_workspace_bytes(n, K))
    check(lib.gm_radius_graph_build(p(b, last), L.D, n, wc.R, K, p(gws), gws.numel(), abi.stream()))
    cws = abi.u8(lib.gm_csr_workspace_bytes(n, cap))
    if flow == 0:
        check(lib.gm_csr_from_graph(p(gws), n, K, p(cws), cws.numel(), abi.stream()))
    else:
        check(lib.gm_csr_from_graph_flow(p(gws), n, K, flow, p(cws), cws.numel(), abi.stream()))
    ea = torch.zeros((cap, 4), dtype=torch.float32, device=dev)
    check(lib.gm_edge_features_csr(p(b, last), L.D, p(cws), n, cap, wc.R, p(ea), abi.stream()))
    fws = abi.u8(lib.gm_forward_workspace_bytes(C.byref(md), n, cap))
    pred_b = torch.empty((n, 3), dtype=torch.float32, device=dev)
    check(lib.gm_epd_forward(handle, p(x), n, p(ea), 1, p(cws), cap, p(pred_b), p(fws), fws.numel(), abi.stream()))
    e_b = C.c_int64(-2)
    check(lib.gm_csr_num_edges(p(cws), C.byref(e_b), abi.stream()))
    nxt = abi.integrate(pred_b, b, fd)
    abi.state_post(b, fd, nxt, rank, target)
    torch.cuda.synchronize()
    snd_ref, rcv_ref = orc.get_connectivity(obs[-1][:, L.cart_idx], wc.R, K)
    assert e_a.value == e_b.value == snd_ref.shape[0]
    assert torch.isfinite(pred_a).all() and float(pred_a.abs().max()) > 0
    assert torch.equal(pred_a, pred_b), float((pred_a - pred_b).abs().max())
    assert torch.equal(a, b), float((a - b).abs().max())
    assert not torch.equal(a, _t(obs, dev))
    return int(np.bincount(snd_ref if flow else rcv_ref, minlength=n).max())   # a segment: the edges that aggregate at one node


@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_a_step_is_the_chain_it_documents(dev, name):
    """gm_rollout_step (fused launches: pre + features, graph + in-degrees, sort + edge features, forward, integrate + post) against
    state_pre -> node features -> radius graph -> csr -> edge features -> forward -> integrate -> state_post through the
    stand-alone entry points: final states, predictions and edge counts equal bit for bit.  The model is pinned to the streamed
    kernels, so that both paths take the same ones."""
    _step_and_chain(dev, name, "hm")


def test_a_step_is_the_chain_it_documents_systolic(dev):
    _step_and_chain(dev, "default", "sys_all")


def test_a_step_is_the_chain_it_documents_at_flow_1_with_long_segments(dev):
    """The sort's own edge features at flow 1 on segments the whole workgroup sorts (more than 96 edges: segment_sort_kernel's long
    path), which run inside gm_rollout_step only.  At flow 1 a query's own list is its segment, so K = 128 on graph_cases'
    a3_cluster150 -- 151 rows on one point, nine more within conn_r of it, whose lists of 128 carry 127 non-zero features each --
    gives 160 segments of 128.  Its positions are the last frame of a state in the default layout."""
    geo = gc.geometry("a3_cluster150")
    on_one_point = np.flatnonzero((geo.pos == geo.pos[17]).all(axis=1))
    assert on_one_point.size >= 151 and geo.r == wc.R
    obs = gc.scene_with_last_frame(geo.pos, on_one_point, seed=812)
    assert obs.shape[::2] == (wc.LAYOUTS["default"].k, wc.LAYOUTS["default"].D)
    assert _step_and_chain(dev, "default", "hm", obs=obs, K=128, flow=1) > 96


def _rollout_model(name, dev):
    L = wc.LAYOUTS[name]
    dims = (L.node_dim, 4, 3, wc.HIDDEN, wc.NUM_LAYERS, wc.M_STEPS)
    params = orc.init_params(*dims, 820 + list(wc.LAYOUTS).index(name))
    return L, params, _model(params, dims, dev)


def _oracle_rollout(params, obs, traj, horizon, L):
    return orc.rollout(params, obs, traj, horizon, STATS, BOUNDS, wc.R, L.cart_idx, [L.mat], L.ctrl_idx, wc.NUM_LAYERS, wc.M_STEPS, record=True)


def _assert_state_close(got, ref, L, what):
    other = [c for c in range(L.D) if c not in L.cart_idx]
    err = np.abs(got[..., L.cart_idx] - ref[..., L.cart_idx]).max()
    print(f"{what}: max |pos - oracle| = {err:.3e}")
    np.testing.assert_allclose(got[..., L.cart_idx], ref[..., L.cart_idx], rtol=0, atol=5e-6)
    assert np.array_equal(got[..., other], ref[..., other]), (what, np.argwhere(got[..., other] != ref[..., other])[:5])


@pytest.mark.parametrize("t_len", [2, 1])
@pytest.mark.parametrize("name", list(wc.LAYOUTS))
def test_rollout_with_records_against_the_oracle(dev, name, t_len):
    """Two steps of RolloutEngine.rollout(record=True) against orc.rollout(record=True): positions at the rollout tests' bar, every
    other column -- payload, material, control -- bit for bit, in the final state and in the records; t_len = 1: the horizon is
    longer than the trajectory.  Without control columns the record is the last frame as it stands."""
    L, params, m = _rollout_model(name, dev)
    obs = wc.scene_in_layout(name)
    traj = wc.drift_trajectory(obs, L, t_len, 830)
    ref, ref_rec = _oracle_rollout(params, obs, traj, 2, L)
    with torch.no_grad():
        eng = rollout_engine(m, wc.R, L, wc.SCENE_N, dev)
        final, recs = eng.rollout(_t(obs, dev), _t(traj, dev), horizon=2, record=True)
        e = eng.status()
        plain = eng.rollout(_t(obs, dev), _t(traj, dev), horizon=2)
    assert e > 10 * wc.SCENE_N and recs.shape == (2, wc.SCENE_N, L.D)
    assert torch.equal(plain, final)                                        # recording does not change the rollout
    _assert_state_close(final.cpu().numpy(), ref, L, f"{name} T={t_len} final")
    _assert_state_close(recs.cpu().numpy(), ref_rec, L, f"{name} T={t_len} records")
    if L.ctrl < 0:
        assert np.array_equal(recs[0].cpu().numpy(), obs[-1])


def test_candidates_without_control_columns(dev):
    name = "no_control"
    L, params, m = _rollout_model(name, dev)
    obs = wc.scene_in_layout(name)
    trajs = np.stack([wc.drift_trajectory(obs, L, 2, 840 + c) for c in range(3)])
    with torch.no_grad():
        one = rollout_engine(m, wc.R, L, wc.SCENE_N, dev)
        singles = [one.rollout(_t(obs, dev), _t(trajs[c], dev), horizon=2).cpu().numpy() for c in range(3)]
        out = rollout_engine(m, wc.R, L, wc.SCENE_N, dev, candidates=3).rollout_candidates(_t(obs, dev), _t(trajs, dev)).cpu().numpy()
    for c in range(3):
        assert np.array_equal(out[c], singles[c]), (c, np.abs(out[c] - singles[c]).max())
    assert not np.array_equal(singles[0], singles[1])
    ref, _ = _oracle_rollout(params, obs, trajs[2], 2, L)
    _assert_state_close(out[2], ref, L, "no_control candidate 2")


def test_renumbered_rollout_with_moved_columns(dev):
    name = "moved"
    L, params, m = _rollout_model(name, dev)
    obs = np.array(wc.scene_in_layout(name))
    obs = np.ascontiguousarray(obs[:, np.random.Generator(np.random.PCG64(850)).permutation(obs.shape[1])])   # rigid rows scattered
    traj = wc.drift_trajectory(obs, L, 2, 851)
    with torch.no_grad():
        f0, r0 = rollout_engine(m, wc.R, L, wc.SCENE_N, dev, renumber=False).rollout(_t(obs, dev), _t(traj, dev), horizon=2, record=True)
        ren = rollout_engine(m, wc.R, L, wc.SCENE_N, dev, renumber=True)
        ren.RENUMBER_EVERY = 1
        f1, r1 = ren.rollout(_t(obs, dev), _t(traj, dev), horizon=2, record=True)
        assert ren.status() > 0 and ren.renumber
    f0, r0, f1, r1 = (x.cpu().numpy() for x in (f0, r0, f1, r1))
    other = [c for c in range(L.D) if c not in L.cart_idx]
    print(f"moved: max |renumbered - plain| = {np.abs(f1 - f0).max():.3e}")
    np.testing.assert_allclose(f1, f0, rtol=0, atol=2e-6)
    np.testing.assert_allclose(r1, r0, rtol=0, atol=2e-6)
    assert np.array_equal(f1[..., other], f0[..., other]) and np.array_equal(r1[..., other], r0[..., other])
    ref, ref_rec = _oracle_rollout(params, obs, traj, 2, L)
    _assert_state_close(f1, ref, L, "moved renumbered final")
    _assert_state_close(r1, ref_rec, L, "moved renumbered records")
