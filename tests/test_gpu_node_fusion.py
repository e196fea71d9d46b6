"""The systolic node path runs a processor step's node MLP and the next step's projections as one launch
(hedge.hip: sys_node_proj_kernel; model.set_node_fusion(False) selects the two launches it is made of).  Per-row arithmetic,
addition orders and stores are those of the two kernels, so the bar is equality bit for bit -- of the decoder output and of
everything the forward leaves in its workspace (h, P, agg, the side buffer, e, Q) -- at the sizes where a block boundary, a partial
last block or a workgroup without blocks can go wrong.  hidden 128 / num_layers 2 / 3 message-passing steps throughout: two fused
launches and the last step's plain node kernel per forward; set_edge_kernel("sys_all") takes the systolic node path at any size."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_support import dev, graph_attr, poison_allocator as _poison, torch_random_graph as _random_graph

pytestmark = pytest.mark.gpu

DIMS = (25, 4, 3, 128, 2, 3)


@pytest.fixture(scope="module")
def model(dev):
    from gnn_manip_amd import EncProcDecGNN
    torch.manual_seed(128)
    m = EncProcDecGNN(*DIMS).to(dev)
    m.set_edge_kernel("sys_all")
    return m


def _forward(m, nodes, ea, ei, fused):
    """gm_epd_forward on a workspace of the test's own (zeroed, so that what no kernel writes compares equal): the decoder output
    and the workspace the forward leaves behind."""
    from gnn_manip_amd import epd_gnn as G
    m.set_node_fusion(fused)
    n, e = int(nodes.shape[0]), int(ea.shape[0])
    L = G.lib()
    h = m.device_handle(nodes.device)
    csr = G.DstCsr(ei, n, flow=m.convention[0])
    d = G.ModelDesc(*m.model_desc())
    ws = torch.zeros(int(L.gm_forward_workspace_bytes(C.byref(d), n, e)), dtype=torch.uint8, device=nodes.device)
    out = torch.empty((n, DIMS[2]), dtype=torch.float32, device=nodes.device)
    G.check(L.gm_epd_forward(h, G.ptr(nodes), n, G.ptr(ea), 0, G.ptr(csr.ws), e, G.ptr(out), G.ptr(ws), ws.numel(), G.current_stream()))
    assert csr.validate() == e   # no device-side error flag (fp16 split range, edge_index)
    return out, ws


def _node_launches(m, nodes, ea, ei, fused):
    m.set_node_fusion(fused)
    m.profile(1 << 1)   # the node kind: stitch, node MLP, projections
    with torch.no_grad():
        m.forward(nodes, ea, ei)
    launches = m.profile_query(1)[0]
    m.profile(0)
    return launches


def _assert_same(a, b, what):
    (out_a, ws_a), (out_b, ws_b) = a, b
    assert torch.isfinite(out_a).all(), what
    assert torch.equal(out_a, out_b), (what, "decoder output", float((out_a - out_b).abs().max()))
    assert torch.equal(ws_a, ws_b), (what, "workspace (h, P, agg, e, Q)", int((ws_a != ws_b).sum()))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 64 + 1, 3000])
def test_fused_forward_equals_the_two_launch_forward(dev, model, n):
    """One block, a partial block, exactly one, one and a row, two and a row, 94 blocks over 256 workgroups: most workgroups own
    no block at all and must leave both phases at once."""
    nodes, ea, ei = _random_graph(n, max(4, 6 * n), 1000 + n, dev)
    _assert_same(_forward(model, nodes, ea, ei, True), _forward(model, nodes, ea, ei, False), n)


def test_the_switch_selects_the_launch_count(dev, model):
    """M - 1 = 2 launches fewer under the node kind with the fused path: it is the path a forward takes by default."""
    nodes, ea, ei = _random_graph(3000, 18000, 4000, dev)
    two = _node_launches(model, nodes, ea, ei, False)
    one = _node_launches(model, nodes, ea, ei, True)
    assert two - one == DIMS[5] - 1, (two, one)
    from gnn_manip_amd import EncProcDecGNN
    fresh = EncProcDecGNN(*DIMS).to(dev)
    fresh.set_edge_kernel("sys_all")
    fresh.profile(1 << 1)
    with torch.no_grad():
        fresh.forward(nodes, ea, ei)
    assert fresh.profile_query(1)[0] == one   # the default is on


def test_hub_destination(dev, model):
    """In-degree 200 > 128: the destination's segment crosses groups of the scatter-add, so its agg row is completed by the
    stitch launch in front of the fused kernel."""
    nodes, ea, ei = _random_graph(600, 4000, 77, dev, hub=200)
    assert int((ei[1] == 300).sum()) >= 200
    _assert_same(_forward(model, nodes, ea, ei, True), _forward(model, nodes, ea, ei, False), "hub")


def test_candidate_of_a_batch_equals_the_graph_alone(dev, model):
    """Three scenes of 700 particles as a block-diagonal batch: candidate 1 == the same scene rolled out alone, bit for bit,
    through the fused kernel (whose blocks are plain runs of 32 rows of the batch: a per-row result does not depend on its block)."""
    from gnn_manip_amd import RolloutEngine, scene
    n, steps, b = 700, 2, 3
    obs = scene.make_scene(n, seed=95, side=0.075)
    trajs = np.stack([scene.rigid_drift_trajectory(obs, steps, seed=100 + c, step_size=3e-4) for c in range(b)])
    model.set_node_fusion(True)
    with torch.no_grad():
        eng_b = RolloutEngine(model, graph_attr(0.015), n, device=dev, candidates=b)
        out = eng_b.rollout_candidates(torch.from_numpy(obs).to(dev), torch.from_numpy(trajs).to(dev))
        eng_1 = RolloutEngine(model, graph_attr(0.015), n, device=dev)
        one = eng_1.rollout(torch.from_numpy(obs).to(dev), torch.from_numpy(trajs[1]).to(dev), horizon=steps)
    assert torch.isfinite(one).all()
    assert torch.equal(out[1], one), float((out[1] - one).abs().max())


def test_rollout_states_do_not_depend_on_the_switch(dev, model):
    """Three rollout steps at N = 3000: the state windows with the fused launch and with the pair."""
    from gnn_manip_amd import RolloutEngine, scene
    n, steps = 3000, 3
    obs = scene.make_scene(n, seed=41, side=0.12)
    traj = torch.from_numpy(scene.rigid_drift_trajectory(obs, steps)).to(dev)
    eng = RolloutEngine(model, graph_attr(0.015), n, device=dev)
    got = {}
    for fused in (True, False):
        model.set_node_fusion(fused)
        with torch.no_grad():
            got[fused] = eng.rollout(torch.from_numpy(obs).to(dev), traj, horizon=steps).clone()
    model.set_node_fusion(True)
    assert torch.isfinite(got[True]).all()
    assert torch.equal(got[True], got[False]), float((got[True] - got[False]).abs().max())


def test_fused_forward_does_not_depend_on_what_the_workspaces_held(dev, model):
    """Phase B reads whole 32-row blocks of h' where phase A wrote the rows below n only, and overlays its LDS map on phase A's:
    the forward and a rollout on workspaces that held NaN return bit for bit what they return on clean memory."""
    from gnn_manip_amd import RolloutEngine, scene
    model.set_node_fusion(True)
    nodes, ea, ei = _random_graph(3000 + 13, 18000, 9, dev)
    obs = scene.make_scene(900, seed=77, side=0.08)
    traj = torch.from_numpy(scene.rigid_drift_trajectory(obs, 2)).to(dev)

    def runs():
        with torch.no_grad():
            out = model.forward(nodes, ea, ei).clone()
            eng = RolloutEngine(model, graph_attr(0.015), obs.shape[1], device=dev)
            state = eng.rollout(torch.from_numpy(obs).to(dev), traj, horizon=2).clone()
        model.status()
        torch.cuda.synchronize()
        return out, state

    clean = runs()
    _poison(dev, float("nan"))
    dirty = runs()
    for c, d in zip(clean, dirty):
        assert torch.isfinite(c).all()
        assert torch.equal(c, d), float((c - d).abs().max())
