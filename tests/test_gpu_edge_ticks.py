"""The systolic edge kernel (hedge.hip: sys_edge_kernel) runs its pipeline's fill and drain as light ticks: a role whose Linear has
no block in a tick runs the barrier and what later ticks or the results need, not a chain on buffers nobody reads.  What can go wrong
is at the ends of a workgroup's range: the first and last blocks' rows, statistics, epilogue and scatter-add, and the hand-over
between the light ticks and the pair loop -- so the sizes here are the ones where a workgroup owns no group, one group (nb = 4: the
fill and drain windows touch), one next to two, and C2's twelve blocks.  hidden 128 / num_layers 2 / 3 message-passing steps
throughout (two launches that write e + e' and one that does not); set_edge_kernel("sys_all") takes the systolic path at any size.
Per case: the decoder output against oracle/torch_epd.py in float64 at the forward parity bar (conftest.assert_forward_close), no
device-side error flag, and the same bits from workspaces that held NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import assert_forward_close
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


def _forward(m, nodes, ea, ei):
    """gm_epd_forward on a zeroed workspace of the test's own; asserts that the device raised no error flag."""
    from gnn_manip_amd import epd_gnn as G
    n, e = int(nodes.shape[0]), int(ea.shape[0])
    L = G.lib()
    h = m.device_handle(nodes.device)
    csr = G.DstCsr(ei, n, flow=m.convention[0])
    d = G.ModelDesc(*m.model_desc())
    ws = torch.zeros(int(L.gm_forward_workspace_bytes(C.byref(d), n, e)), dtype=torch.uint8, device=nodes.device)
    out = torch.empty((n, DIMS[2]), dtype=torch.float32, device=nodes.device)
    G.check(L.gm_epd_forward(h, G.ptr(nodes), n, G.ptr(ea), 0, G.ptr(csr.ws), e, G.ptr(out), G.ptr(ws), ws.numel(), G.current_stream()))
    assert csr.validate() == e   # no device-side error flag (fp16 split range, edge_index)
    return out


def _reference(m, nodes, ea, ei):
    from oracle import torch_epd
    p = {k: v.detach().cpu().double() for k, v in m.state_dict().items()}
    with torch.no_grad():
        return torch_epd.epd_forward(p, nodes.cpu().double(), ea.cpu().double(), ei.cpu().long(), DIMS[4], DIMS[5]).numpy()


def _check(dev, m, nodes, ea, ei, what):
    out = _forward(m, nodes, ea, ei)
    assert_forward_close(out.cpu().numpy(), _reference(m, nodes, ea, ei), floor=1e-3, what=str(what))
    with torch.no_grad():
        clean = m.forward(nodes, ea, ei).clone()
        _poison(dev, float("nan"))
        dirty = m.forward(nodes, ea, ei).clone()
    m.status()
    assert torch.equal(clean, out), (what, "own workspace against the module's", float((clean - out).abs().max()))
    assert torch.equal(clean, dirty), (what, "NaN-poisoned workspaces", float((clean - dirty).abs().max()))


@pytest.mark.parametrize("e", [1, 31, 32, 33, 127, 128, 129, 4 * 128 + 1])
def test_one_group_and_its_neighbours(dev, model, e):
    """One row, a block short of / exactly / past 32 rows, a group short of / exactly / past 128, four groups and a row: every
    workgroup owns no group or one (nb = 4, where only ticks 2 and 3 have all three roles multiplying)."""
    nodes, ea, ei = _random_graph(40, e, 2000 + e, dev)
    _check(dev, model, nodes, ea, ei, e)


def test_one_group_next_to_two(dev, model):
    """E = 128 * 256 + 1: 257 groups over 256 workgroups -- every workgroup has nb = 4 but one, which has nb = 8."""
    nodes, ea, ei = _random_graph(2000, 128 * 256 + 1, 31, dev)
    _check(dev, model, nodes, ea, ei, "257 groups")


def test_twelve_blocks_per_workgroup(dev, model):
    """N = 5000, E = 98 000: three groups per workgroup (some two, some three), the small-scene shape of the benchmark."""
    nodes, ea, ei = _random_graph(5000, 98000, 32, dev)
    _check(dev, model, nodes, ea, ei, "C2 shape")


def test_hub_destination(dev, model):
    """In-degree 200 > 128: the destination's segment crosses groups, so its pieces leave through the side buffer from the first
    and last blocks of neighbouring workgroups' ranges."""
    nodes, ea, ei = _random_graph(600, 4000, 77, dev, hub=200)
    assert int((ei[1] == 300).sum()) >= 200
    _check(dev, model, nodes, ea, ei, "hub")


def test_candidate_of_a_batch_equals_the_graph_alone(dev, model):
    """Three scenes of 700 particles as a block-diagonal batch: candidate 1 == the same scene rolled out alone, bit for bit.  The
    workgroups' ranges -- and with them which blocks meet a fill or drain tick -- differ between the two runs."""
    from gnn_manip_amd import RolloutEngine, scene
    n, steps, b = 700, 2, 3
    obs = scene.make_scene(n, seed=95, side=0.075)
    trajs = np.stack([scene.rigid_drift_trajectory(obs, steps, seed=100 + c, step_size=3e-4) for c in range(b)])
    with torch.no_grad():
        eng_b = RolloutEngine(model, graph_attr(0.015), n, device=dev, candidates=b)
        out = eng_b.rollout_candidates(torch.from_numpy(obs).to(dev), torch.from_numpy(trajs).to(dev))
        eng_1 = RolloutEngine(model, graph_attr(0.015), n, device=dev)
        one = eng_1.rollout(torch.from_numpy(obs).to(dev), torch.from_numpy(trajs[1]).to(dev), horizon=steps)
    assert torch.isfinite(one).all()
    assert torch.equal(out[1], one), float((out[1] - one).abs().max())
