"""BASELINE.json's full sizes (N = 100k target scene, N = 50k C3 scene): bit-exact graph against the oracle where the
oracle still runs in seconds, and size-independent properties for the rest (sortedness, stability, window shift,
two independent kernel sets agreeing)."""
import numpy as np
import pytest
import torch

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc
from gpu_support import dev, to_dev as _t

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scene100k():
    from gnn_manip_amd import scene
    return scene.make_scene(100000, seed=5)


@pytest.mark.parametrize("n,seed", [(100000, 5), (50000, 6)])
def test_radius_graph_full_size_bit_exact(dev, n, seed):
    from gnn_manip_amd import get_connectivity, scene
    pos = scene.make_scene(n, seed=seed)[-1][:, 2:5]
    s_ref, r_ref = orc.get_connectivity(pos, 0.015, 20)
    s, r = get_connectivity(_t(pos, dev), 0.015, 20)
    np.testing.assert_array_equal(s.cpu().numpy(), s_ref)
    np.testing.assert_array_equal(r.cpu().numpy(), r_ref)
    # properties of the list itself: grouped by query, self edge first, distances ascending and inside the radius, cap 20
    s_np, r_np = s.cpu().numpy(), r.cpu().numpy()
    assert (np.diff(s_np) >= 0).all()
    starts = np.flatnonzero(np.r_[True, np.diff(s_np) > 0])
    assert (r_np[starts] == s_np[starts]).all()
    counts = np.diff(np.r_[starts, len(s_np)])
    assert counts.max() <= 20 and len(starts) == n
    d = np.linalg.norm(pos[s_np].astype(np.float64) - pos[r_np].astype(np.float64), axis=1)
    assert (d <= 0.015).all()
    same = s_np[1:] == s_np[:-1]
    p64 = pos.astype(np.float64)
    d2 = ((p64[s_np] - p64[r_np]) ** 2).sum(axis=1)
    assert (d2[1:][same] > d2[:-1][same]).all()  # strictly ascending: no tie among the kept neighbours of this random scene (ties go to the smaller index: test_gpu_graph_edges.py)


def test_csr_full_size_is_a_stable_sort(dev, scene100k):
    from gnn_manip_amd import get_connectivity
    from gnn_manip_amd.epd_gnn import DstCsr
    from gnn_manip_amd._lib import lib
    pos = scene100k[-1][:, 2:5]
    s, r = get_connectivity(_t(pos, dev), 0.015, 20)
    ei = torch.stack((s, r))
    n, e = pos.shape[0], int(ei.shape[1])
    csr = DstCsr(ei, n)
    assert csr.validate() == e
    # the workspace layout is internal; read it back through the same carve the library uses (ints after the header)
    ws = csr.ws.cpu().numpy().view(np.int32)
    # in_ptr is the first array after the 16-byte header, 256-byte aligned
    in_ptr = ws[64:64 + n + 1]
    assert in_ptr[0] == 0 and in_ptr[-1] == e and (np.diff(in_ptr) >= 0).all()
    indeg = np.bincount(r.cpu().numpy(), minlength=n)
    np.testing.assert_array_equal(np.diff(in_ptr), indeg)


def test_forward_full_size_two_kernel_sets_agree(dev, scene100k):
    """Fused inference kernels (systolic fp16 x 3 edge kernel with its in-register segmented scatter-add, streamed fp16 x 3 node
    kernels) against the tape-recording training forward (bf16 x 3 split chains on the bf16 matrix pipe, separate deterministic
    segment sums) on the target scene: E = 1.96 M."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    params = orc.init_params(25, 4, 3, 128, 2, 10, 77)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    with torch.no_grad():
        nodes, ea, s, r, _ = ga.process(_t(scene100k, dev), None)
        ei = torch.stack((s, r))
        a = m.forward(nodes, ea, ei)
    b = m.forward(nodes, ea, ei).detach()  # autograd enabled: training forward
    assert torch.isfinite(a).all()
    assert (a - b).abs().max() <= 1e-5 * a.abs().max()
    # permutation of the edge list is immaterial (destination sort + deterministic order inside a segment)
    perm = torch.randperm(ei.shape[1], device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    with torch.no_grad():
        c = m.forward(nodes, ea[perm], ei[:, perm])
    assert (a - c).abs().max() <= 1e-5 * a.abs().max()


def test_forward_c3_size_against_the_oracle(dev):
    """EncProcDecGNN.forward at BASELINE config C3's size (N = 50k, E ~ 1M) with m_steps = 2 against the numpy oracle on
    the same graph and weights: 1e-5 relative (north_star).  The production path of this size: systolic fp16 x 3 edge kernel."""
    from gnn_manip_amd import EncProcDecGNN, scene
    obs = scene.make_scene(50000, seed=6)
    params = orc.init_params(25, 4, 3, 128, 2, 2, 79)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 2)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    nodes, ea, s, r, _ = orc.process(obs, None, STATS, BOUNDS, 0.015, CART, MAT, CTRL)
    ei = np.stack((s, r))
    assert ei.shape[1] > 900000
    with torch.no_grad():
        out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy()
    ref = orc.epd_forward(params, nodes, ea, ei, 2, 2)
    assert np.isfinite(out).all()
    assert np.abs(out - ref).max() <= 1e-5 * np.abs(ref).max()


def _forward_vs_oracle(dev, obs, hidden, seed, m_steps=1, host="numpy"):
    """host: "numpy" -- oracle/epd_oracle.py; "torch32" -- oracle/torch_epd.py in float32 with the box's host threads (the same
    restatement, itself checked against the numpy oracle: what makes the full-depth sizes affordable)."""
    from gnn_manip_amd import EncProcDecGNN
    params = orc.init_params(25, 4, 3, hidden, 2, m_steps, seed)
    m = EncProcDecGNN(25, 4, 3, hidden, 2, m_steps)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    nodes, ea, s, r, _ = orc.process(obs, None, STATS, BOUNDS, 0.015, CART, MAT, CTRL)
    ei = np.stack((s, r))
    with torch.no_grad():
        out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy()
    assert m.status() == ei.shape[1]
    if host == "numpy":
        ref = orc.epd_forward(params, nodes, ea, ei, 2, m_steps)
    else:
        import os
        from oracle import torch_epd
        torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
        with torch.no_grad():
            ref = torch_epd.epd_forward({k: torch.from_numpy(v) for k, v in params.items()}, torch.from_numpy(nodes),
                                        torch.from_numpy(ea), torch.from_numpy(ei), 2, m_steps).numpy()
    assert np.isfinite(out).all()
    # per element, not only against the largest one: |out - ref| <= 1e-5 |ref| + 1e-5 rms(ref) everywhere, so that a component much
    # smaller than the tensor's maximum is still held in relative terms (down to the tensor's rms, below which float32 itself -- the
    # reference's arithmetic -- carries no relative information through a 10-step network)
    rms = float(np.sqrt(np.mean(ref.astype(np.float64) ** 2)))
    worst = float((np.abs(out - ref) / (1e-5 * np.abs(ref) + 1e-5 * rms)).max())
    assert worst <= 1.0, ("per-element bound", worst)
    return np.abs(out - ref).max() / np.abs(ref).max(), ei.shape[1]


def test_target_size_is_as_accurate_as_float32_against_float64(dev, scene100k):
    """The split-operand kernels at the benchmark's own size and depth (N = 100k, E ~ 1.97 M, hidden 128, all ten message-passing
    steps) against a FLOAT64 evaluation of the same model on the host (oracle/torch_epd.py): their error must be of the order of
    a plain float32 evaluation's on the same inputs (tests/test_gpu_parity.py holds the same over five seeds at N = 2,500)."""
    import os
    from gnn_manip_amd import EncProcDecGNN
    from oracle import torch_epd
    params = orc.init_params(25, 4, 3, 128, 2, 10, 84)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    nodes, ea, s, r, _ = orc.process(scene100k, None, STATS, BOUNDS, 0.015, CART, MAT, CTRL)
    ei = np.stack((s, r))
    with torch.no_grad():
        out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy()
    torch.set_num_threads(max(1, min(32, os.cpu_count() or 1)))
    with torch.no_grad():
        ref = torch_epd.epd_forward({k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}, torch.tensor(nodes, dtype=torch.float64),
                                    torch.tensor(ea, dtype=torch.float64), torch.from_numpy(ei), 2, 10).numpy()
        f32 = torch_epd.epd_forward({k: torch.from_numpy(v) for k, v in params.items()}, torch.from_numpy(nodes), torch.from_numpy(ea),
                                    torch.from_numpy(ei), 2, 10).numpy()
    scale = np.abs(ref).max()
    err, err32 = np.abs(out - ref).max() / scale, np.abs(f32 - ref).max() / scale
    assert err <= max(2.5 * err32, 2.5e-6), (err, err32)
    rms = float(np.sqrt(np.mean(ref ** 2)))
    assert float((np.abs(out - ref) / (1e-5 * np.abs(ref) + 1e-5 * rms)).max()) <= 1.0


def test_forward_target_size_against_the_oracle(dev, scene100k):
    """The north_star target scene (N = 100k, E ~ 1.97 M, hidden 128) through encoder, one processor step and decoder --
    the systolic edge kernel at its full size -- against the numpy oracle on the same graph and weights: 1e-5 relative."""
    err, e = _forward_vs_oracle(dev, scene100k, 128, 80)
    assert e > 1900000
    assert err <= 1e-5, err


def test_forward_target_size_full_depth(dev, scene100k):
    """The benchmarked computation itself: the target scene through ALL TEN message-passing steps (epd_gnn.py:92-94) against
    the float32 host restatement on the same graph and weights: 1e-5 relative (north_star)."""
    err, e = _forward_vs_oracle(dev, scene100k, 128, 83, m_steps=10, host="torch32")
    assert e > 1900000
    assert err <= 1e-5, err


def test_forward_c4_size_against_the_oracle(dev, scene100k):
    """BASELINE config C4 (N = 100k, hidden 256) through encoder, two processor steps and decoder -- the streamed `hm`
    kernels at their full size, the second step on the first one's latents -- against the float32 host restatement: 1e-5
    relative."""
    err, e = _forward_vs_oracle(dev, scene100k, 256, 81, m_steps=2, host="torch32")
    assert e > 1900000
    assert err <= 1e-5, err


def test_rollout_c2_size_against_the_oracle(dev):
    """BASELINE config C2's scene (N = 5k dense, hidden 128, 10 message-passing steps): a 10-step device-resident rollout
    (graph rebuilt every step) against oracle.rollout, the restatement of the reference's cma_objective loop
    (rollout_utils.py:38-61): positions to 5e-6 absolute (positions are O(0.5); one float32 ulp there is 6e-8)."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, scene
    n, steps = 5000, 10
    obs = scene.make_scene(n, seed=11)
    traj = scene.rigid_drift_trajectory(obs, steps, seed=12)
    params = orc.init_params(25, 4, 3, 128, 2, 10, 82)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    eng = RolloutEngine(m, ga, n, device=dev)
    with torch.no_grad():
        final = eng.rollout(_t(obs, dev), _t(traj, dev), horizon=steps).cpu().numpy()
    ref = orc.rollout(params, obs, traj, steps, STATS, BOUNDS, 0.015, CART, MAT, CTRL, 2, 10)
    assert np.isfinite(final).all() and eng.status() > 90000
    # "Flip" against "drift": the same rollout step by step, the radius graph of every step's state compared with the graph of
    # the oracle's state of that step.  Up to the first flipped edge the lists are identical, and afterwards they differ in a
    # handful of edges only (a drifting kernel would lose thousands).
    from gnn_manip_amd import get_connectivity
    state_o = obs.copy()
    state_d = _t(obs, dev).clone()
    eng2 = RolloutEngine(m, ga, n, device=dev)
    eng2.set_scene(state_d)
    first_flip, worst = None, 0
    with torch.no_grad():
        for i in range(steps):
            sd, rd = get_connectivity(state_d[-1][:, 2:5].contiguous(), 0.015, 20)
            so, ro = orc.get_connectivity(state_o[-1][:, 2:5], 0.015, 20)
            a = set(zip(sd.cpu().numpy().tolist(), rd.cpu().numpy().tolist()))
            b = set(zip(so.tolist(), ro.tolist()))
            flips = len(a ^ b)
            worst = max(worst, flips)
            if flips and first_flip is None:
                first_flip = i
            if i == 0:   # the same state: identical lists in identical order (later states differ in the last bits, and two
                np.testing.assert_array_equal(sd.cpu().numpy(), so)   # neighbours at nearly the same distance may swap places)
                np.testing.assert_array_equal(rd.cpu().numpy(), ro)
            eng2.step(state_d, _t(traj[i], dev))
            state_o = orc.rollout(params, state_o, traj[i:i + 1], 1, STATS, BOUNDS, 0.015, CART, MAT, CTRL, 2, 10)
    print(f"C2 rollout: first step with a flipped edge: {first_flip}, most differing edges in a step: {worst} of ~{len(b)}")
    assert first_flip is None or first_flip >= 1   # the initial state is the same: step 0's lists are
    assert worst <= 200, worst
    # The whole final window [k, N, D]: positions and control columns of the last k frames, ids / material untouched.  Ten
    # steps of a random-weight model amplify a last-bit difference wherever a pair sits exactly at the radius / 20th-neighbour
    # boundary (one flipped edge moves two particles by ~1e-5): all but a handful of the 90 000 coordinates must agree to
    # 5e-6, and none may be off by more than 5e-5.
    d = np.abs(final[:, :, 2:8] - ref[:, :, 2:8])
    assert d.max() <= 5e-5, d.max()
    assert (d > 5e-6).mean() <= 2e-4, ((d > 5e-6).sum(), d.max())
    np.testing.assert_array_equal(final[:, :, :2], ref[:, :, :2])


def test_rollout_full_size_state_properties(dev, scene100k):
    """Three device-resident steps at N = 100k: the window shifts bit-exactly, rigid rows land on the scripted pose,
    control columns hold pose - position, everything stays finite, the edge count is the graph's."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, get_connectivity, scene
    ga = GraphBoundedMultimaterialControl(0.015, dict(STATS, acceleration_mean=[0.0, 0.0, 0.0]), CART, MAT, CTRL, BOUNDS)
    params = orc.init_params(25, 4, 3, 128, 2, 10, 78)
    params["decoder.4.weight"] = params["decoder.4.weight"] * 1e-5
    params["decoder.4.bias"] = params["decoder.4.bias"] * 1e-5
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    n = scene100k.shape[1]
    obs = _t(scene100k, dev).clone()
    eng = RolloutEngine(m, ga, n, device=dev)
    n_rigid = eng.set_scene(obs)
    rigid = obs[-1, :, 1] == 1
    assert n_rigid == int(rigid.sum())
    traj = _t(scene.rigid_drift_trajectory(scene100k, 3, seed=9, step_size=1e-5), dev)
    with torch.no_grad():
        for i in range(3):
            before = obs.clone()
            eng.step(obs, traj[i])
            assert torch.equal(obs[:-1, :, 2:5], before[1:, :, 2:5])       # window shift
            assert torch.equal(obs[-1, rigid, 2:5], traj[i])               # scripted pose written back
            assert torch.equal(obs[-2, rigid, 5:8], traj[i] - before[-1, rigid, 2:5])  # control = pose - position
            assert torch.isfinite(obs).all()
    s, _ = get_connectivity(before[-1, :, 2:5], 0.015, 20)
    assert eng.status() == int(s.shape[0])


def test_rollout_full_size_is_invariant_under_particle_numbering(dev, scene100k):
    """A size-independent property at the benchmark's size: the rollout does not depend on how the particles are numbered.
    RolloutEngine.run at N = 100k renumbers its working copy in grid-cell order (default at this size, re-sorted here after every
    two steps) -- the result, returned in the caller's numbering, must be the plain engine's up to the summation order of a
    node's incoming messages, with the same edge count, rigid rows on their own scripted poses and ids / materials untouched."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, scene
    ga = GraphBoundedMultimaterialControl(0.015, dict(STATS, acceleration_mean=[0.0, 0.0, 0.0]), CART, MAT, CTRL, BOUNDS)
    params = orc.init_params(25, 4, 3, 128, 2, 10, 78)
    params["decoder.4.weight"] = params["decoder.4.weight"] * 1e-3
    params["decoder.4.bias"] = params["decoder.4.bias"] * 1e-3
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    n, steps = scene100k.shape[1], 3
    traj = _t(scene.rigid_drift_trajectory(scene100k, steps, seed=9, step_size=1e-5), dev)
    rigid = scene100k[-1, :, 1] == 1
    with torch.no_grad():
        plain = RolloutEngine(m, ga, n, device=dev, renumber=False)
        f0 = plain.rollout(_t(scene100k, dev), traj, horizon=steps)
        e0 = plain.status()
        ren = RolloutEngine(m, ga, n, device=dev)
        assert ren.renumber                                       # "auto" at this size
        ren.RENUMBER_EVERY = 2
        f1, recs = ren.rollout(_t(scene100k, dev), traj, horizon=steps, record=True)
        e1 = ren.status()
    assert e0 == e1
    assert torch.equal(f1[:, :, :2], f0[:, :, :2]) and torch.equal(f1[:, :, :2], _t(scene100k, dev)[:, :, :2])
    assert torch.equal(f1[-1, _t(rigid, dev), 2:5], traj[steps - 1])
    assert torch.equal(recs[-1, :, 2:5], f1[-2, :, 2:5])          # the record of the last step is the frame before the final one
    d = (f1[:, :, 2:8] - f0[:, :, 2:8]).abs()
    assert float(d.max()) <= 2e-6, float(d.max())


def test_batch_invariance_does_not_depend_on_the_batch_size(dev):
    """A block-diagonal batch large enough to cross the node kernels' size threshold by its TOTAL (10 scenes x 5000 = 50 000 nodes
    against 49 152): the kernels are chosen by the size of one graph, so candidate c of the batch still equals candidate c rolled
    out alone bit for bit (round 5 chose by the total: the systolic and the streamed node kernels add a row's terms in different
    orders, and a batch of 10 differed from a batch of 8 in the last bits)."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, scene
    n, steps, b = 5000, 2, 10
    obs = scene.make_scene(n, seed=17)
    trajs = np.stack([scene.rigid_drift_trajectory(obs, steps, seed=300 + c, step_size=2e-4) for c in range(b)])
    params = orc.init_params(25, 4, 3, 128, 2, 10, 85)
    m = EncProcDecGNN(25, 4, 3, 128, 2, 10)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    m = m.to(dev)
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    with torch.no_grad():
        out = RolloutEngine(m, ga, n, device=dev, candidates=b).rollout_candidates(_t(obs, dev), _t(trajs, dev))
        eng1 = RolloutEngine(m, ga, n, device=dev)
        for c in (0, 7, 9):
            one = eng1.rollout(_t(obs, dev), _t(trajs[c], dev), horizon=steps)
            assert torch.equal(out[c], one), (c, float((out[c] - one).abs().max()))


def test_single_pass_scans_over_thousands_of_tiles(dev):
    """The destination sort's in-degree scan (scan_lookback_kernel: decoupled look-back, one launch) far beyond the sizes of the
    benchmark: 3 M nodes = 1465 tiles of 2048, i.e. a look-back that spans many 64-tile looks -- in_ptr read back from the csr
    workspace against cumsum(bincount) -- and the radius graph of 600 k particles (586 tiles of cell counts, 293 of neighbour
    counts) against the oracle's lists, bit for bit."""
    from gnn_manip_amd import get_connectivity
    from gnn_manip_amd.epd_gnn import DstCsr
    g = torch.Generator(device="cpu").manual_seed(5)
    n, e = 3_000_000, 4_000_000
    ei = torch.randint(0, n, (2, e), generator=g, dtype=torch.int64)
    ei[1, : e // 4] = ei[1, : e // 4] % 1000          # a crowd of hubs: long segments, and long runs of empty ones behind them
    csr = DstCsr(ei.to(dev), n)
    assert csr.validate() == e
    in_ptr = csr.ws[256:256 + 4 * (n + 1)].view(torch.int32).cpu().numpy()   # carve_csr: header (one 256-byte slot), then in_ptr[n + 1]
    ref = np.concatenate(([0], np.cumsum(np.bincount(ei[1].numpy(), minlength=n))))
    assert np.array_equal(in_ptr, ref)
    del csr
    rng = np.random.default_rng(6)
    m = 600_000
    pos = rng.uniform(0.1, 0.1 + 0.015 * (m / 5.0) ** (1.0 / 3.0) * 1.6, size=(m, 3)).astype(np.float32)   # mean in-radius count ~5
    s_d, r_d = get_connectivity(_t(pos, dev), 0.015, 20)
    s_o, r_o = orc.get_connectivity(pos, 0.015, 20)
    assert len(s_o) > 2 * m
    assert np.array_equal(s_d.cpu().numpy(), s_o) and np.array_equal(r_d.cpu().numpy(), r_o)
