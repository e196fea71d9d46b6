"""Numeric domain of the fp16-split matrix-pipe kernels (include/gnn_manip_hip.h, "Numeric domain"): the reference computes in
plain float32 (epd_gnn.py:72-84), so a function-preserving rescaling of the weights, or features of very different magnitude,
must not change the 1e-5 parity bar.  What cannot be represented is reported (status() raises, predictions are NaN), never
clamped."""
import numpy as np
import pytest
import torch

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc
from gpu_support import dev, load_model as _model, poison_allocator as _poison, to_dev as _t

pytestmark = pytest.mark.gpu

KW = dict(stats=STATS, bounds=BOUNDS, conn_r=0.015, cartesian_idx=CART, material_idx=MAT)
MLPS = ["encoder.phi_edge", "encoder.phi_node", "processor.0.phi_edge", "processor.1.phi_node", "decoder"]


@pytest.fixture(scope="module")
def graph():
    from gnn_manip_amd import scene
    obs = scene.make_scene(600, seed=31, side=0.07)
    nodes, ea, s, r, _ = orc.process(obs, None, control_idx=CTRL, **KW)
    return nodes, ea, np.stack((s, r))


def _rel(out, ref):
    return np.abs(out - ref).max() / max(np.abs(ref).max(), 1e-30)


@pytest.mark.parametrize("hidden,kernel", [(128, "sys"), (128, "hm"), (64, "hm"), (256, "hm")])
@pytest.mark.parametrize("log2s", [-12, -6, 6, 12])
def test_weight_rescaling_between_linears_is_immaterial(dev, graph, hidden, kernel, log2s):
    """A ReLU MLP is positively homogeneous: (W_l, b_l) * s with W_(l+1) / s is the same function (for a power of two s, bit
    for bit in float32).  The hidden activations between the two Linears are s times larger or smaller -- 2^-12 .. 2^12 --
    which the operand scales must absorb: same 1e-5 bar against the oracle for every MLP of the model and both pairs of
    Linears, and the oracle itself must not move."""
    nodes, ea, ei = graph
    nl, ms = 2, 2
    base = orc.init_params(25, 4, 3, hidden, nl, ms, 300 + hidden)
    ref0 = orc.epd_forward(base, nodes, ea, ei, nl, ms)
    s = np.float32(2.0 ** log2s)
    worst = 0.0
    for mlp in MLPS:
        for l in range(nl):
            p = {k: v.copy() for k, v in base.items()}
            p[f"{mlp}.{2 * l}.weight"] *= s
            p[f"{mlp}.{2 * l}.bias"] *= s
            p[f"{mlp}.{2 * l + 2}.weight"] /= s
            ref = orc.epd_forward(p, nodes, ea, ei, nl, ms)
            assert _rel(ref, ref0) <= 2e-6, (mlp, l)          # the function is unchanged (float32 oracle: rounding only)
            m = _model(p, (25, 4, 3, hidden, nl, ms), dev, kernel)
            with torch.no_grad():
                out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy()
            assert m.status() == ei.shape[1]
            err = _rel(out, ref)
            worst = max(worst, err)
            assert err <= 1e-5, (mlp, l, err)


@pytest.mark.parametrize("hidden,kernel", [(128, "sys"), (64, "hm"), (256, "hm")])
@pytest.mark.parametrize("c", [1e-6, 1e-3, 1e3, 1e4])
def test_feature_magnitude_is_immaterial(dev, graph, hidden, kernel, c):
    """Raw node and edge features of magnitude c (with the encoders' first Linears scaled by 1 / c: the same function) go
    through the per-row power-of-two scale of the encoder kernels: 1e-5 against the float32 oracle for c = 1e-6 .. 1e4."""
    nodes, ea, ei = graph
    nl, ms = 2, 2
    p = orc.init_params(25, 4, 3, hidden, nl, ms, 400 + hidden)
    c32 = np.float32(c)
    p["encoder.phi_node.0.weight"] = (p["encoder.phi_node.0.weight"] / c32).astype(np.float32)
    p["encoder.phi_edge.0.weight"] = (p["encoder.phi_edge.0.weight"] / c32).astype(np.float32)
    nodes_c, ea_c = (nodes * c32).astype(np.float32), (ea * c32).astype(np.float32)
    ref = orc.epd_forward(p, nodes_c, ea_c, ei, nl, ms)
    m = _model(p, (25, 4, 3, hidden, nl, ms), dev, kernel)
    with torch.no_grad():
        out = m.forward(_t(nodes_c, dev), _t(ea_c, dev), _t(ei, dev)).cpu().numpy()
    assert m.status() == ei.shape[1]
    assert _rel(out, ref) <= 1e-5, _rel(out, ref)


def test_rows_of_very_different_magnitude(dev, graph):
    """Every raw feature row gets its own scale: rows whose features differ by ten orders of magnitude inside one tile (and an
    all-zero row) are each as accurate as in float32."""
    nodes, ea, ei = graph
    rng = np.random.Generator(np.random.PCG64(5))
    p = orc.init_params(25, 4, 3, 128, 2, 2, 500)
    nodes_s = (nodes * (10.0 ** rng.uniform(-6, 4, (nodes.shape[0], 1)))).astype(np.float32)
    ea_s = (ea * (10.0 ** rng.uniform(-6, 4, (ea.shape[0], 1)))).astype(np.float32)
    nodes_s[7] = 0.0
    ea_s[11] = 0.0
    ref = orc.epd_forward(p, nodes_s, ea_s, ei, 2, 2)
    for kernel in ("sys", "hm"):
        m = _model(p, (25, 4, 3, 128, 2, 2), dev, kernel)
        with torch.no_grad():
            out = m.forward(_t(nodes_s, dev), _t(ea_s, dev), _t(ei, dev)).cpu().numpy()
        assert m.status() == ei.shape[1]
        assert _rel(out, ref) <= 1e-5, (kernel, _rel(out, ref))


@pytest.mark.parametrize("kernel", ["sys", "hm"])
def test_unrepresentable_latents_are_reported_not_clamped(dev, graph, kernel):
    """Latents enter the operand images at their natural magnitude: a LayerNorm gain of 1e6 in the node encoder puts |h| beyond
    65504.  The float32 reference would stay finite; here the forward must say so -- status() raises, the prediction is NaN --
    instead of returning saturated numbers."""
    from gnn_manip_amd._lib import GMError
    nodes, ea, ei = graph
    p = orc.init_params(25, 4, 3, 128, 2, 2, 600)
    p["encoder.phi_node.5.weight"] = (p["encoder.phi_node.5.weight"] * np.float32(1e6)).astype(np.float32)
    m = _model(p, (25, 4, 3, 128, 2, 2), dev, kernel)
    with torch.no_grad():
        out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev))
    with pytest.raises(GMError, match="fp16 split range"):
        m.status()
    assert torch.isnan(out).all()
    # a healthy forward afterwards is clean again
    q = orc.init_params(25, 4, 3, 128, 2, 2, 600)
    m2 = _model(q, (25, 4, 3, 128, 2, 2), dev, kernel)
    with torch.no_grad():
        out2 = m2.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy()
    assert m2.status() == ei.shape[1] and np.isfinite(out2).all()


def test_deep_mlp_scales_stay_in_range(dev, graph):
    """num_layers = 8 (nine Linears per MLP): the ridden scales are chosen from each Linear's gain, so the operand images stay in
    range however deep the chain; hidden 64, streamed kernels, against the oracle."""
    nodes, ea, ei = graph
    p = orc.init_params(25, 4, 3, 64, 8, 1, 700)
    ref = orc.epd_forward(p, nodes, ea, ei, 8, 1)
    m = _model(p, (25, 4, 3, 64, 8, 1), dev, "hm")
    with torch.no_grad():
        out = m.forward(_t(nodes, dev), _t(ea, dev), _t(ei, dev)).cpu().numpy()
    assert m.status() == ei.shape[1]
    assert _rel(out, ref) <= 2e-5, _rel(out, ref)


@pytest.mark.parametrize("pattern", [float("nan"), float("inf"), 3e38])
def test_results_do_not_depend_on_what_the_workspaces_held(dev, pattern):
    """Every workspace the library is given is uninitialised memory.  A row that is read for nothing must be dropped by a select,
    never by a multiplication with zero (NaN x 0 = NaN, and a NaN operand is flushed to zero by the next ReLU: a wrong, FINITE
    result -- found in the node kernel's stitch of head partials, where rows without one read side row 0).  Each entry point, run
    after the allocator's free blocks were filled with NaN / inf / huge values, must return bit for bit what it returns on clean memory:
    the standalone blocks, the fused forward on both kernel families, a rollout, a training step."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, scene
    torch.manual_seed(5)
    obs = scene.make_scene(900, seed=77, side=0.08)
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    with torch.no_grad():
        nodes, ea, ei, _ = ga.process_collate([(torch.from_numpy(obs).to(dev), torch.zeros(obs.shape[1], 3, device=dev))])
    traj = torch.from_numpy(scene.rigid_drift_trajectory(obs, 2)).to(dev)

    def runs():
        out = {}
        for hid in (128, 64, 256, 100):   # the systolic kernels, the streamed ones at two widths, a zero-padded width
            torch.manual_seed(hid)
            m = EncProcDecGNN(25, 4, 3, hid, 2, 3).to(dev)
            with torch.no_grad():
                out[f"forward{hid}"] = m.forward(nodes, ea, ei).clone()
                h0, e0, _ = m.encoder(nodes, ea, ei)
                h1, e1, _ = m.processor[0](h0, e0, ei)
                out[f"block{hid}"] = torch.cat((h1.flatten(), e1.flatten())).clone()
                if hid == 128:
                    eng = RolloutEngine(m, ga, obs.shape[1], device=dev)
                    out["rollout"] = eng.rollout(torch.from_numpy(obs).to(dev), traj, horizon=2).clone()
                    m.set_edge_kernel("sys_all")   # the systolic node + projection kernels (large graphs take them by themselves)
                    out["forward128_sys_all"] = m.forward(nodes, ea, ei).clone()
                    out["rollout_sys_all"] = eng.rollout(torch.from_numpy(obs).to(dev), traj, horizon=2).clone()
                    m.set_edge_kernel("auto")
            if hid not in (128, 64):      # (the training entry points take the instantiated widths)
                continue
            m.zero_grad()
            m.forward(nodes, ea, ei).square().sum().backward()
            out[f"grads{hid}"] = torch.cat([p.grad.flatten() for p in m.parameters()]).clone()
            m.status()
        from gnn_manip_amd.losses import SamplesLoss
        g = np.random.Generator(np.random.PCG64(9))
        x = torch.from_numpy(g.random((700, 3), dtype=np.float32)).to(dev)
        y = torch.from_numpy(g.random((650, 3), dtype=np.float32) + np.float32(0.1)).to(dev)
        out["sinkhorn"] = SamplesLoss(loss="sinkhorn", p=2, blur=.05)(x, y).reshape(1).clone()
        torch.cuda.synchronize()
        return out

    clean = runs()
    _poison(dev, pattern)
    dirty = runs()
    for k in clean:
        assert torch.isfinite(clean[k]).all(), k
        assert torch.equal(clean[k], dirty[k]), (k, float((clean[k] - dirty[k]).abs().max()))


@pytest.mark.parametrize("hid", [128, 64, 100])
def test_standalone_encoder_turns_a_non_finite_input_row_into_a_nan_row(dev, hid):
    """gm_graph_independent_forward has no header to flag (include/gnn_manip_hip.h): a row with a NaN / inf feature must come out
    NaN in every feature -- the one-instruction ReLU flushes a NaN operand to zero, so the kernels carry a per-row poison term
    from every Linear's accumulators into the LayerNorm -- and every other row must be untouched, bit for bit.  A huge but finite
    feature (1e30) is inside the numeric domain and stays finite."""
    from gnn_manip_amd import EncProcDecGNN
    torch.manual_seed(hid)
    m = EncProcDecGNN(25, 4, 3, hid, 2, 2).to(dev)
    n, e = 300, 2000
    x, ea = torch.randn(n, 25, device=dev), torch.randn(e, 4, device=dev)
    ei = torch.randint(0, n, (2, e), device=dev)
    with torch.no_grad():
        h0, e0, _ = m.encoder(x, ea, ei)
        xb, eb = x.clone(), ea.clone()
        xb[7, 3] = float("nan"); xb[100, 24] = float("inf"); xb[299, 0] = float("-inf"); xb[20, 0] = 1e30
        eb[11, 1] = float("inf"); eb[1999, 3] = float("nan"); eb[64, 0] = -1e30
        h1, e1, _ = m.encoder(xb, eb, ei)
    bad_n, bad_e = [7, 100, 299], [11, 1999]
    assert torch.isnan(h1[bad_n]).all() and torch.isnan(e1[bad_e]).all()
    keep_n = torch.ones(n, dtype=torch.bool, device=dev); keep_n[bad_n + [20]] = False
    keep_e = torch.ones(e, dtype=torch.bool, device=dev); keep_e[bad_e + [64]] = False
    assert torch.equal(h1[keep_n], h0[keep_n]) and torch.equal(e1[keep_e], e0[keep_e])
    assert torch.isfinite(h1[20]).all() and torch.isfinite(e1[64]).all()


def test_entry_points_follow_the_callers_stream(dev):
    """Everything is enqueued on the stream the caller passes (torch's current stream in the host layer): a forward, a rollout and
    a training step issued on a side stream -- with the default stream kept busy by unrelated work -- return the bits of the same
    calls on the default stream."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, RolloutEngine, scene
    obs = scene.make_scene(1200, seed=78, side=0.085)
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    with torch.no_grad():
        nodes, ea, ei, _ = ga.process_collate([(torch.from_numpy(obs).to(dev), torch.zeros(obs.shape[1], 3, device=dev))])
    traj = torch.from_numpy(scene.rigid_drift_trajectory(obs, 2)).to(dev)

    def runs():
        torch.manual_seed(11)
        m = EncProcDecGNN(25, 4, 3, 128, 2, 3).to(dev)
        out = {}
        with torch.no_grad():
            out["forward"] = m.forward(nodes, ea, ei).clone()
            out["rollout"] = RolloutEngine(m, ga, obs.shape[1], device=dev).rollout(torch.from_numpy(obs).to(dev), traj, horizon=2).clone()
        m.forward(nodes, ea, ei).square().sum().backward()
        out["grads"] = torch.cat([p.grad.flatten() for p in m.parameters()]).clone()
        return out

    ref = runs()
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    busy = torch.randn(4096, 4096, device=dev)
    for _ in range(20):
        busy = busy @ busy * 1e-3          # the default stream has work queued while the side stream runs
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = runs()
    side.synchronize()
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(ref[k], got[k]), (k, float((ref[k] - got[k]).abs().max()))


def test_model_loaded_on_one_stream_is_usable_from_others(dev):
    """A handle's weight copy and its operand images are queued on the stream of the call that triggers them; a call on ANOTHER
    stream waits for them through an event recorded behind the last pack (csrc/model.h: `ready`), not through luck.  The weights
    are loaded (training forward) on the default stream behind a long queue of unrelated work, the first inference -- which packs
    the inference images -- runs on a side stream, a second inference on a third stream right after it, none of them synchronised
    with the others: all three must return the bits of the same calls made one after the other on one stream."""
    from gnn_manip_amd import EncProcDecGNN, GraphBoundedMultimaterialControl, scene
    obs = scene.make_scene(900, seed=79, side=0.08)
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    with torch.no_grad():
        nodes, ea, ei, _ = ga.process_collate([(torch.from_numpy(obs).to(dev), torch.zeros(obs.shape[1], 3, device=dev))])

    def model():
        torch.manual_seed(12)
        return EncProcDecGNN(25, 4, 3, 128, 2, 3).to(dev)

    m = model()
    ref_t = m.forward(nodes, ea, ei).detach().clone()
    with torch.no_grad():
        ref_i = m.forward(nodes, ea, ei).clone()
    torch.cuda.synchronize()
    m = model()
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    busy = torch.randn(4096, 4096, device=dev)
    for _ in range(30):
        busy = busy @ busy * 1e-3                      # the weight copy + training pack queue up behind this
    got_t = m.forward(nodes, ea, ei).detach()          # default stream: loads the weights, packs the training streams
    with torch.cuda.stream(s1), torch.no_grad():
        got_1 = m.forward(nodes, ea, ei)               # side stream: must wait for the load, then packs the inference images
    with torch.cuda.stream(s2), torch.no_grad():
        got_2 = m.forward(nodes, ea, ei)               # third stream: must wait for s1's pack
    torch.cuda.synchronize()
    assert torch.equal(got_t, ref_t) and torch.equal(got_1, ref_i) and torch.equal(got_2, ref_i)
