"""Every LayerNorm implementation of the library against float64 where eps and the centring decide the answer (cases, references and
the figures of every regime: layernorm_cases.py; that the cases can tell a wrong treatment from a right one:
test_layernorm_cases.py).

  forward      EncProcDecGNN.forward without autograd: the systolic processor edge kernel, the systolic node and projection launches
               fused and apart (hidden 128, num_layers 2, edge kernels "sys" / "hm" / "sys_all"), the streamed kernels at hidden 64,
               256, 100 and at num_layers 3 -- every case of the table.  (The edge ENCODER of these forwards is the streamed kernel:
               the module hands edge_attr over in the caller's order.)
  sorted       gm_epd_forward with edge_attr already in destination order, as a rollout step hands it over: the only route to the
               systolic edge encoder (hedge.hip: sys_enc_kernel, the ring-in-LDS form with eps in the accumulators' scale) and to the
               encoder image of pack_h3_kernel -- every case of the table, "sys" and "sys_all"
  blocks       GraphIndependent / InteractionNetwork built from Sequentials whose LayerNorms carry the case's eps, hidden 128 and 100;
               the encoder also on raw features times 1e-4 and 1e3 (the per-row scale enters eps t^2)
  f16          set_precision("f16") held to precision_cases' envelope, its restatement now taking eps
  training     one L1 step, forward and every parameter gradient by tests/yardstick.py, hidden 64 / 128 / 256 / 100, num_layers 3
  rollout      one RolloutEngine.step against the numpy oracle's rollout at the rollout tests' bar

Forward bar: max |out - ref64| <= max(1e-5, 4 e32) max |ref64|, e32 the error of the same computation in torch float32
(layernorm_cases.forward_bar); every case prints err, e32 and the bar.  The e32 term passes 1e-5 only on offset(c) (values in
layernorm_cases' docstring).  Measured on an MI355X, library against float32 torch, over every route, width and block:
  offset(256)   inference 3e-7 .. 1.1e-6                                              against 3.0e-5 .. 4.9e-4
                training forward 4e-7 .. 9e-7, 2.8e-5 at hidden 100 (the host centres in float32)    against 1.7e-4 .. 4.9e-4
  offset(8)     inference 4e-7 .. 1.3e-6, training forward 8e-7 .. 2.7e-6             against 9e-7 .. 1.3e-5
so up to several hundred times more accurate than the bar's reference: the coarse part of the mean is taken off the weights,
unrounded, when they are packed.  The systolic edge encoder (sorted attributes): 5.7e-7 .. 1.2e-6 over the whole table.  Everything
else is within 0.25 of the 1e-5 bar (worst: 2.3e-6, training forward at hidden 256 on shrunk14-all).  Gradients: 8 of the 55
training cases go beyond the plain yardstick and are within it with the ReLU flip allowance, the closest at 0.98 of it (hidden 256,
plain weights at eps = 1e-2, decoder.2.weight).  f16: 0.97 .. 1.04 of its restatement's error.  The bar is not tightened to these
figures."""
import numpy as np
import pytest
import torch

import layernorm_cases as lc
import precision_cases as pc
import yardstick
from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc
from gpu_support import compare_parameter_gradients, dev, graph_attr, l1_step, load_model, to_dev as _t

pytestmark = pytest.mark.gpu


def _set_eps(module, eps):
    for m in module.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.eps = eps


def _model(hidden, nl, name, dev, kernel=None, precision=None, eps=None):
    """The case's parameters through gpu_support.load_model, every LayerNorm's eps set before the first call."""
    m = load_model(lc.case_params(hidden, nl, name), lc.dims(hidden, nl), dev, kernel, precision)
    _set_eps(m, lc.BY_NAME[name].eps if eps is None else eps)
    return m


def _held(fails, what, got, r64, r32):
    """One output against the forward bar: prints err, e32 and the bar; appends to `fails` what misses it."""
    e32 = lc.rel_err(r32, r64)
    bar = lc.forward_bar(e32)
    finite = bool(np.isfinite(got).all())
    err = lc.rel_err(got, r64) if finite else float("inf")
    print(f"[layernorm] {what}: err {err:.2e} e32 {e32:.2e} bar {bar:.2e}" + ("  (the e32 term decides)" if 4 * e32 > 1e-5 else ""))
    if not (finite and err <= bar):
        fails.append((what, err, bar))
    return err


# ================================================================== inference forward
GROUPS = {"plain": [c.name for c in lc.CASES if c.regime == "plain"],
          "shrunk": [c.name for c in lc.CASES if c.regime == "shrunk" and c.eps == 1e-5],
          "shrunk_tiny_eps": [c.name for c in lc.CASES if c.regime == "shrunk" and c.eps == 1e-12],
          "offset": [c.name for c in lc.CASES if c.regime == "offset"],   # bar above 1e-5 by its e32 term: offset8-enc_node 3.6e-5,
          #                                   offset8-all 4.0e-5, offset256-* 1.2e-4 .. 1.1e-3 at hidden 128 (printed per case)
          "flat": [c.name for c in lc.CASES if c.regime == "flat"]}
assert sorted(n for g in GROUPS.values() for n in g) == sorted(c.name for c in lc.CASES)
# (hidden, num_layers, edge kernel): 5, 6, 7 of test_gpu_parity.py at the systolic kernels' shape, the streamed kernels elsewhere
FORWARD = [(128, 2, "sys"), (128, 2, "hm"), (128, 2, "sys_all"), (64, 2, "hm"), (256, 2, "hm"), (100, 2, "hm"), (128, 3, "hm")]


@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("hidden,nl,kernel", FORWARD)
def test_forward_against_float64(dev, hidden, nl, kernel, group):
    nodes, ea, ei = (_t(a, dev) for a in lc.scene())
    fails = []
    print()
    for name in GROUPS[group]:
        r64, r32, _ = lc.forward_reference(hidden, nl, name)
        m = _model(hidden, nl, name, dev, kernel)
        for fusion in ((True, False) if kernel in ("sys", "sys_all") else (True,)):
            m.set_node_fusion(fusion)
            with torch.no_grad():
                out = m.forward(nodes, ea, ei).cpu().numpy()
            assert m.status() == ei.shape[1]
            _held(fails, f"forward h{hidden} l{nl} {kernel} fusion {int(fusion)} {name}", out, r64, r32)
    assert not fails, fails


# ================================================================== the fused forward on sorted edge attributes
@pytest.mark.parametrize("group", list(GROUPS))
@pytest.mark.parametrize("kernel", ["sys", "sys_all"])
def test_forward_on_sorted_attributes_against_float64(dev, kernel, group):
    """sys_enc_kernel runs only where the fused forward is told that edge_attr is in the csr's order (model.hip: route_forward),
    which EncProcDecGNN.forward never says.  The scene's edges sorted by destination on the host are in that order already, so
    gm_epd_forward takes them with edge_attr_is_csr_order = 1.  The references are those of the unsorted scene: a prediction does not
    depend on the order of the edges.  On the plain weights the result must differ in its bits from EncProcDecGNN.forward on the same
    edges -- the same kernels but for the edge encoder -- which says that another encoder ran."""
    import ctypes as C
    from gnn_manip_amd._lib import ModelDesc, check, current_stream, lib, ptr
    from gnn_manip_amd.epd_gnn import DstCsr
    from gnn_manip_amd.graph import _ws
    hidden, nl = 128, 2
    nodes, ea, ei = (_t(a, dev) for a in lc.scene_sorted())
    n, e = nodes.shape[0], ea.shape[0]
    L = lib()
    fails = []
    print()
    for name in GROUPS[group]:
        r64, r32, _ = lc.forward_reference(hidden, nl, name)
        m = _model(hidden, nl, name, dev, kernel)
        csr = DstCsr(ei, n)
        d = ModelDesc(*m.model_desc())
        fws = _ws(L.gm_forward_workspace_bytes(C.byref(d), n, e), dev)
        out = torch.empty((n, 3), dtype=torch.float32, device=dev)
        check(L.gm_epd_forward(m.device_handle(dev), ptr(nodes), n, ptr(ea), 1, ptr(csr.ws), e, ptr(out), ptr(fws), fws.numel(), current_stream(dev)))
        assert csr.validate() == e
        _held(fails, f"sorted attributes h{hidden} l{nl} {kernel} {name}", out.cpu().numpy(), r64, r32)
        if group == "plain":
            with torch.no_grad():
                assert not yardstick.same_bits(m.forward(nodes, ea, ei), out), name
    assert not fails, fails


# ================================================================== the stand-alone blocks
def _sequential(params, prefix, fin, hidden, nl, eps, dev):
    from gnn_manip_amd import EncProcDecGNN
    seq = EncProcDecGNN._build_mlp(fin, hidden, hidden, nl, norm=True)
    seq.load_state_dict({k[len(prefix) + 1:]: torch.from_numpy(np.array(v)) for k, v in params.items() if k.startswith(prefix + ".")}, strict=True)
    seq[-1].eps = eps
    return seq.to(dev)


def _is_bias(out, beta):
    return yardstick.same_bits(out, np.broadcast_to(np.asarray(beta, np.float32), out.shape))


@pytest.mark.parametrize("hidden", [128, 100])
def test_encoder_block_against_float64(dev, hidden):
    """GraphIndependent on the raw features as they are and times 1e-4 / 1e3 with the first Linears scaled inversely (float32): the
    encoder kernels give every row its own power-of-two scale, which then enters eps t^2.  flat(0): the accumulators are exactly
    zero, so the outputs are the LayerNorm's bias bit for bit."""
    from gnn_manip_amd import GraphIndependent
    nl = 2
    fails = []
    print()
    for c in lc.ALL_MLPS:
        for scale in (1.0, 1e-4, 1e3):
            p, nodes, ea = lc.feature_scaled(lc.case_params(hidden, nl, c.name), lc.scene()[0], lc.scene()[1], scale)
            blk = GraphIndependent(phi_edge=_sequential(p, "encoder.phi_edge", 4, hidden, nl, c.eps, dev),
                                   phi_node=_sequential(p, "encoder.phi_node", 25, hidden, nl, c.eps, dev))
            with torch.no_grad():
                h, e, _ = blk(_t(nodes, dev), _t(ea, dev))
            h, e = h.cpu().numpy(), e.cpu().numpy()
            (h64, e64), (h32, e32) = lc.encoder_reference(hidden, nl, c.name, scale)
            _held(fails, f"encoder h{hidden} features x {scale:g} {c.name}: h", h, h64, h32)
            _held(fails, f"encoder h{hidden} features x {scale:g} {c.name}: e", e, e64, e32)
            if c.regime == "flat" and c.arg == 0:
                assert _is_bias(h, p[f"encoder.phi_node.{2 * nl + 1}.bias"]) and _is_bias(e, p[f"encoder.phi_edge.{2 * nl + 1}.bias"]), (c.name, scale)
    assert not fails, fails


@pytest.mark.parametrize("hidden", [128, 100])
def test_processor_block_against_float64(dev, hidden):
    """InteractionNetwork (no residual) on seeded latents and the scene's edges; flat(0): both outputs are the LayerNorm's bias bit
    for bit."""
    from gnn_manip_amd import InteractionNetwork
    nl = 2
    h_in, e_in = lc.block_inputs(hidden)
    ei = lc.scene()[2]
    fails = []
    print()
    for c in lc.ALL_MLPS:
        p = lc.case_params(hidden, nl, c.name)
        blk = InteractionNetwork(phi_edge=_sequential(p, "processor.0.phi_edge", 3 * hidden, hidden, nl, c.eps, dev),
                                 phi_node=_sequential(p, "processor.0.phi_node", 2 * hidden, hidden, nl, c.eps, dev))
        with torch.no_grad():
            h, e, _ = blk(_t(h_in, dev), _t(e_in, dev), _t(ei, dev))
        h, e = h.cpu().numpy(), e.cpu().numpy()
        (h64, e64), (h32, e32) = lc.block_reference(hidden, nl, c.name)
        _held(fails, f"block h{hidden} {c.name}: h'", h, h64, h32)
        _held(fails, f"block h{hidden} {c.name}: e'", e, e64, e32)
        if c.regime == "flat" and c.arg == 0:
            assert _is_bias(h, p[f"processor.0.phi_node.{2 * nl + 1}.bias"]) and _is_bias(e, p[f"processor.0.phi_edge.{2 * nl + 1}.bias"]), c.name
    assert not fails, fails


def test_blocks_refuse_layer_norms_that_disagree(dev):
    from gnn_manip_amd import GraphIndependent, InteractionNetwork
    p = lc.case_params(128, 2, "plain-all-eps1e-05")
    nodes, ea, ei = (_t(a, dev) for a in lc.scene())
    enc = GraphIndependent(phi_edge=_sequential(p, "encoder.phi_edge", 4, 128, 2, 1e-5, dev), phi_node=_sequential(p, "encoder.phi_node", 25, 128, 2, 1e-3, dev))
    with pytest.raises(ValueError, match="1e-05 and 0.001"), torch.no_grad():
        enc(nodes, ea)
    blk = InteractionNetwork(phi_edge=_sequential(p, "processor.0.phi_edge", 384, 128, 2, 1e-2, dev),
                             phi_node=_sequential(p, "processor.0.phi_node", 256, 128, 2, 1e-5, dev))
    with pytest.raises(ValueError, match="0.01 and 1e-05"), torch.no_grad():
        blk(_t(lc.block_inputs(128)[0], dev), _t(lc.block_inputs(128)[1], dev), ei)


# ================================================================== the fp16 mode
@pytest.mark.parametrize("kernel", ["sys_all", "hm"])
@pytest.mark.parametrize("name", ["shrunk7-all-eps1e-05", "offset8-all-eps1e-05", "plain-all-eps0.01"])
def test_f16_mode_in_the_envelope_of_its_restatement(dev, name, kernel):
    """precision_cases' rule B on these parameters and this eps: err(x) = max |x - ref64| / max(max |ref64|, 1e-3); the device within
    err(restatement with rounded operands) / 4 .. 4 err(restatement)."""
    hidden, nl = 128, 2
    c = lc.BY_NAME[name]
    ref, err_r = pc.b_reference(lc.case_params(hidden, nl, name), *lc.scene(), nl, lc.M_STEPS, ln_eps=c.eps)
    m = _model(hidden, nl, name, dev, kernel, "f16")
    nodes, ea, ei = (_t(a, dev) for a in lc.scene())
    with torch.no_grad():
        out = m.forward(nodes, ea, ei).cpu().numpy()
    assert m.status() == ei.shape[1] and np.isfinite(out).all()
    err_g = pc.max_err(out, ref, pc.B_FLOOR)
    print(f"\n[layernorm] f16 {kernel} {name}: err(f16 forward) {err_g:.2e}, err(restatement) {err_r:.2e}, ratio {err_g / err_r:.2f}")
    assert err_r / 4 <= err_g <= 4 * err_r, (name, err_g, err_r)


# ================================================================== training
TRAIN = [(64, 2), (128, 2), (256, 2), (100, 2), (128, 3)]


@pytest.mark.parametrize("name", [c.name for c in lc.ALL_MLPS])
@pytest.mark.parametrize("hidden,nl", TRAIN)
def test_training_step_against_float64(dev, hidden, nl, name):
    """One L1 step (csrc/train.hip: layer_norm_tape and the LayerNorm backward): prediction and loss at the forward bar, every
    parameter gradient by the yardstick, the references and the ReLU flip allowance evaluated with the case's eps.  Hidden 100 runs
    zero-padded at 128 with eps' = eps Hv / Hp and gamma' = gamma sqrt(Hv / Hp) written by the host: eps = 1e-2 and 1.0 on the plain
    weights are where a wrong eps' shows."""
    c = lc.BY_NAME[name]
    p = lc.case_params(hidden, nl, name)
    nodes, ea, ei = lc.scene()
    target = lc.target()
    m = _model(hidden, nl, name, dev)
    out, loss = l1_step(m, nodes, ea, ei, target, dev)
    ref_out, ref_loss, g64, g32 = lc.gradient_reference(hidden, nl, name)
    out32 = lc.torch_forward(p, nodes, ea, ei, nl, lc.M_STEPS, c.eps, torch.float32)
    fails = []
    print()
    _held(fails, f"training forward h{hidden} l{nl} {name}", out.detach().cpu().numpy(), ref_out, out32)
    assert not fails, fails
    bar = lc.forward_bar(lc.rel_err(out32, ref_out))
    assert abs(float(loss.detach()) - ref_loss) <= bar * abs(ref_loss), ("loss", float(loss.detach()), ref_loss)
    worst, worst2 = compare_parameter_gradients(m, p, nodes, ea, ei, target, nl, lc.M_STEPS, g64, g32, ln_eps=c.eps)
    print(f"[layernorm] training gradients h{hidden} l{nl} {name}: worst err / tol {worst[1]:.3f} at {worst[0]} (err {worst[2]:.2e}, tol {worst[3]:.2e})"
          + ("" if worst2 is None else f"; with the ReLU flip allowance {worst2[1]:.3f} at {worst2[0]}"))


# ================================================================== one rollout step
def test_rollout_step_with_shrunk_weights_and_a_large_eps(dev):
    """RolloutEngine.step at hidden 128, shrunk(10) in every MLP, eps = 1e-2 (variance / eps about 3e-7: the latents are z / sqrt(eps))
    against the numpy oracle's rollout with the same eps: positions and controls to 5e-6, the rollout tests' bar.  A step moves a
    position by its prediction times the acceleration's deviation, 3e-4: the oracle at eps = 1e-5 is itself only 2e-6 away, inside
    that bar.  So the step's prediction is held as well, at the forward bar against float64 on the step's own features -- there eps
    = 1e-5 is 0.08 of the maximum away (the device's prediction: 5.6e-7)."""
    from gnn_manip_amd import RolloutEngine, scene
    hidden, nl, eps = 128, 2, 1e-2
    name = "shrunk10-all-eps1e-05"
    p = lc.case_params(hidden, nl, name)
    obs = scene.make_scene(600, seed=3, side=0.07)
    traj = scene.rigid_drift_trajectory(obs, 1)
    m = _model(hidden, nl, name, dev, eps=eps)
    eng = RolloutEngine(m, graph_attr(0.015), obs.shape[1], device=dev)
    a = _t(obs, dev)
    assert eng.set_scene(a) == traj.shape[1]
    pred = torch.empty((obs.shape[1], 3), dtype=torch.float32, device=dev)
    with torch.no_grad():
        eng.step(a, _t(traj[0], dev), pred_out=pred)
    assert eng.status() > 0
    got = a.cpu().numpy()
    seen = {}

    def forward_fn(n, e, i):
        seen.update(nodes=n, ea=e, ei=i)
        return orc.epd_forward(p, n, e, i, nl, lc.M_STEPS, ln_eps=eps)

    ref = orc.rollout(p, obs, traj, 1, STATS, BOUNDS, 0.015, CART, MAT, CTRL, nl, lc.M_STEPS, forward_fn=forward_fn)
    r64, r32, at_default = (lc.torch_forward(p, seen["nodes"], seen["ea"], seen["ei"], nl, lc.M_STEPS, e, dt)
                            for e, dt in ((eps, torch.float64), (eps, torch.float32), (1e-5, torch.float64)))
    fails = []
    print()
    _held(fails, "rollout step: prediction", pred.cpu().numpy(), r64, r32)
    assert not fails, fails
    print(f"[layernorm] rollout step: the prediction at eps 1e-5 is {lc.rel_err(at_default, r64):.2e} of the maximum away")
    assert lc.rel_err(at_default, r64) > 1e-2
    default = orc.rollout(p, obs, traj, 1, STATS, BOUNDS, 0.015, CART, MAT, CTRL, nl, lc.M_STEPS)
    err = np.abs(got[:, :, 2:8] - ref[:, :, 2:8]).max()
    print(f"[layernorm] rollout step: max |state - oracle| {err:.2e} (bar 5e-6); the oracle at eps 1e-5 is {np.abs(default[:, :, 2:8] - ref[:, :, 2:8]).max():.2e} away")
    np.testing.assert_allclose(got[:, :, 2:8], ref[:, :, 2:8], rtol=0, atol=5e-6)
    np.testing.assert_array_equal(got[:, :, :2], ref[:, :, :2])


# ================================================================== one common eps through the module's life
def test_a_common_eps_survives_state_dict_trainer_and_inference(dev):
    """A model whose LayerNorms all carry eps = 1e-3: state_dict() -> a second model with the same eps gives the same bits; the
    library trainer built on it trains with that eps (its evaluation is the module's own prediction), sync_module brings the
    weights back without touching eps, and inference afterwards is the float64 forward of the trained weights at that eps."""
    from gnn_manip_amd import Trainer, train
    hidden, nl, eps = 64, 2, 1e-3
    name = "shrunk7-all-eps1e-05"
    nodes, ea, ei = lc.scene()
    batch = tuple(_t(a, dev) for a in (nodes, ea, ei, lc.target()))
    m = _model(hidden, nl, name, dev, eps=eps)
    with torch.no_grad():
        out0 = m.forward(*batch[:3]).clone()
    twin = _model(hidden, nl, "plain-all-eps1e-05", dev, eps=eps)
    twin.load_state_dict(m.state_dict())
    with torch.no_grad():
        assert yardstick.same_bits(twin.forward(*batch[:3]), out0)
    assert m.model_desc()[6] == twin.model_desc()[6] == eps
    p0 = lc.case_params(hidden, nl, name)
    r64 = lc.torch_forward(p0, nodes, ea, ei, nl, lc.M_STEPS, eps, torch.float64)
    r32 = lc.torch_forward(p0, nodes, ea, ei, nl, lc.M_STEPS, eps, torch.float32)
    at_default = lc.torch_forward(p0, nodes, ea, ei, nl, lc.M_STEPS, 1e-5, torch.float64)
    fails = []
    print()
    _held(fails, "common eps 1e-3, before training", out0.cpu().numpy(), r64, r32)
    assert lc.rel_err(at_default, r64) > 1e-2        # and eps = 1e-5 would be somewhere else
    t = Trainer(m, lr=1e-3)
    t.evaluate(*batch)
    want = float(np.abs(out0.cpu().numpy().astype(np.float32) - lc.target()).astype(np.float64).sum() / nodes.shape[0])
    assert abs(float(t.last_loss) - want) <= 1e-5 * want, (float(t.last_loss), want)
    for _ in range(2):
        t.step(*batch)
    t.sync_module()
    assert all(mod.eps == eps for mod in m.modules() if isinstance(mod, torch.nn.LayerNorm)) and m.model_desc()[6] == eps
    trained = {k: w.cpu().numpy() for (k, _), w in zip(m.named_parameters(), t.export(train.PARAMS))}
    assert all(np.array_equal(trained[k], v.detach().cpu().numpy()) for k, v in m.named_parameters())
    assert any(not np.array_equal(trained[k], p0[k]) for k in p0)
    with torch.no_grad():
        out1 = m.forward(*batch[:3]).cpu().numpy()
    t64 = lc.torch_forward(trained, nodes, ea, ei, nl, lc.M_STEPS, eps, torch.float64)
    t32 = lc.torch_forward(trained, nodes, ea, ei, nl, lc.M_STEPS, eps, torch.float32)
    _held(fails, "common eps 1e-3, after two trainer steps and sync_module", out1, t64, t32)
    t.status()
    assert not fails, fails
