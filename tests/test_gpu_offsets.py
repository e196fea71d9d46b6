"""The kernels across the 2 GiB and 4 GiB buffer-offset boundaries (tests/offset_cases.py: block-diagonal graphs of T small copies,
every copy held to its class's float64 reference).

Every model is num_layers = 2, m_steps = 1 (F1s2 / F3s2: 2) with oracle.init_params weights.  The bars are the project's own: the forward bar of
conftest.assert_forward_close (1e-5: against the tensor's maximum and per element), applied to every copy against its class
reference (`_assert_copies_close` is that rule on the device, one reshape per class instead of T calls; the first and the last
copy also go through assert_forward_close itself), and the gradient rule of tests/yardstick.py (GRAD_TOL, 4 x float32 torch's own
error, the ReLU flip allowance as the only fallback).

  case  path                                   what crosses
  F1    forward, 'hm', hidden 256              edge rows in [2, 4) GiB
  F1s2  the same, two message-passing steps    ... and the first step STORES its e + e' rows (the last step of a forward discards them)
  F2    forward, 'hm', hidden 256              edge rows beyond 4 GiB
  F2c   forward, 'hm', hidden 256              edge rows beyond 8 GiB: row * hidden beyond 2^31 FLOATS (an index formed in int wraps)
  F3    forward, 'auto' (systolic), hidden 128 edge rows in [2, 4) GiB
  F3s2  the same, two message-passing steps    ... and sys_edge_kernel's e_out epilogue runs
  F4    forward, 'auto', hidden 128            edge rows beyond 4 GiB, edge_sys_fits still true
  F5    forward, 'auto', sparse family         the LAST tiling edge_sys_fits admits: P rows gathered, side-buffer rows stored at 32-bit
                                               offsets in [2, 4) GiB by the systolic edge kernel
  F5b   the same, 4108 copies                  P table just below 4 GiB, agg + side buffer beyond: the streamed edge kernel
  F6    the same, 4109 copies                  P table beyond 4 GiB, agg beyond 2 GiB: the streamed edge kernel
  B1    InteractionNetwork.forward, hidden 256 edge rows in [2, 4) GiB read through the eid gather (edges in a random order),
                                               e_out row for row in the caller's order
  T0    training step, hidden 128              tapes in [2, 4) GiB
  T1    training step, hidden 256, inputs too  edge rows 3.97 GiB; the dxidx stores of d_edge_attr
  T2    the same, E >= 4 194 304               edge rows beyond 4 GiB: inside the fused step's range (e < 2^31 / hidden), which has
                                               no hidden-wide indexed operand -- held to the same yardstick as T1
  T2g   InteractionNetwork under autograd      the 4 GiB guard of the indexed weight-gradient operand (csrc/train.hip
                                               wgrad_enqueue), where it applies: GMError GM_ERR_UNSUPPORTED, no .grad touched
  T1g   InteractionNetwork under autograd      just under that guard: the indexed operand's 32-bit row offsets and the dxidx stores of
                                               de_in in [2, 4) GiB
  R1    RolloutEngine(candidates=211), 1 step  the step's fused graph / sort / feature / forward chain at > 2 GiB of edge rows

The routes of F5 / F5b / F6 are INFERRED from edge_sys_fits restated on the sizes passed (offset_cases.edge_sys_fits, asserted per
case before the GPU is touched), not observed: the model's profile counters count the systolic and the streamed edge launch under the
same kind.  What is observed is that all three agree with the float64 reference on either side of the switch.

Every case sizes its need from the library's own *_bytes functions plus its tensors and FAILS (it does not skip) when the device has
less free; it frees what it allocated and empties torch's cache at the end."""
import ctypes as C
import functools
import gc

import numpy as np
import pytest
import torch

import offset_cases as oc
from conftest import BOUNDS, CART, CTRL, MAT, STATS, assert_forward_close
from oracle import epd_oracle as orc
from oracle import torch_epd
import yardstick
from gpu_support import dev, load_model
from grad_cases import flip_allowance
from yardstick import GRAD_TOL

pytestmark = pytest.mark.gpu

NL, MS = 2, 1
SEEDS = {128: 6128, 256: 6256}
GIB = float(1 << 30)


@pytest.fixture(autouse=True)
def _release_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _dims(hidden, ms=MS):
    return (25, 4, 3, hidden, NL, ms)


@functools.lru_cache(maxsize=None)
def _params(hidden, ms=MS):
    return orc.init_params(*_dims(hidden, ms), SEEDS[hidden] + 1000 * (ms - MS))


def _family(name):
    return oc.dense_family() if name == "dense" else oc.sparse_family()


def _model(hidden, dev, ms=MS):
    return load_model(_params(hidden, ms), _dims(hidden, ms), dev)


@functools.lru_cache(maxsize=None)
def _forward_refs(family, hidden, ms=MS):
    """float64 prediction of every class (oracle/torch_epd.py), once per module."""
    fam = _family(family)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in _params(hidden, ms).items()}
    with torch.no_grad():
        return [torch_epd.epd_forward(p, torch.tensor(fam.nodes[c], dtype=torch.float64), torch.tensor(fam.edge_attr[c], dtype=torch.float64),
                                      torch.tensor(fam.edge_index[c]), NL, ms).numpy() for c in range(oc.K)]


@functools.lru_cache(maxsize=None)
def _grad_refs(family, hidden, dtype_name):
    fam = _family(family)
    return oc.class_grad_refs(fam, _params(hidden), oc.class_targets(fam), NL, MS, dtype=getattr(torch, dtype_name), inputs=True)


def _need(dev, what, **parts):
    """Fail (not skip) when the device has less free memory than the case needs."""
    need = sum(int(v) for v in parts.values())
    free, total = torch.cuda.mem_get_info(dev)
    detail = ", ".join(f"{k} {v / GIB:.2f}" for k, v in parts.items())
    print(f"[offsets] {what}: needs {need / GIB:.2f} GiB ({detail}); device has {free / GIB:.1f} of {total / GIB:.1f} GiB free")
    assert free >= need, f"{what}: needs {need / GIB:.2f} GiB of device memory ({detail}), {free / GIB:.2f} GiB are free"


def _lib_desc(m):
    from gnn_manip_amd._lib import ModelDesc, lib
    return lib(), ModelDesc(*m.model_desc())


def _case(name):
    case = oc.gpu_cases()[name].check()
    print("\n[offsets] regime " + case.describe())
    return case


def _assert_copies_close(view, refs, what, rel=1e-5):
    """conftest.assert_forward_close of every copy against its class reference: view [T, rows, w] on the device (copy t holds class
    t mod K), refs K x [rows, w] float64.  Returns the worst (max-normalised error, per-element ratio) over the classes."""
    assert bool(torch.isfinite(view).all()), what
    t = view.shape[0]
    worst_max, worst_el = 0.0, 0.0
    for c in range(min(oc.K, t)):
        ref = torch.from_numpy(np.ascontiguousarray(refs[c], np.float64)).to(view.device)
        err = (view[c::oc.K].double() - ref[None]).abs().amax(dim=0)       # the worst copy of the class, element by element
        scale = float(ref.abs().max())
        rms = float(ref.pow(2).mean().sqrt())
        e_max = float(err.max()) / scale
        e_el = float((err / (rel * ref.abs() + rel * rms)).max())
        copy = int((view[c::oc.K].double() - ref[None]).abs().amax(dim=(1, 2)).argmax()) * oc.K + c
        assert e_max <= rel, (what, "class", c, "worst copy", copy, "max-normalised", e_max)
        assert e_el <= 1.0, (what, "class", c, "worst copy", copy, "per-element bound", e_el)
        worst_max, worst_el = max(worst_max, e_max), max(worst_el, e_el)
    for copy in (0, t - 1):   # the rule itself, on the two ends of the array
        assert_forward_close(view[copy].cpu().numpy(), refs[copy % oc.K], what=f"{what} copy {copy}")
    return worst_max, worst_el


def _assert_edge_rows_close(e_out, refs, fam, t, what, rel=1e-5):
    """conftest.assert_forward_close of every copy's edge rows against its class reference: e_out [E, w] on the device in the
    copy-by-copy layout, refs K x [e0_c, w] float64.  A period at a time (100 MB of float64)."""
    dev = e_out.device
    assert bool(torch.isfinite(e_out).all()), what
    per_ref = torch.from_numpy(np.concatenate(refs)).to(dev)   # one period [sum e0, w]
    per = per_ref.shape[0]
    row_scale = torch.cat([torch.full((fam.e0[c],), float(np.abs(refs[c]).max()), dtype=torch.float64, device=dev) for c in range(oc.K)])[:, None]
    row_rms = torch.cat([torch.full((fam.e0[c],), float(np.sqrt(np.mean(refs[c] ** 2))), dtype=torch.float64, device=dev) for c in range(oc.K)])[:, None]
    full, rem = divmod(t, oc.K)
    tail = sum(fam.e0[:rem])
    assert e_out.shape[0] == full * per + tail
    w_max, w_el = 0.0, 0.0
    for q in range(full + (1 if rem else 0)):
        rows_q = per if q < full else tail
        err = (e_out[q * per:q * per + rows_q].double() - per_ref[:rows_q]).abs()
        w_max = max(w_max, float((err / row_scale[:rows_q]).max()))
        w_el = max(w_el, float((err / (rel * per_ref[:rows_q].abs() + rel * row_rms[:rows_q])).max()))
    assert w_max <= rel, (what, "max-normalised", w_max)
    assert w_el <= 1.0, (what, "per-element bound", w_el)
    for copy in (0, t - 1):   # the rule itself, on the two ends of the array
        lo = (copy // oc.K) * per + sum(fam.e0[:copy % oc.K])
        assert_forward_close(e_out[lo:lo + fam.e0[copy % oc.K]].cpu().numpy(), refs[copy % oc.K], what=f"{what} copy {copy}")
    return w_max, w_el


# ------------------------------------------------------------------------------------------ F1 .. F6: the inference forward
@pytest.mark.parametrize("name,family,kernel,ms", [("F1", "dense", "hm", 1), ("F1s2", "dense", "hm", 2), ("F2", "dense", "hm", 1), ("F2c", "dense", "hm", 1),
                                                   ("F3", "dense", "auto", 1), ("F3s2", "dense", "auto", 2), ("F4", "dense", "auto", 1),
                                                   ("F5", "sparse", "auto", 1), ("F5b", "sparse", "auto", 1), ("F6", "sparse", "auto", 1)])
def test_forward_across_the_offset_boundaries(dev, name, family, kernel, ms):
    """EncProcDecGNN.forward without autograd on a tiling of `family`: every copy's prediction against its class's float64 one.  The
    route of the hidden-128 cases is the one the regime names (edge_sys_fits restated: inferred, see the module docstring).  ms: the
    message-passing steps -- the last step of a forward discards its e + e' rows, so only a model of two steps has the processor
    edge kernels STORE edge rows (hm_edge_kernel's line stores, sys_edge_kernel's WRITE_E epilogue)."""
    from gnn_manip_amd._lib import lib
    case = _case(name)
    fam, t, hidden = case.family, case.copies, case.hidden
    assert fam is _family(family)
    n, e = case.regime["n"], case.regime["e"]
    if kernel == "auto":
        assert hidden == 128   # the systolic kernels exist at this width: edge_sys_fits alone decides the route
    refs = _forward_refs(family, hidden, ms)
    m = _model(hidden, dev, ms)
    m.set_edge_kernel(kernel)
    L, d = _lib_desc(m)
    _need(dev, name, forward_ws=L.gm_forward_workspace_bytes(C.byref(d), n, e), csr_ws=lib().gm_csr_workspace_bytes(n, e),
          inputs=n * 25 * 4 + e * 4 * 4 + 2 * e * 8, tiling_scratch=6 * e * 8 + n * 25 * 4, out=n * 3 * 4 * 8)
    nodes, ea, ei = oc.tile_device(fam, t, dev)
    assert nodes.shape[0] == n and ei.shape[1] == e
    with torch.no_grad():
        out = m.forward(nodes, ea, ei)
    assert m.status() == e
    worst = _assert_copies_close(oc.copies_view(out, fam, t), refs, name)
    print(f"[offsets] {name}: worst copy error {worst[0]:.3e} of the class maximum (bar 1e-5), per-element ratio {worst[1]:.3f} (bar 1)")


# ------------------------------------------------------------------------------------------ B1: the stand-alone block, eid gather
@functools.lru_cache(maxsize=None)
def _block_refs(hidden):
    """Per class: float32 latents (the encoder's outputs, as a caller would hand them on) and the float64 block outputs on them."""
    fam = oc.dense_family()
    p32 = _params(hidden)
    p = {k: torch.tensor(v, dtype=torch.float64) for k, v in p32.items()}
    res = []
    for c in range(oc.K):
        h0, e0 = orc.graph_independent(p32, "encoder", fam.nodes[c], fam.edge_attr[c], NL)
        h, e = torch.tensor(h0, dtype=torch.float64), torch.tensor(e0, dtype=torch.float64)
        j, i = torch.tensor(fam.edge_index[c][0]), torch.tensor(fam.edge_index[c][1])
        with torch.no_grad():
            e_new = torch_epd.mlp(p, "processor.0.phi_edge", torch.cat((h[i], h[j], e), dim=1), NL, True)
            agg = torch.zeros_like(h).index_add_(0, i, e_new)
            h_new = torch_epd.mlp(p, "processor.0.phi_node", torch.cat((h, agg), dim=1), NL, True)
        res.append(dict(h=h0.astype(np.float32), e=e0.astype(np.float32), h_out=h_new.numpy(), e_out=e_new.numpy()))
    return res


def test_block_forward_gathers_and_returns_rows_in_the_callers_order(dev):
    """B1: InteractionNetwork.forward alone (gm_interaction_network_forward: hm_edge_kernel reads its e rows through eid and writes
    e_out through eid_out) at hidden 256 on 2.1 GiB of edge rows handed over in a seeded random order: h_out per copy, and e_out
    row for row where the caller's order put it."""
    from gnn_manip_amd._lib import lib
    case = _case("B1")
    fam, t, hidden = case.family, case.copies, case.hidden
    n, e = case.regime["n"], case.regime["e"]
    refs = _block_refs(hidden)
    m = _model(hidden, dev)
    L, d = _lib_desc(m)
    rows = e * hidden * 4
    _need(dev, "B1", block_ws=L.gm_block_workspace_bytes(C.byref(d), n, e), csr_ws=lib().gm_csr_workspace_bytes(n, e),
          edge_rows_x4=4 * rows, node_rows_x2=2 * n * hidden * 4, index=8 * e * 8, compare=rows // 8)
    _, _, ei = oc.tile_device(fam, t, dev)
    h = oc.tile_rows([torch.from_numpy(r["h"]).to(dev) for r in refs], t, torch)
    e_in = oc.tile_rows([torch.from_numpy(r["e"]).to(dev) for r in refs], t, torch)
    perm = torch.randperm(e, device=dev, generator=torch.Generator(device=dev).manual_seed(4242))
    assert not bool((perm[:-1] < perm[1:]).all())
    e_in_p, ei_p = e_in[perm], ei[:, perm].contiguous()
    del e_in, ei
    with torch.no_grad():
        h_out, e_out_p, _ = m.processor[0](h, e_in_p, ei_p)
    torch.cuda.synchronize()
    del e_in_p
    wh = _assert_copies_close(oc.copies_view(h_out, fam, t), [r["h_out"] for r in refs], "B1 h_out")
    # e_out: row k of the result belongs to edge perm[k] of the copy-by-copy layout
    e_out = torch.empty_like(e_out_p)
    e_out[perm] = e_out_p
    del e_out_p
    we_max, we_el = _assert_edge_rows_close(e_out, [r["e_out"] for r in refs], fam, t, "B1 e_out")
    print(f"[offsets] B1: worst copy error h_out {wh[0]:.3e} / e_out {we_max:.3e} of the class maximum (bar 1e-5), per-element ratio "
          f"{wh[1]:.3f} / {we_el:.3f} (bar 1)")


# ------------------------------------------------------------------------------------------ T0 .. T2: the training step
def _input_grad_check(what, view, g64, g32, scale_to_tiled, allowance):
    """yardstick.within's rule on the worst copy of a class: view [copies, rows, w] on the device."""
    ref = torch.from_numpy(np.ascontiguousarray(g64 * scale_to_tiled, np.float64)).to(view.device)
    assert bool(torch.isfinite(view).all()), what
    err = (view.double() - ref[None]).abs().amax(dim=0).cpu().numpy()
    scale = max(float(np.abs(g64).max()) * scale_to_tiled, 1e-30)
    tol = max(GRAD_TOL, 4.0 * float(np.abs(g32 - g64).max()) * scale_to_tiled / scale)
    ratio = float(err.max()) / scale / tol
    if ratio > 1.0:
        a = allowance() * scale_to_tiled
        over = err > tol * scale
        worst = float((err / (tol * scale + a)).max())
        print(f"[offsets] {what}: err {float(err.max()) / scale:.3e} of the maximum, tol {tol:.3e}: {int(over.sum())} elements in "
              f"{int(over.any(axis=1).sum())} of {err.shape[0]} rows beyond the plain bound; with the ReLU flip allowance (non-zero in "
              f"{int((a > 0).any(axis=1).sum())} rows) worst err / (tol + allowance) {worst:.3e}")
        assert worst <= 1.0, (what, float(err.max()) / scale, tol, worst)
    return ratio


@functools.lru_cache(maxsize=None)
def _class_input_allowance(hidden, c, dev):
    """grad_cases.flip_allowance of class c's loss sum |out - target| / n0: per-element bounds for (d_nodes, d_edge_attr).
    Plain torch in float64 ON THE DEVICE (up to 256 backward passes through a 20 k-edge graph: seconds there, most of a minute on
    the host), once per class and module."""
    fam = oc.dense_family()
    p = {k: torch.tensor(v, dtype=torch.float64, device=dev) for k, v in _params(hidden).items()}
    x = torch.tensor(fam.nodes[c], dtype=torch.float64, device=dev, requires_grad=True)
    a = torch.tensor(fam.edge_attr[c], dtype=torch.float64, device=dev, requires_grad=True)
    idx = torch.tensor(fam.edge_index[c], device=dev)
    tgt = torch.tensor(oc.class_targets(fam)[c], dtype=torch.float64, device=dev)
    allow, _ = flip_allowance(lambda fwd: torch.nn.functional.l1_loss(fwd(p, x, a, idx, NL, MS), tgt, reduction="sum") / fam.n0, [x, a])
    return allow


def _training_step(dev, name, inputs_grad):
    case = _case(name)
    fam, t, hidden = case.family, case.copies, case.hidden
    n, e = case.regime["n"], case.regime["e"]
    params, targets = _params(hidden), oc.class_targets(fam)
    r64, r32 = _grad_refs("dense", hidden, "float64"), _grad_refs("dense", hidden, "float32")
    m = _model(hidden, dev)
    L, d = _lib_desc(m)
    tape, ws = L.gm_train_tape_bytes(C.byref(d), n, e), L.gm_train_backward_workspace_bytes(C.byref(d), n, e)
    print(f"[offsets] {name}: tape {tape / GIB:.1f} GiB, backward workspace {ws / GIB:.1f} GiB")
    _need(dev, name, tape=tape, backward_ws=ws, inputs_and_grads=2 * (n * 25 * 4 + e * 4 * 4) + 2 * e * 8, tiling_scratch=6 * e * 8,
          out_and_target=n * 3 * 4 * 8)
    nodes, ea, ei = oc.tile_device(fam, t, dev)
    target = oc.tile_rows([torch.from_numpy(x).to(dev) for x in targets], t, torch)
    if inputs_grad:
        nodes.requires_grad_(True)
        ea.requires_grad_(True)
    out = m.forward(nodes, ea, ei)
    loss = torch.nn.functional.l1_loss(out, target, reduction="sum") / out.shape[0]
    loss.backward()
    m.status()   # a flagged edge_index would raise here
    wf = _assert_copies_close(oc.copies_view(out.detach(), fam, t), [r["out"] for r in r64], f"{name} forward")
    ref_loss = oc.assemble_loss(r64, t)
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * abs(ref_loss), (name, float(loss.detach()), ref_loss)
    got = {k: p.grad.cpu().numpy() for k, p in m.named_parameters()}
    assert all(np.isfinite(g).all() for g in got.values())
    wg, _ = yardstick.compare(got, oc.assemble_param_grads(r64, t), oc.assemble_param_grads(r32, t), tag="[offsets]",
                              allowance=lambda: (oc.assembled_flip_allowance(fam, params, targets, NL, MS, t), None))
    print(f"[offsets] {name}: forward worst copy error {wf[0]:.3e} (bar 1e-5), per-element ratio {wf[1]:.3f}; worst parameter gradient "
          f"{wg[0]}: err {wg[2]:.3e} of its maximum, tol {wg[3]:.3e} (err / tol {wg[1]:.3f})")
    if inputs_grad:
        s = oc.input_grad_scale(t)
        dn = oc.copies_view(nodes.grad, fam, t)
        full, rem = divmod(t, oc.K)
        per = fam.edge_period
        worst_in = 0.0
        for c in range(oc.K):
            allow = functools.partial(_class_input_allowance, hidden, c, dev)
            worst_in = max(worst_in, _input_grad_check(f"{name} d_nodes class {c}", dn[c::oc.K], r64[c]["d_nodes"], r32[c]["d_nodes"], s,
                                                       lambda: allow()[0]))
            lo, cnt = sum(fam.e0[:c]), fam.e0[c]   # class c's edge rows of every period it occurs in
            copies = full + (1 if c < rem else 0)
            idx = (torch.arange(copies, device=dev) * per + lo)[:, None] + torch.arange(cnt, device=dev)[None]
            worst_in = max(worst_in, _input_grad_check(f"{name} d_edge_attr class {c}", ea.grad[idx], r64[c]["d_edge_attr"],
                                                       r32[c]["d_edge_attr"], s, lambda: allow()[1]))
        print(f"[offsets] {name}: worst input gradient err / tol {worst_in:.3f} (bar 1, before any flip allowance)")


def test_training_step_with_tapes_beyond_2_gib(dev):
    """T0: hidden 128, E = 4.3 M -- every edge-sized tape array is 2.05 GiB."""
    _training_step(dev, "T0", inputs_grad=False)


def test_training_step_just_under_4_gib_of_edge_rows_with_input_gradients(dev):
    """T1: hidden 256, E = 4.16 M (3.97 GiB of edge rows), nodes and edge_attr requiring grad: the chains' rows, the segment sums, the
    weight-gradient chunks and the dxidx stores of d_edge_attr (train_bwd_kernel) at offsets up to 4 GiB."""
    _training_step(dev, "T1", inputs_grad=True)


def test_training_step_beyond_4_gib_of_edge_rows_with_input_gradients(dev):
    """T2: the same at E = 4 200 616 >= 4 194 304 (4.006 GiB of edge rows).  The fused training step is documented for
    e < 2^31 / hidden (8.4 M at hidden 256) and hands wgrad_body no hidden-wide INDEXED operand (its only indexed one is edge_attr, 16
    bytes a row), so the 4 GiB guard does not apply to it: the step must be right, to T1's yardstick.  The guard itself: T2g below."""
    _training_step(dev, "T2", inputs_grad=True)


def test_block_backward_refuses_an_indexed_operand_beyond_4_gib(dev):
    """T2g: the guard where it applies.  InteractionNetwork under autograd reads its weight-gradient operand e_in through eid with
    32-bit byte offsets (csrc/train.hip wgrad_body); at E * hidden * 4 >= 4 GiB gm_interaction_network_backward returns
    GM_ERR_UNSUPPORTED naming the limit.  No parameter's .grad is touched, and the same block then passes a small step."""
    from gnn_manip_amd._lib import GMError, ModelDesc, lib
    case = _case("T2g")
    fam, t, hidden = case.family, case.copies, case.hidden
    n, e = case.regime["n"], case.regime["e"]
    assert e * hidden * 4 >= oc.GIB4 and e < (1 << 31) // hidden   # beyond the guard, inside the entry point's range
    m = _model(hidden, dev)
    blk = m.processor[0]
    desc, _ = blk._standalone(dev)
    L, d = lib(), ModelDesc(*desc)
    rows = e * hidden * 4
    _need(dev, "T2g", block_tape=L.gm_block_tape_bytes(C.byref(d), 1, n, e), backward_ws=L.gm_block_backward_workspace_bytes(C.byref(d), n, e),
          edge_rows_x5=5 * rows, node_rows_x5=5 * n * hidden * 4, index=8 * e * 8)
    _, _, ei = oc.tile_device(fam, t, dev)
    g = torch.Generator(device=dev).manual_seed(77)
    h = torch.randn((n, hidden), device=dev, generator=g).requires_grad_(True)
    e_in = torch.randn((e, hidden), device=dev, generator=g).requires_grad_(True)
    h_out, e_out, _ = blk(h, e_in, ei)
    with pytest.raises(GMError, match="4 GiB") as info:
        (h_out.sum() + e_out.sum()).backward()
    assert info.value.code == -2   # GM_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters()) and h.grad is None and e_in.grad is None
    del h, e_in, h_out, e_out, ei
    gc.collect()
    torch.cuda.empty_cache()
    # the same block then runs a small step (one class graph) exactly as a block that never met the error does: bit for bit, the
    # kernels are deterministic -- and that step's own correctness is tests/test_gpu_train_regimes.py's subject
    r = _block_refs(hidden)[0]
    idx = torch.from_numpy(fam.edge_index[0]).to(dev)
    rng = np.random.default_rng(78)
    wh = torch.from_numpy(rng.standard_normal(r["h"].shape).astype(np.float32)).to(dev)
    we = torch.from_numpy(rng.standard_normal(r["e"].shape).astype(np.float32)).to(dev)

    def small_step(model):
        hs = torch.from_numpy(r["h"]).to(dev).requires_grad_(True)
        es = torch.from_numpy(r["e"]).to(dev).requires_grad_(True)
        ho, eo, _ = model.processor[0](hs, es, idx)
        ((ho * wh).sum() + (eo * we).sum()).backward()
        return [ho.detach(), eo.detach(), hs.grad, es.grad] + [q.grad for q in model.processor[0].parameters()]

    after, fresh = small_step(m), small_step(_model(hidden, dev))
    assert len(after) == len(fresh) > 4
    for x, y in zip(after, fresh):
        assert x is not None and bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0.0 and torch.equal(x, y)
    assert_forward_close(after[0].cpu().numpy(), r["h_out"], what="T2g small step h_out")
    assert all(q.grad is None for k, q in m.named_parameters() if not k.startswith("processor.0."))


@functools.lru_cache(maxsize=None)
def _block_weights(hidden, c):
    """Seeded weights of class c's loss sum(h_out * wh) + sum(e_out * we)."""
    rng = np.random.default_rng(8800 + c)
    fam = oc.dense_family()
    return rng.standard_normal((fam.n0, hidden)).astype(np.float32), rng.standard_normal((fam.e0[c], hidden)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _block_grad_refs(hidden, dtype_name):
    """Per class: the block's parameter gradients of that loss on the class's latents, plain torch on the host."""
    dtype = getattr(torch, dtype_name)
    fam, res = oc.dense_family(), []
    for c, r in enumerate(_block_refs(hidden)):
        p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in _params(hidden).items() if k.startswith("processor.0.")}
        h, e = torch.tensor(r["h"], dtype=dtype), torch.tensor(r["e"], dtype=dtype)
        j, i = torch.tensor(fam.edge_index[c][0]), torch.tensor(fam.edge_index[c][1])
        e_new = torch_epd.mlp(p, "processor.0.phi_edge", torch.cat((h[i], h[j], e), dim=1), NL, True)
        h_new = torch_epd.mlp(p, "processor.0.phi_node", torch.cat((h, torch.zeros_like(h).index_add_(0, i, e_new)), dim=1), NL, True)
        wh, we = _block_weights(hidden, c)
        ((h_new * torch.tensor(wh, dtype=dtype)).sum() + (e_new * torch.tensor(we, dtype=dtype)).sum()).backward()
        res.append({k[len("processor.0."):]: v.grad.numpy() for k, v in p.items()})
    return res


@functools.lru_cache(maxsize=None)
def _block_flip_allowance(hidden, c, dev):
    """oracle/torch_epd.relu_flip_allowance restated for the stand-alone block's loss on class c (the same tau = 1e-5 of a Linear's
    rms, the same 256 units closest to zero, first order, absolute values summed over the units): {parameter: max |allowed change|}.
    Plain torch in float64 on the device, as _class_input_allowance."""
    fam, r = oc.dense_family(), _block_refs(hidden)[c]
    t64 = lambda a, grad=False: torch.tensor(a, dtype=torch.float64, device=dev, requires_grad=grad)
    p = {k: t64(v, True) for k, v in _params(hidden).items() if k.startswith("processor.0.")}
    h, e = t64(r["h"]), t64(r["e"])
    j, i = torch.tensor(fam.edge_index[c][0], device=dev), torch.tensor(fam.edge_index[c][1], device=dev)
    tape = []
    e_new = torch_epd._mlp_taped(p, "processor.0.phi_edge", torch.cat((h[i], h[j], e), dim=1), NL, True, tape)
    h_new = torch_epd._mlp_taped(p, "processor.0.phi_node", torch.cat((h, torch.zeros_like(h).index_add_(0, i, e_new)), dim=1), NL, True, tape)
    wh, we = _block_weights(hidden, c)
    ((h_new * t64(wh)).sum() + (e_new * t64(we)).sum()).backward(retain_graph=True)
    bounds = torch_epd.flip_bounds(tape, torch_epd.near_zero_units(tape), list(p.values()))
    return {k[len("processor.0."):]: float(v.max()) for k, v in zip(p, bounds)}


def test_block_backward_just_under_the_guard(dev):
    """T1g: InteractionNetwork under autograd at hidden 256 on 3.97 GiB of edge rows, the largest size the guard of T2g admits: the
    weight-gradient kernel gathers e_in rows through eid at 32-bit byte offsets up to 4 GiB (wgrad_body), and train_bwd_kernel
    stores de_in through dxidx.  Forward per copy at the forward bar; parameter gradients (sums over all copies) by the gradient
    rule against the assembled float64 / float32 references (fallback: _block_flip_allowance, assembled like them -- a unit near zero
    flips in every copy of its class at once); the input gradients dh_in / de_in of every copy BIT-equal to the same class graph run alone -- a row's
    gradient does not depend on where the row lies (the batch invariant), and a stand-alone block's input gradients at ordinary
    sizes are tests/test_gpu_train_regimes.py's subject."""
    from gnn_manip_amd._lib import ModelDesc, lib
    case = _case("T1g")
    fam, t, hidden = case.family, case.copies, case.hidden
    n, e = case.regime["n"], case.regime["e"]
    assert oc.GIB2 <= e * hidden * 4 < oc.GIB4
    refs = _block_refs(hidden)
    m = _model(hidden, dev)
    blk = m.processor[0]
    desc, _ = blk._standalone(dev)
    L, d = lib(), ModelDesc(*desc)
    rows = e * hidden * 4
    _need(dev, "T1g", block_tape=L.gm_block_tape_bytes(C.byref(d), 1, n, e), backward_ws=L.gm_block_backward_workspace_bytes(C.byref(d), n, e),
          edge_rows_x9=9 * rows, node_rows_x9=9 * n * hidden * 4, index=8 * e * 8)
    weights = [_block_weights(hidden, c) for c in range(oc.K)]

    def run(h_rows, e_rows, wh_rows, we_rows, ei):
        h, e_in = h_rows.clone().requires_grad_(True), e_rows.clone().requires_grad_(True)
        for q in blk.parameters():
            q.grad = None
        h_out, e_out, _ = blk(h, e_in, ei)
        ((h_out * wh_rows).sum() + (e_out * we_rows).sum()).backward()
        return h_out.detach(), e_out.detach(), h.grad, e_in.grad

    on_dev = lambda a: torch.from_numpy(a).to(dev)
    alone = [run(on_dev(refs[c]["h"]), on_dev(refs[c]["e"]), on_dev(weights[c][0]), on_dev(weights[c][1]), on_dev(fam.edge_index[c]))
             for c in range(oc.K)]
    _, _, ei = oc.tile_device(fam, t, dev)
    h_out, e_out, dh, de = run(oc.tile_rows([on_dev(r["h"]) for r in refs], t, torch), oc.tile_rows([on_dev(r["e"]) for r in refs], t, torch),
                               oc.tile_rows([on_dev(w[0]) for w in weights], t, torch), oc.tile_rows([on_dev(w[1]) for w in weights], t, torch), ei)
    torch.cuda.synchronize()
    wf = _assert_copies_close(oc.copies_view(h_out, fam, t), [r["h_out"] for r in refs], "T1g h_out")
    we = _assert_edge_rows_close(e_out, [r["e_out"] for r in refs], fam, t, "T1g e_out")
    del h_out, e_out
    # parameter gradients: the multiplicity-weighted sums of the class gradients (the loss is a plain sum: no 1 / N)
    mult = oc.multiplicity(t)
    r64, r32 = _block_grad_refs(hidden, "float64"), _block_grad_refs(hidden, "float32")
    g64 = {k: sum(mu * r64[c][k].astype(np.float64) for c, mu in enumerate(mult)) for k in r64[0]}
    g32 = {k: sum(mu * r32[c][k].astype(np.float64) for c, mu in enumerate(mult)) for k in r32[0]}
    got = {k: q.grad.cpu().numpy() for k, q in blk.named_parameters()}
    def allowance():
        per_class = [_block_flip_allowance(hidden, c, dev) for c in range(oc.K)]
        return {k: sum(mu * per_class[c][k] for c, mu in enumerate(mult)) for k in per_class[0]}, None
    wg, _ = yardstick.compare(got, g64, g32, allowance=allowance, tag="[offsets]")
    # input gradients: every copy is its class graph alone, bit for bit
    dhv = oc.copies_view(dh, fam, t)
    full, rem = divmod(t, oc.K)
    per = fam.edge_period
    for c in range(oc.K):
        assert bool(torch.isfinite(alone[c][2]).all()) and bool(torch.isfinite(alone[c][3]).all())
        bad = (dhv[c::oc.K] != alone[c][2][None]).flatten(1).any(dim=1)
        assert not bool(bad.any()), ("T1g dh_in: copies of class", c, "differ from the class alone", torch.nonzero(bad).flatten()[:8].tolist())
        lo, cnt = sum(fam.e0[:c]), fam.e0[c]
        copies = full + (1 if c < rem else 0)
        idx = (torch.arange(copies, device=dev) * per + lo)[:, None] + torch.arange(cnt, device=dev)[None]
        bad = (de[idx] != alone[c][3][None]).flatten(1).any(dim=1)
        assert not bool(bad.any()), ("T1g de_in: copies of class", c, "differ from the class alone", torch.nonzero(bad).flatten()[:8].tolist())
    print(f"[offsets] T1g: forward worst copy error h_out {wf[0]:.3e} / e_out {we[0]:.3e} (bar 1e-5); worst parameter gradient {wg[0]}: err "
          f"{wg[2]:.3e} of its maximum, tol {wg[3]:.3e} (err / tol {wg[1]:.3f}); dh_in / de_in of all {t} copies bit-equal to their class alone")


# ------------------------------------------------------------------------------------------ R1: a rollout step of 211 candidates
def test_rollout_step_of_a_candidate_batch_beyond_2_gib_of_edge_rows(dev):
    """R1: RolloutEngine(candidates=211) on a 1021-particle scene, one step -- 215 431 nodes, 4.3 M edges, 2.05 GiB of edge rows through
    the step's fused graph build, destination sort, feature and forward chain.  Every candidate is bit-equal to the same trajectory
    rolled out alone (the batch invariant of test_batch_invariance_does_not_depend_on_the_batch_size); the first, the last and the
    three candidates around the one whose edge rows straddle 2^31 bytes are held to oracle.rollout at the bar of
    test_rollout_small_and_ragged_scenes (5e-6 absolute)."""
    from gnn_manip_amd import GraphBoundedMultimaterialControl, RolloutEngine, scene
    from gnn_manip_amd._lib import lib
    case = _case("R1")
    b, hidden, n0 = case.copies, case.hidden, oc.N0
    obs = scene.make_scene(n0, seed=900, side=oc.DENSE_SIDE)
    s_ref, _ = orc.get_connectivity(obs[-1][:, 2:5], 0.015, 20)
    e_scene = int(len(s_ref))
    row_bytes = hidden * 4
    assert oc.GIB2 <= b * e_scene * row_bytes < oc.GIB4 and b * n0 == case.regime["n"]
    straddler = oc.GIB2 // (e_scene * row_bytes)
    assert 0 < straddler < b - 1 and straddler * e_scene * row_bytes <= oc.GIB2 < (straddler + 1) * e_scene * row_bytes
    trajs = np.stack([scene.rigid_drift_trajectory(obs, 1, seed=5000 + c, step_size=2e-4) for c in range(b)])
    m = _model(hidden, dev)
    ga = GraphBoundedMultimaterialControl(0.015, STATS, CART, MAT, CTRL, BOUNDS)
    L, d = _lib_desc(m)
    _need(dev, "R1", rollout_ws=L.gm_rollout_workspace_bytes(C.byref(d), b * n0, 20), states=4 * obs.shape[0] * b * n0 * 8 * 4)
    obs_d, trajs_d = torch.from_numpy(obs).to(dev), torch.from_numpy(trajs).to(dev)
    with torch.no_grad():
        eng = RolloutEngine(m, ga, n0, device=dev, candidates=b)
        out = eng.rollout_candidates(obs_d, trajs_d)
        assert eng.status() == b * e_scene
        assert bool(torch.isfinite(out).all())
        one = RolloutEngine(m, ga, n0, device=dev)
        differing = []
        for c in range(b):
            alone = one.rollout(obs_d, trajs_d[c], horizon=1)
            if not torch.equal(out[c], alone):
                differing.append((c, float((out[c] - alone).abs().max())))
        assert one.status() == e_scene
    assert not differing, differing[:8]
    worst = 0.0
    for c in sorted({0, straddler - 1, straddler, straddler + 1, b - 1}):
        ref = orc.rollout(_params(hidden), obs, trajs[c], 1, STATS, BOUNDS, 0.015, CART, MAT, CTRL, NL, MS)
        got = out[c].cpu().numpy()
        np.testing.assert_allclose(got[:, :, 2:8], ref[:, :, 2:8], rtol=0, atol=5e-6)
        np.testing.assert_array_equal(got[:, :, :2], ref[:, :, :2])
        worst = max(worst, float(np.abs(got[:, :, 2:8] - ref[:, :, 2:8]).max()))
    print(f"[offsets] R1: {b} candidates bit-equal to their single rollouts; worst |state - oracle| over 5 candidates {worst:.3e} (bar 5e-6)")
