"""Device plumbing of the GPU tests, once -- a plain helper module (no test, no conftest).  The library is imported inside the
functions: importing this module does not load it.  The `dev` fixture is imported by name into a test module, which makes it that
module's own module-scoped fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc
from oracle import torch_epd
import grad_cases as gc
import rollout_grad_cases as rc
import yardstick

TILE = 128            # rows of one training tile (csrc/train.h)
K_NB = 20             # the neighbour cap of the rollout's radius graph
L0 = gc.L0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def to_dev(a, dev):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a if a.flags.writeable else a.copy()).to(dev)     # a copy: the cases' arrays are read-only


def load_model(params, dims, dev, kernel=None, precision=None, **conv):
    """EncProcDecGNN(*dims, **conv) with the oracle's parameters on the device; kernel / precision: set_edge_kernel / set_precision."""
    from gnn_manip_amd import EncProcDecGNN
    m = EncProcDecGNN(*dims, **conv)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, strict=True)
    m = m.to(dev)
    if kernel is not None:
        m.set_edge_kernel(kernel)
    if precision not in (None, "f32"):
        m.set_precision(precision)
    return m


def graph_attr(r, layout=None):
    """The feature functions of a width_cases layout, or of the default scene's columns."""
    from gnn_manip_amd import GraphBoundedMultimaterial, GraphBoundedMultimaterialControl
    if layout is None:
        return GraphBoundedMultimaterialControl(r, STATS, CART, MAT, CTRL, BOUNDS)
    if layout.ctrl < 0:
        return GraphBoundedMultimaterial(r, STATS, layout.cart_idx, [layout.mat], BOUNDS)
    return GraphBoundedMultimaterialControl(r, STATS, layout.cart_idx, [layout.mat], layout.ctrl_idx, BOUNDS)


def feature_desc(r, layout, n_per=0):
    from gnn_manip_amd.graph import make_feature_desc
    d = make_feature_desc(r, STATS, BOUNDS, layout.cart_idx, [layout.mat], layout.ctrl_idx, layout.k, layout.D)
    d.nodes_per_graph = n_per
    return d


def rollout_engine(m, r, layout, n, dev, **kw):
    from gnn_manip_amd import RolloutEngine
    return RolloutEngine(m, graph_attr(r, layout), n, k_steps=layout.k, data_dim=layout.D, device=dev, **kw)


def step_engine(m, dev, candidates=1):
    """The engine of grad_cases' step scene."""
    return rollout_engine(m, gc.R, L0, gc.STEP_N, dev, candidates=candidates)


def poison_allocator(dev, pattern):
    """Fill the caching allocator's free blocks: what torch.empty hands out next (the library's workspaces) holds `pattern`."""
    junk = [torch.full((n,), pattern, device=dev) for n in (1 << 24, 1 << 22, 1 << 20, 3 << 18, 5 << 16, 7 << 12, 65536 * 3, 257)]
    junk += [torch.full((n,), 0x7fc00000, dtype=torch.int32, device=dev) for n in (1 << 22, 1 << 20, 1 << 18, 4096)]
    del junk


def cus(dev):
    return int(torch.cuda.get_device_properties(dev).multi_processor_count)


def tiles(rows):
    return -(-rows // TILE)


def torch_random_graph(n, e, seed, dev, hub=0, node_dim=25, edge_dim=4):
    """n nodes, e random edges (torch's generator); hub > 0: the first `hub` edges all arrive at node n // 2."""
    g = torch.Generator().manual_seed(seed)
    nodes = torch.randn(n, node_dim, generator=g)
    ea = torch.randn(e, edge_dim, generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[1, :hub] = n // 2
    return nodes.to(dev), ea.to(dev), ei.to(dev)


# ------------------------------------------------------------------------------------------ the training step
def l1_step(m, nodes, ea, ei, target, dev):
    """One forward and backward of the L1 training loss (train_dyn.py:65: sum / N): (prediction, loss), attached."""
    out = m.forward(to_dev(nodes, dev), to_dev(ea, dev), to_dev(ei, dev))
    loss = torch.nn.functional.l1_loss(out, to_dev(target, dev), reduction="sum") / out.shape[0]
    loss.backward()
    return out, loss


def compare_parameter_gradients(m, params, nodes, ea, ei, target, num_layers, m_steps, ref_g, g32, ln_eps=1e-5):
    """Every parameter gradient of m against float64 by the rule of tests/yardstick.py, the allowance per tensor
    (torch_epd.relu_flip_allowance of THIS input, at the model's ln_eps): no seed is exempt.  Returns yardstick.compare's two worst tensors."""
    got = {}
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        got[name] = p.grad.cpu().numpy()
    return yardstick.compare(got, ref_g, g32, lambda: torch_epd.relu_flip_allowance(params, nodes, ea, ei, target, num_layers, m_steps, ln_eps=ln_eps))


def check_training_step(m, params, nodes, ea, ei, dims, dev, seed, ref=None):
    """One L1 step on a seeded target: forward and loss to 1e-5, every parameter gradient by compare_parameter_gradients.
    ref: a dict that receives the target and the float64 / float32 reference gradients (target, ref_g, g32), for a caller that
    looks at single tensors afterwards."""
    rng = np.random.default_rng(seed)
    target = rng.standard_normal((nodes.shape[0], dims[2])).astype(np.float32)
    out, loss = l1_step(m, nodes, ea, ei, target, dev)
    ref_out, ref_loss, ref_g = torch_epd.loss_and_grads(params, nodes, ea, ei, target, dims[4], dims[5])
    _, _, g32 = torch_epd.loss_and_grads(params, nodes, ea, ei, target, dims[4], dims[5], torch.float32)
    err = np.abs(out.detach().cpu().numpy() - ref_out).max()
    assert err <= 1e-5 * max(np.abs(ref_out).max(), 1e-3), ("forward", err, np.abs(ref_out).max())
    assert abs(float(loss.detach()) - ref_loss) <= 1e-5 * abs(ref_loss), ("loss", float(loss.detach()), ref_loss)
    if ref is not None:
        ref.update(target=target, ref_g=ref_g, g32=g32)
    return compare_parameter_gradients(m, params, nodes, ea, ei, target, dims[4], dims[5], ref_g, g32)


def rank_sum(rows_np, count, dev, fill=float("nan"), guard=8):
    """gm_rank_sum through ctypes over `rows_np` [world, stride] into a destination of count + guard floats filled with `fill`."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    world, stride = rows_np.shape
    src = to_dev(rows_np, dev)
    dst = torch.full((count + guard,), fill, dtype=torch.float32, device=dev)
    check(lib().gm_rank_sum(ptr(src), count, world, stride, ptr(dst), current_stream(dev)))
    out = dst.cpu().numpy()
    assert np.array_equal(out[count:].view(np.uint32), np.full(guard, fill, np.float32).view(np.uint32)), "written past count"
    return out[:count]


# ------------------------------------------------------------------------------------------ the rollout's reverse sweep through ctypes
def edges_of(window, eng):
    """The radius graph of a pre-step window: get_connectivity on its last frame's positions (state_pre moves no position)."""
    from gnn_manip_amd import get_connectivity
    c0 = L0.cart
    s, r = get_connectivity(window[-1][:, c0:c0 + 3], gc.R, K_NB, eng.n_per if eng.candidates > 1 else None)
    return torch.stack((s, r)).cpu().numpy()


def step_call(eng, obs, tgt, g, dev, ws=None):
    """gm_rollout_step_backward through ctypes, in a workspace of the queried size (or the caller's): (d_obs, d_target, edges)."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    from gnn_manip_amd.graph import _ws
    L = lib()
    h, tensors, t_arr, md = eng._training_model()
    need = L.gm_rollout_step_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    assert need > 0, need
    if ws is None:
        ws = _ws(need, dev)
    assert ws.numel() >= need, (ws.numel(), need)
    d_obs = torch.full_like(obs, float("nan"))
    d_tgt = None if tgt is None else torch.full_like(tgt, float("nan"))
    e = C.c_int64(-1)
    check(L.gm_rollout_step_backward(h, t_arr, len(tensors), ptr(obs), eng.n, C.byref(eng.fdesc), K_NB, ptr(eng.rigid_rank), ptr(tgt),
                                     ptr(g), ptr(d_obs), ptr(d_tgt), C.byref(e), ptr(ws), need, current_stream(dev)))
    return d_obs, d_tgt, int(e.value)


def forward_windows(eng, obs_np, traj_np, steps, dev):
    """The inference rollout keeping every pre-step window: (windows [steps, k, N, D], final state)."""
    obs = to_dev(obs_np, dev).clone()
    eng.set_scene(obs)
    tr = None if traj_np is None else to_dev(traj_np, dev)
    windows = torch.empty((steps,) + tuple(obs.shape), device=dev)
    for t in range(steps):
        windows[t].copy_(obs)
        eng.step(obs, None if tr is None or t >= tr.shape[0] else tr[t])
    eng.status()
    return windows, obs


def sweep_call(eng, windows, traj, steps, d_final, dev, ws=None, want_traj=True):
    """gm_rollout_backward through ctypes: (d_obs0, d_trajectory)."""
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    from gnn_manip_amd.graph import _ws
    L = lib()
    h, tensors, t_arr, md = eng._training_model()
    need = L.gm_rollout_backward_workspace_bytes(C.byref(md), C.byref(eng.fdesc), eng.n, K_NB)
    if ws is None:
        ws = _ws(need, dev)
    assert ws.numel() >= need, (ws.numel(), need)
    d_obs0 = torch.full_like(d_final, float("nan"))
    d_traj = torch.full_like(traj, float("nan")) if traj is not None and want_traj else None
    check(L.gm_rollout_backward(h, t_arr, len(tensors), ptr(windows), eng.n, C.byref(eng.fdesc), K_NB, ptr(eng.rigid_rank), ptr(traj),
                                0 if traj is None else traj.shape[0], eng.n_rigid, steps, ptr(d_final), ptr(d_obs0), ptr(d_traj), ptr(ws),
                                need, current_stream(dev)))
    return d_obs0, d_traj


# ------------------------------------------------------------------------------------------ the planner's solvers
def planner_solver(dev, n=400, horizon=5, cands=4):
    """A TrajectoryCMAsolver on make_scene(n, seed 31) with a damped random model: (solver, parameters, scene)."""
    from gnn_manip_amd import scene
    from gnn_manip_amd.planner import TrajectoryCMAsolver
    obs = scene.make_scene(n, seed=31, side=0.06)
    params = orc.init_params(25, 4, 3, 128, 2, 2, 31)
    params["decoder.4.weight"] = params["decoder.4.weight"] * 1e-3  # keep the random-weight scene from exploding
    m = load_model(params, (25, 4, 3, 128, 2, 2), dev)
    state = (to_dev(obs, dev), to_dev(obs[-1, :, 2:5], dev))
    s = TrajectoryCMAsolver(m, graph_attr(0.015), state, 180, [0.5, 0.5, 0.4], scale_rot=1.0, scale_ty=1.0, alpha=0.1, beta=1000.0,
                            gamma=0.05, penalty=1.0, rho=0.0, device=dev, cma_iter=3, cma_popsize=6, total_steps=horizon,
                            candidates_per_gpu=cands)
    sample = np.stack((180.0 - 0.4 * np.arange(horizon + 1), 1e-4 * np.arange(horizon + 1)), axis=1)
    s.set_sample_traj(sample)
    coffee = obs[-1, obs[-1, :, 1] == 0][:, 2:5]
    s.desired_pos = to_dev(coffee + np.float32(0.002), dev)
    return s, params, obs


def step_solver(dev, cls=None):
    """A TrajectoryCMAsolver on the step scene, total_steps = 4, traj_points = 2.  The cup frame is centred on the rigid rows and
    the solver's rigid particles are their mirror images in x, so that the pose at the initial rotation (180 degrees) and no
    translation is where the rigid rows are: the scripted poses then move them by a fraction of a millimetre per step."""
    from gnn_manip_amd.planner import TrajectoryCMAsolver
    obs_np = gc.step_state("step_a")
    m = load_model(rc.params(), gc.STEP_DIMS, dev)
    rigid = obs_np[-1][gc.rigid_rows(obs_np, L0)][:, L0.cart:L0.cart + 3]
    cx, cy, cz = (float(np.float32(round(float(v), 3))) for v in rigid.mean(axis=0))
    ty_init = [cx, cz, cy]
    state = (to_dev(obs_np, dev), to_dev(obs_np[-1][:, L0.cart:L0.cart + 3], dev))
    s = (cls or TrajectoryCMAsolver)(m, graph_attr(gc.R, L0), state, 180, ty_init, scale_rot=1.0, scale_ty=1.0, alpha=0.1, beta=1000.0,
                                     gamma=0.05, penalty=1.0, rho=0.0, device=dev, total_steps=4, traj_points=2, candidates_per_gpu=1)
    mirrored = rigid.copy()
    mirrored[:, 0] = np.float32(2.0) * np.float32(cx) - rigid[:, 0]
    s.rigid_particles = to_dev(mirrored, dev)
    s.set_sample_traj(np.stack((180.0 - 0.4 * np.arange(5), 1e-4 * np.arange(5)), axis=1))
    fluid, cloud = rc.desired_cloud(obs_np)
    assert np.array_equal(fluid, np.nonzero(s.coffee_particles_idx.cpu().numpy())[0]), "the solver's fluid rows are not the case's"
    s.desired_pos = to_dev(cloud, dev)
    return s, obs_np, mirrored, fluid, cloud
