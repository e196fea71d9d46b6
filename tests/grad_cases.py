"""Cases and the float64 reference of the differentiable rollout step (tests/test_grad_cases.py checks them on the CPU,
tests/test_gpu_input_grads.py holds the HIP backward to them).

The reference is a plain-PyTorch float64 restatement of the per-step functions -- node features, edge features, integrator, the
two state updates -- differentiable by autograd; the model is oracle/torch_epd.epd_forward.  Its forward is held to the numpy
oracle (oracle/epd_oracle.py) and its gradients to central finite differences by the CPU test, so the GPU test compares against
something that was itself checked.

The cases are states in the layouts of tests/width_cases.py whose particle cloud overlaps the lower wall's band (so that boundary
features are clamped for some particles and not for others, on either side of zero) with one particle alone next to the upper
wall (a node whose only edge is its self edge; an unclamped upper feature).  `regime` measures what a case is there for."""
import functools

import numpy as np
import torch

from conftest import BOUNDS, STATS
from oracle import epd_oracle as orc
from oracle import torch_epd
import train_cases
import width_cases as wc
from yardstick import lazy, within

F32 = np.float32
R = wc.R
ALONE = 7                      # the row placed alone next to the upper wall
ALONE_AT = (0.893, 0.5, 0.52)
F64 = torch.float64


def _stat(name, like):
    return torch.tensor(STATS[name], dtype=like.dtype)


# ------------------------------------------------------------------------------------------ the restatement (torch; float64, or the
# dtype of its inputs: the GPU tests' yardstick also runs it in float32)
def node_features(obs, L):
    """collate_utils.py:195-232: [N, 3 (k - 1) + 6 + 1 (+ 3)]."""
    pos = obs[:, :, L.cart:L.cart + 3]
    vm, vs = _stat("velocity_mean", obs), _stat("velocity_std", obs)
    vel = ((pos[1:] - pos[:-1] - vm) / vs).permute(1, 0, 2).reshape(obs.shape[1], -1)
    lower = (pos[-1] - torch.tensor(BOUNDS["lower_bounds"], dtype=obs.dtype)) / R
    upper = (torch.tensor(BOUNDS["upper_bounds"], dtype=obs.dtype) - pos[-1]) / R
    # the material column is a label (0 / 1 / other), not a coordinate: it is read, and gets no gradient
    cols = [vel, torch.clamp(lower, -1.0, 1.0), torch.clamp(upper, -1.0, 1.0), obs[-1][:, L.mat:L.mat + 1].detach()]
    if L.ctrl >= 0:
        cols.append((obs[-1][:, L.ctrl:L.ctrl + 3] - vm) / vs)
    return torch.cat(cols, dim=1)


def unclamped_boundary(obs, L):
    """[N, 6] numpy float64: the boundary features before the clamp."""
    pos = np.asarray(obs, np.float64)[-1][:, L.cart:L.cart + 3]
    return np.concatenate(((pos - np.asarray(BOUNDS["lower_bounds"])) / R, (np.asarray(BOUNDS["upper_bounds"]) - pos) / R), axis=1)


def edge_features(pos, senders, receivers):
    """utils.py:43-61: [(p_s - p_r) / r, ||.||]; torch.linalg.norm's gradient at 0 is 0."""
    d = (pos[senders] - pos[receivers]) / R
    return torch.cat((d, torch.linalg.norm(d, dim=1, keepdim=True)), dim=1)


def integrate(pred, obs, L):
    """rollout_utils.py:145-158."""
    pos = obs[:, :, L.cart:L.cart + 3]
    acc = pred * _stat("acceleration_std", pred) + _stat("acceleration_mean", pred)
    return pos[-1] + ((pos[-1] - pos[-2]) + acc)


def state_pre(obs, L, rows, target):
    """rollout_utils.py:40-47; rows: indices of the rigid rows (ascending), target: [len(rows), 3] or None."""
    if L.ctrl < 0:
        return obs
    last = obs[-1]
    cur = last[rows][:, L.cart:L.cart + 3]
    new = last.clone()
    new[rows, L.ctrl:L.ctrl + 3] = cur if target is None else target - cur
    return torch.cat((obs[:-1], new[None]))


def state_post(obs, L, next_pos, rows, target):
    """rollout_utils.py:53-61: window shift; a rigid row keeps its pre-step row, with the scripted pose when there is one."""
    keep = obs[-1][rows].clone()
    if target is not None:
        keep[:, L.cart:L.cart + 3] = target
    last = obs[-1].clone()
    last[:, L.cart:L.cart + 3] = next_pos
    last[rows] = keep
    return torch.cat((obs[1:], last[None]))


def step(p64, obs, L, rows, target, edge_index, num_layers, m_steps, forward=torch_epd.epd_forward):
    """One rollout step on a given edge list (the radius graph is a constant of the step): (next_obs, pred).  forward: the model
    (a caller that records the hidden pre-activations passes its own)."""
    pre = state_pre(obs, L, rows, target)
    nodes = node_features(pre, L)
    ea = edge_features(pre[-1][:, L.cart:L.cart + 3], edge_index[0], edge_index[1])
    pred = forward(p64, nodes, ea, edge_index, num_layers, m_steps)
    return state_post(pre, L, integrate(pred, pre, L), rows, target), pred


# ------------------------------------------------------------------------------------------ states
STATE_SEEDS = {"default": 811, "k2": 812, "k3": 813, "k8": 814, "moved": 815, "no_control": 816, "step_a": 821, "step_b": 822}
STEP_N, STEP_SIDE = 400, 0.07
STEP_DIMS = (25, 4, 3, 128, 2, 2)


@functools.lru_cache(maxsize=None)
def state(name, layout=None, n=wc.SCENE_N, side=0.06):
    """[k, n, D] float32 in LAYOUTS[layout or name].  The cloud starts 0.012 below the lower wall's plane (0.1): rows inside
    [0.085, 0.115] have unclamped lower features of either sign, the rest are clamped; row ALONE sits 0.007 from the upper wall,
    away from every other particle.  The last tenth of the rows is rigid; control and payload columns carry seeded values."""
    L = wc.LAYOUTS[layout or name]
    rng = np.random.Generator(np.random.PCG64(STATE_SEEDS[name]))
    p0 = 0.088 + side * rng.random((n, 3))
    p0[ALONE] = ALONE_AT
    v = 5e-4 * rng.standard_normal((n, 3))
    obs = np.zeros((L.k, n, L.D), F32)
    for c in L.payload:
        obs[:, :, c] = rng.standard_normal((L.k, n)).astype(F32)
    if L.ctrl >= 0:
        obs[:, :, L.ctrl:L.ctrl + 3] = (1e-3 * rng.standard_normal((L.k, n, 3))).astype(F32)
    for t in range(L.k):
        obs[t, :, L.cart:L.cart + 3] = (p0 + (t - (L.k - 1)) * v + 1e-5 * rng.standard_normal((n, 3))).astype(F32)
    mat = np.zeros(n, F32)
    mat[n - n // 10:] = 1.0
    mat[list(wc.OTHER_MATERIAL_ROWS)] = 2.0
    obs[:, :, L.mat] = mat
    obs.setflags(write=False)
    return obs


def step_state(name):
    return state(name, "default", STEP_N, STEP_SIDE)


def rigid_rows(obs, L):
    return np.nonzero(np.asarray(obs)[-1][:, L.mat] == 1)[0]


def rigid_target(obs, L, seed, step_size=3e-4):
    """[n_rigid, 3] float32: the rigid rows' positions moved along one seeded direction, plus a seeded per-row offset (so that the
    rows of a target are told apart by their gradients)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    base = np.asarray(obs)[-1][rigid_rows(obs, L)][:, L.cart:L.cart + 3].astype(np.float64)
    d = rng.standard_normal(3)
    return (base + d / np.linalg.norm(d) * step_size + 2e-5 * rng.standard_normal(base.shape)).astype(F32)


@functools.lru_cache(maxsize=None)
def radius_edges(name, layout=None, n=wc.SCENE_N, side=0.06):
    """The oracle's radius graph [2, E] on the last frame of `state` (computed once)."""
    obs = state(name, layout, n, side)
    L = wc.LAYOUTS[layout or name]
    s, r = orc.get_connectivity(obs[-1][:, L.cart:L.cart + 3], R, 20)
    ei = np.ascontiguousarray(np.stack((s, r)).astype(np.int64))
    ei.setflags(write=False)
    return ei


@functools.lru_cache(maxsize=None)
def multigraph():
    """(pos [HUB_N, 3] float32, edge_index [2, HUB_E]): the seeded hub / duplicate / self-loop / isolated-node multigraph of
    tests/train_cases.py (hub_graph), in its random edge order, over seeded positions."""
    ei = train_cases.hub_graph()
    pos = (0.3 + 0.05 * np.random.Generator(np.random.PCG64(831)).random((train_cases.HUB_N, 3))).astype(F32)
    return pos, ei


def regime(obs, L, ei):
    """What a case is there for, measured: counts of clamped / unclamped boundary features, the distance of the nearest unclamped
    value to +-1, the shortest non-self edge (in units of r), self edges, nodes whose only edge is their self edge, rigid rows."""
    u = unclamped_boundary(obs, L)
    pos = np.asarray(obs, np.float64)[-1][:, L.cart:L.cart + 3]
    s, r = ei
    self_e = s == r
    length = np.linalg.norm((pos[s] - pos[r]) / R, axis=1)
    n = pos.shape[0]
    deg = np.bincount(s, minlength=n) + np.bincount(r, minlength=n)
    self_deg = 2 * np.bincount(s[self_e], minlength=n)
    return dict(clamped=int((np.abs(u) > 1).sum()), unclamped=int((np.abs(u) < 1).sum()),
                unclamped_negative=int(((u < 0) & (u > -1)).sum()),
                kink_distance=float(np.abs(np.abs(u) - 1).min()),
                shortest_edge=float(length[~self_e].min()) if (~self_e).any() else np.inf,
                self_edges=int(self_e.sum()), only_self=int(((deg == self_deg) & (self_deg > 0)).sum()),
                rigid=int(len(rigid_rows(obs, L))))


def assert_in_regime(reg, n):
    assert reg["clamped"] > 0 and reg["unclamped"] > 0 and reg["unclamped_negative"] > 0, reg
    assert reg["kink_distance"] > 1e-6, reg
    assert reg["shortest_edge"] >= 1e-6, reg
    assert reg["self_edges"] >= n and reg["only_self"] >= 1 and reg["rigid"] > 0, reg


# ------------------------------------------------------------------------------------------ helpers shared by the two test files
def t64(a, grad=False, dtype=F64):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def weights(shape, seed):
    """Seeded float32 weights w of a loss (out * w).sum()."""
    return np.random.default_rng(seed).standard_normal(shape).astype(F32)


# ------------------------------------------------------------------------------------------ the ReLU flip allowance of input gradients
def flip_allowance(run, leaves, tau=1e-5, max_units=256):
    """oracle/torch_epd.relu_flip_allowance for INPUT gradients, per element instead of per tensor (an input gradient is not summed
    over rows: one unit of one edge moves that edge's row and its two nodes' rows, and nothing else).  run(forward) evaluates the
    float64 loss with `forward` as the model (torch_epd.epd_forward's signature; it records the hidden pre-activations).
    Returns ([per-element bound of each leaf], number of near-zero units)."""
    tape = []
    run(lambda *args: torch_epd.epd_forward_taped(*args, tape)).backward(retain_graph=True)
    units = torch_epd.near_zero_units(tape, tau, max_units)
    bounds = torch_epd.flip_bounds(tape, units, leaves)
    return [v.cpu().numpy() for v in bounds], len(units)   # (the leaves may live on a device: tests/test_gpu_offsets.py)


# ------------------------------------------------------------------------------------------ the step scene: references and allowance
L0 = wc.LAYOUTS["default"]


def step_allowance(params, obs_np, targets, edge_lists, w_o, w_p, end_grad=None):
    """flip_allowance of the unrolled restatement: ([bound for obs, bound for each target that is not None], units), evaluated once.
    end_grad: the gradient w.r.t. the end state that stands for a loss behind it (first order)."""
    def compute():
        p = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
        rows = torch.tensor(rigid_rows(obs_np, L0))
        obs = t64(obs_np, True)
        tg = [None if t is None else t64(t, True) for t in targets]

        def run(fwd):
            cur = obs
            for t, ei in zip(tg, edge_lists):
                cur, pred = step(p, cur, L0, rows, t, torch.tensor(ei), STEP_DIMS[4], STEP_DIMS[5], forward=fwd)
            if end_grad is not None:
                return (cur * t64(end_grad)).sum()
            return (cur * t64(w_o)).sum() + (pred * t64(w_p)).sum()
        return flip_allowance(run, [obs] + [t for t in tg if t is not None])
    return lazy(compute)


def step_reference(params, obs_np, targets, edge_lists, w_o, w_p, dtype, end_loss=None):
    """The unrolled restatement on the GPU's edge lists: gradients w.r.t. obs and every step's target of sum(next_obs * w_o) +
    sum(pred * w_p) over the last step -- or of end_loss(next_obs) (a function returning the gradient w.r.t. next_obs)."""
    p = {k: torch.tensor(v, dtype=dtype) for k, v in params.items()}
    rows = torch.tensor(rigid_rows(obs_np, L0))
    obs = t64(obs_np, True, dtype)
    tg = [None if t is None else t64(t, True, dtype) for t in targets]
    cur, preds = obs, []
    for t, ei in zip(tg, edge_lists):
        cur, pred = step(p, cur, L0, rows, t, torch.tensor(ei), STEP_DIMS[4], STEP_DIMS[5])
        preds.append(pred.detach().numpy())
    if end_loss is None:
        ((cur * t64(w_o, dtype=dtype)).sum() + (pred * t64(w_p, dtype=dtype)).sum()).backward()
    else:
        cur.backward(gradient=torch.tensor(end_loss(cur.detach().numpy()), dtype=dtype))
    return cur.detach().numpy(), preds, obs.grad.numpy(), [None if t is None else t.grad.numpy() for t in tg]


def split(what, got, g64, g32, allow):
    """d / d obs by the rule of tests/yardstick.py, position and control columns separately; the other columns -- zero (the
    material label) or the loss's own weights passed through the window shift, at most one float32 addition -- to 1e-6 of their
    maximum."""
    c, u = slice(L0.cart, L0.cart + 3), slice(L0.ctrl, L0.ctrl + 3)
    for name, cols in (("position", c), ("control", u)):
        part = (slice(None), slice(None), cols)
        within(f"{what} d_obs {name}", got[part], g64[part], g32[part], lambda: (allow()[0][0], allow()[1]), part)
    rest = [i for i in range(L0.D) if not (c.start <= i < c.stop or u.start <= i < u.stop)]
    err, bar = np.abs(got[:, :, rest] - g64[:, :, rest]).max(), 1e-6 * max(np.abs(g64[:, :, rest]).max(), 1e-30)
    assert err <= bar, (what, "columns other than position and control", err, bar)
