"""Cases and numpy restatements of the library's training step (csrc/train_step.hip; the contract is in include/gnn_manip_hip.h)
-- a plain helper module (no test) of tests/test_train_step_cases.py (CPU: the restatements against torch, the table's own regime),
tests/test_abi_train_step.py and tests/test_gpu_train_step.py (the kernels against the restatements, bit for bit).

The loss: the float64 sum of the float32 values |pred - target| over the counted rows, divided by their count; its gradient is
sign(pred - target) * (float)(1.0 / count).  Adam: float64 scalars (running products of the betas), float32 elements with every
operation rounded on its own -- numpy's float32 arithmetic is exactly that."""
import math

import numpy as np

# ---------------------------------------------------------------------------------------------- the loss kernel's geometry
LOSS_WG = 256           # threads of a workgroup of the loss kernels, one row each per pass (kLossThreads)
LOSS_GRID_MAX = 128     # workgroups of a pass at most (kLossGridMax): rows past LOSS_WG * LOSS_GRID_MAX are a further pass
LOSS_ROWS = (1, 255, 256, 257, 300, 50_000)
LOSS_OUT_DIMS = (2, 3)
LOSS_NODE_DIM = 6
# name -> mask column (None: plain); "empty": a mask that counts no row
LOSS_MASKS = {"plain": None, "last": LOSS_NODE_DIM - 1, "middle": 2, "empty": LOSS_NODE_DIM - 1}


def loss_regime(n):
    """(workgroups launched, passes of the grid) for n rows."""
    groups = -(-n // LOSS_WG)
    return min(groups, LOSS_GRID_MAX), -(-groups // LOSS_GRID_MAX)


def loss_case(n, out_dim, mask, seed=0):
    """(pred, target, nodes, mask_col) of a case: normal values, ONE exactly equal element on a counted row (sign 0), a 0 / 1
    material flag in the mask column (at least one row of each kind where n allows) and other values in the other columns."""
    rng = np.random.default_rng([seed, n, out_dim, sorted(LOSS_MASKS).index(mask)])
    pred = rng.standard_normal((n, out_dim)).astype(np.float32)
    target = rng.standard_normal((n, out_dim)).astype(np.float32)
    nodes = rng.standard_normal((n, LOSS_NODE_DIM)).astype(np.float32)
    col = LOSS_MASKS[mask]
    if col is not None:
        flag = (rng.random(n) < 0.4).astype(np.float32)
        flag[n // 2] = 0.0                       # counted
        if n > 1:
            flag[(n // 2 + 1) % n] = 1.0         # not counted
        if mask == "empty":
            flag[:] = 1.0
        nodes[:, col] = flag
        for other in (c for c in range(LOSS_NODE_DIM) if c != col):
            nodes[:, other] = 1.0 - flag          # reading the wrong column counts the wrong rows
    target[n // 2, out_dim - 1] = pred[n // 2, out_dim - 1]
    return pred, target, nodes, -1 if col is None else col


def l1_restated(pred, target, nodes=None, mask_col=-1):
    """(loss float64, rows counted, grad float32 [n, out_dim]) as gm_l1_loss defines them."""
    pred, target = np.asarray(pred, np.float32), np.asarray(target, np.float32)
    counted = np.ones(len(pred), bool) if mask_col < 0 else np.asarray(nodes, np.float32)[:, mask_col] < np.float32(0.5)
    count = int(counted.sum())
    d = pred - target                                                   # float32
    grad = np.zeros_like(pred)
    if count == 0:
        return float("nan"), 0, grad
    loss = float(np.abs(d)[counted].astype(np.float64).sum() / count)
    grad[counted] = np.sign(d[counted]) * np.float32(1.0 / count)
    return loss, count, grad


# ---------------------------------------------------------------------------------------------- Adam
def adam_state(shapes_or_arrays):
    """Zero moments for a list of arrays, and the scalar record of a trainer that has not stepped."""
    return {"m": [np.zeros_like(np.asarray(a, np.float32)) for a in shapes_or_arrays],
            "v": [np.zeros_like(np.asarray(a, np.float32)) for a in shapes_or_arrays],
            "b1p": 1.0, "b2p": 1.0, "steps": 0}


def adam_restated(params, grads, state, lr, betas=(0.9, 0.999), eps=1e-8):
    """One step of the library's Adam on float32 arrays, in place on `state` (adam_state) and returning the new parameters.
    Scalars in float64 (Python floats), elements in float32 with every operation rounded on its own."""
    f = np.float32
    state["b1p"] *= betas[0]
    state["b2p"] *= betas[1]
    state["steps"] += 1
    step = f(lr / (1.0 - state["b1p"]))
    s2 = f(math.sqrt(1.0 - state["b2p"]))
    b1, o1, b2, o2, e = f(betas[0]), f(1.0 - betas[0]), f(betas[1]), f(1.0 - betas[1]), f(eps)
    out = []
    for i, (p, g) in enumerate(zip(params, grads)):
        p, g = np.asarray(p, f), np.asarray(g, f)
        m = (b1 * state["m"][i]) + (o1 * g)
        v = (b2 * state["v"][i]) + ((o2 * g) * g)
        state["m"][i], state["v"][i] = m, v
        out.append(p - step * (m / ((np.sqrt(v) / s2) + e)))
        assert out[-1].dtype == f and m.dtype == f and v.dtype == f
    return out


ADAM_STEPS, ADAM_LR, ADAM_ELEMENTS = 20, 1e-3, 4099


def adam_gradients(seed=5):
    """[ADAM_STEPS, ADAM_ELEMENTS] float32 gradients with magnitudes from 1e-6 to 10, both signs, and exact zeros -- some elements
    zero at every step, some at some steps -- and the start parameters."""
    rng = np.random.default_rng(seed)
    g = (10.0 ** rng.uniform(-6, 1, (ADAM_STEPS, ADAM_ELEMENTS)) * rng.choice([-1.0, 1.0], (ADAM_STEPS, ADAM_ELEMENTS))).astype(np.float32)
    g[rng.random(g.shape) < 0.1] = 0.0
    g[:, :7] = 0.0
    return g, rng.standard_normal(ADAM_ELEMENTS).astype(np.float32)


# ---------------------------------------------------------------------------------------------- models
def tensor_shapes(dims):
    """Shapes of an EncProcDecGNN's tensors in state_dict order; dims = (node_dim, edge_dim, out_dim, hidden, num_layers, m_steps)."""
    node_dim, edge_dim, out_dim, h, nl, m = dims

    def mlp(fin, fout, norm):
        s = [(h, fin), (h,)]
        for _ in range(nl - 1):
            s += [(h, h), (h,)]
        s += [(fout, h), (fout,)]
        return s + ([(fout,), (fout,)] if norm else [])

    shapes = mlp(edge_dim, h, True) + mlp(node_dim, h, True)
    for _ in range(m):
        shapes += mlp(3 * h, h, True) + mlp(2 * h, h, True)
    return shapes + mlp(h, out_dim, False)


def flat_count(dims):
    """Floats Adam's flat launch walks: every tensor starts on 16 bytes in the model's flat buffer, the walk ends with the last
    tensor (the decoder's bias, out_dim floats) -- so out_dim decides the scalar tail."""
    off = 0
    for s in tensor_shapes(dims):
        count = int(np.prod(s))
        end = off + count
        off += (count + 3) & ~3
    return end


# the models of the step tests: (dims, nodes, side of the scene, seed); N ~ 300 and E ~ 4000
SMALL = (25, 4, 3, 64, 2, 2)
# "h256_m3": more floats than ONE pass of the flat Adam launch's capped grid walks (2048 workgroups x 256 threads x 4 floats)
STEP_MODELS = {"h64": SMALL, "h128": (25, 4, 3, 128, 2, 2), "h256": (25, 4, 3, 256, 2, 2), "h64_out4": (25, 4, 4, 64, 2, 2),
               "h256_m3": (25, 4, 3, 256, 2, 3)}
SCENE = dict(n=300, side=0.05)
MATERIAL_COL = -1 - 3        # train_dyn.py:60 with three control columns, from the end of the 25 node features


def scene_graph(seed, n=None, side=None):
    from train_cases import graph
    return graph(n or SCENE["n"], side or SCENE["side"], seed)


def step_target(nodes, out_dim, seed):
    return np.random.default_rng(seed).standard_normal((nodes.shape[0], out_dim)).astype(np.float32)


# the learning-rate schedules of train_dyn.py:100-107,143-144 as host formulas
def lr_linear(lr0, lr_final, epoch, epochs):
    """SWALR(anneal_strategy='linear', anneal_epochs=epochs, swa_lr=lr_final) after `epoch` scheduler steps."""
    a = min(1.0, epoch / epochs)
    return lr_final * a + lr0 * (1.0 - a)


def lr_exponential(lr0, gamma, epoch, start=500):
    """ExponentialLR(gamma), stepped once per epoch from epoch `start` + 1 on (train_dyn.py:143: ``ep > 500``, ep counted from 0):
    the rate in force DURING epoch `epoch`."""
    return lr0 * gamma ** max(0, epoch - start - 1)
