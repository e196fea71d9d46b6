"""Cases of the trajectory refinement (gnn_manip_amd.planner.projected_adam / refine_starts): a numpy restatement of Adam with
bias correction followed by the clamp to a box, written from the textbook formulas independently of the library's loop; a
separable quadratic in 6 variables whose minimiser lies outside the box in one coordinate; stub objectives; and the worker of
the two-rank gloo test.  No GPU is involved: the objective is a callable."""
import os

import numpy as np

DIM = 6
HALF_WIDTHS = np.array([0.5, 0.5, 0.5, 2e-3, 2e-3, 2e-3])          # two scales, like rotation and translation variables
CURVATURE = np.array([1.0, 4.0, 0.25, 3.0e4, 1.0e5, 2.0e4])
MINIMISER = np.array([0.2, -0.1, 0.9, 1e-3, -5e-4, 1.5e-3])         # coordinate 2 lies outside the box: 0.9 > 0.5
OUTSIDE = 2
PENALTY = 20.0                                                      # the planner's boundary penalty


def starts(p=3, seed=3):
    """p starts strictly inside the box."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.8, 0.8, (p, DIM)) * HALF_WIDTHS


def quadratic(X):
    """sum_j c_j (x_j - m_j)^2 / 2 per row and its gradient."""
    d = np.asarray(X, dtype=np.float64) - MINIMISER
    return 0.5 * (CURVATURE * d * d).sum(axis=1), CURVATURE * d


def adam_reference(grad, x0, half_widths, iters, lr, b1=0.9, b2=0.999, eps=1e-8):
    """ONE start.  z = x / half_widths; z_0 = clamp(z); per iteration t = 1..iters: g = dF/dz = half_widths dF/dx,
    m_t = b1 m + (1 - b1) g, v_t = b2 v + (1 - b2) g^2, z <- clamp(z - lr (m_t / (1 - b1^t)) / (sqrt(v_t / (1 - b2^t)) + eps), -1, 1).
    Returns the iterates [iters + 1, dim] in x."""
    z = np.minimum(np.maximum(np.asarray(x0, dtype=np.float64) / half_widths, -1.0), 1.0)
    m = np.zeros(len(z))
    v = np.zeros(len(z))
    out = [z * half_widths]
    for t in range(1, iters + 1):
        g = half_widths * grad(z * half_widths)
        for j in range(len(z)):                                     # coordinate by coordinate: nothing shared with a vectorised loop
            m[j] = b1 * m[j] + (1.0 - b1) * g[j]
            v[j] = b2 * v[j] + (1.0 - b2) * g[j] ** 2
            z[j] = min(max(z[j] - lr * (m[j] / (1.0 - b1 ** t)) / (np.sqrt(v[j] / (1.0 - b2 ** t)) + eps), -1.0), 1.0)
        out.append(z * half_widths)
    return np.stack(out)


class Counting:
    """An objective that records the rows of every call."""

    def __init__(self, fn=quadratic):
        self.fn, self.calls = fn, []

    def __call__(self, X):
        self.calls.append(np.array(X, dtype=np.float64))
        return self.fn(X)


class PenalisedAt:
    """The quadratic with PENALTY added to the value (not the gradient) of every row at call `at`: a boundary penalty that one
    iterate runs into."""

    def __init__(self, at):
        self.at, self.n = at, 0

    def __call__(self, X):
        f, g = quadratic(X)
        if self.n == self.at:
            f = f + PENALTY
        self.n += 1
        return f, g


GLOO_ITERS, GLOO_LR = 5, 0.05


def gloo_worker(rank, world, port, q):
    """refine_starts over world ranks with the counting quadratic as the block objective: what the rank got back, and the rows
    its objective saw.  Only rank 0 owns the starts."""
    import torch.distributed as dist
    from gnn_manip_amd.planner import refine_starts
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    obj = Counting()
    x, f, info = refine_starts(obj, starts(3) if rank == 0 else None, HALF_WIDTHS, iters=GLOO_ITERS, lr=GLOO_LR)
    q.put((rank, x, f, info["f"], [c[:, 0].tolist() for c in obj.calls]))
    dist.barrier()
    dist.destroy_process_group()
