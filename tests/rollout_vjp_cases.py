"""Cases and the float32 restatement of the two state updates' transposes (gm_state_pre_backward, gm_state_post_backward):
tests/test_rollout_vjp_cases.py holds the restatement to float64 autograd through grad_cases.state_pre / state_post on the CPU,
tests/test_gpu_rollout_vjp.py holds the HIP kernels to the restatement, bit for bit.

Both updates are linear in the window, the pose and the next positions, with coefficients 0 and +-1: every element of a transpose
is a copy, a negation or a sum of two terms of the upstream gradient.  The restatement forms them in float32 in the one order
there is, so a float32 device result has nothing to differ by.

Shapes: N on the wave (64) and workgroup (256) edges of a 256-thread launch, windows of k = 2 (the last frame is also the first
that shifts) and k = 6; rigid rows none, one (not the first row), every row; with and without a scripted pose."""
import numpy as np

import width_cases as wc

F32 = np.float32
SIZES = (1, 63, 64, 65, 257, 1000)
KS = (2, 6)
RIGID = ("none", "one", "all")
LAYOUTS = {2: wc.LAYOUTS["k2"], 6: wc.LAYOUTS["default"]}
CASES = [(n, k, rigid, has_target) for n in SIZES for k in KS for rigid in RIGID for has_target in (True, False)]


def case_id(c):
    return f"n{c[0]}-k{c[1]}-rigid_{c[2]}-{'target' if c[3] else 'no_target'}"


def rigid_rank(n, rigid):
    """int32 [n]: the rank of each rigid row among the rigid rows, -1 elsewhere (gm_rigid_rank's output)."""
    rank = np.full(n, -1, np.int32)
    if rigid == "one":
        rank[n // 2] = 0
    elif rigid == "all":
        rank[:] = np.arange(n)
    return rank


def gradient(n, k, seed):
    """Seeded upstream gradient [k, n, D] float32 for the layout of window length k."""
    L = LAYOUTS[k]
    return np.random.default_rng(seed).standard_normal((k, n, L.D)).astype(F32)


def state_pre_transpose(g, L, rank, has_target):
    """(d_obs_before [k, n, D], d_rigid_target [n_rigid, 3]) float32 from g = d_obs_after: a rigid row's control columns were
    replaced by (target - xyz), or by xyz without a target."""
    g = np.asarray(g, F32)
    out = g.copy()
    rows = np.nonzero(rank >= 0)[0]
    c, u = slice(L.cart, L.cart + 3), slice(L.ctrl, L.ctrl + 3)
    gu = g[-1][rows][:, u]
    gx = g[-1][rows][:, c]
    out[-1][rows, c] = (gx - gu) if has_target else (gx + gu)
    out[-1][rows, u] = 0
    d_target = np.zeros((len(rows), 3), F32)
    if has_target:
        d_target[rank[rows]] = gu
    return out, d_target


def state_post_transpose(g, L, rank, has_target):
    """(d_obs_before [k, n, D], d_next_pos [n, 3], d_rigid_target [n_rigid, 3]) float32 from g = d_obs_after: the window shifted by
    one frame; the last frame passed on every column but xyz (a non-rigid row: xyz came from next_pos; a rigid row with a pose: from
    the pose) or the whole row (a rigid row without one)."""
    g = np.asarray(g, F32)
    k, n, _ = g.shape
    out = np.zeros_like(g)
    out[1:] = g[:-1]
    rigid = rank >= 0
    c = slice(L.cart, L.cart + 3)
    passed = g[-1].copy()
    replaced = ~rigid | bool(has_target)
    passed[replaced, c] = 0
    last = g[-2] + passed                     # float32: frame k - 2 first, then what frame k - 1 passed on
    rows = np.nonzero(replaced)[0]
    last[rows, c] = g[-2][rows, c]            # a copy where nothing was passed on (not a sum with a zero: the sign of a zero)
    out[-1] = last
    d_next = np.where(rigid[:, None], F32(0), g[-1][:, c]).astype(F32)
    d_target = np.zeros((int(rigid.sum()), 3), F32)
    if has_target:
        d_target[rank[rigid]] = g[-1][rigid][:, c]
    return out, d_next, d_target


def ctype(decl):
    """The ctypes type _lib.py uses for a C parameter declaration."""
    import ctypes as C
    from gnn_manip_amd import _lib
    decl = decl.strip()
    if "*" in decl:
        if decl.startswith("const gm_feature_desc"):
            return _lib._FD
        if decl.startswith("const gm_model_desc"):
            return _lib._MD
        if decl.startswith("int64_t*"):
            return C.POINTER(C.c_int64)
        return C.c_void_p
    return {"int64_t": C.c_int64, "int": C.c_int, "size_t": C.c_size_t}[decl.rsplit(" ", 1)[0]]
