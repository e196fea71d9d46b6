"""Planner loss on the device: the ``geomloss.SamplesLoss(loss="sinkhorn", p=2, blur=.05)`` the reference builds at
gnn_manip/utils/traj_utils.py:69 and calls at :279.  geomloss is an un-vendored pip dependency of the reference
(environment.yml:25, version not pinned): csrc/sinkhorn.hip restates its published algorithm; see the header there.

The loss is differentiable like geomloss's: ``loss(x, y).backward()`` fills ``x.grad`` / ``y.grad`` through HIP kernels
(gm_sinkhorn_divergence_batched_backward).  The gradient follows geomloss's convention for its tensorized backend, read from
its published code and -- like the forward -- unpinned against geomloss itself: the potentials are detached and only the last
extrapolation at eps = blur^2 is differentiated, with the right-hand cloud of every cost matrix detached; dS/dx_i is
(1/N) (T_xx(x_i) - T_xy(x_i)), the difference of the softmax barycentres of x_i over x and over y.  Double backward is not
supported.

Weighted clouds -- geomloss's ``loss(a, x, b, y)`` -- go through gm_sinkhorn_divergence_weighted and its backward: the softmins
and barycentres carry log a / log b in place of -log N / -log M, the cost is <a, b_x - a_x> + <b, a_y - b_y> and a row's gradient
has the factor a_i in place of 1/N (formulas and conventions: include/gnn_manip_hip.h).  The two-argument call is untouched.
"""
import torch
from torch.autograd.function import once_differentiable

from ._lib import check, current_stream, lib, ptr
from .graph import _need_cuda, _ws


def _workspace_bytes(x, y, a, b):
    if a is None and b is None:
        return lib().gm_sinkhorn_batched_workspace_bytes(x.shape[0], x.shape[1], y.shape[-2])
    return lib().gm_sinkhorn_weighted_workspace_bytes(x.shape[0], x.shape[1], y.shape[-2], a is not None, b is not None, y.dim() == 2)


def _forward(loss, x, y, ws, a=None, b=None):
    """Launch the batched divergence of x [B, N, 3] against y ([M, 3] or [B, M, 3]) with workspace ws -> [B] device tensor.
    a / b: the clouds' weights or None; without any, the unweighted entry point."""
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    shared = 1 if y.dim() == 2 else 0
    if a is None and b is None:
        check(lib().gm_sinkhorn_divergence_batched(ptr(x), x.shape[0], x.shape[1], ptr(y), y.shape[-2], shared, loss.blur,
                                                   loss.scaling, loss.diameter, ptr(out), ptr(ws), ws.numel(), current_stream()))
    else:
        check(lib().gm_sinkhorn_divergence_weighted(ptr(a), ptr(x), x.shape[0], x.shape[1], ptr(b), ptr(y), y.shape[-2], shared, loss.blur,
                                                    loss.scaling, loss.diameter, ptr(out), ptr(ws), ws.numel(), current_stream()))
    return out


class _SinkhornFunction(torch.autograd.Function):
    """SamplesLoss.batched under autograd: the forward runs in a workspace of the call's own (the backward reads its plan and
    potentials, which the next call would overwrite in the loss's shared one); the backward is
    gm_sinkhorn_divergence_batched_backward, or gm_sinkhorn_divergence_weighted_backward when a cloud carries weights (a, b:
    constants, no gradient)."""

    @staticmethod
    def forward(ctx, loss, x, y, a, b):
        ws = _ws(_workspace_bytes(x, y, a, b), x.device)
        out = _forward(loss, x, y, ws, a, b)
        ctx.loss, ctx.ws, ctx.weights = loss, ws, (a, b)
        ctx.save_for_backward(x, y)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        if ctx.ws is None:
            raise RuntimeError("SamplesLoss: a call's backward runs once (its workspace is released after it)")
        L = lib()
        x, y = ctx.saved_tensors
        a, b = ctx.weights
        bsz, n, m, shared = x.shape[0], x.shape[1], y.shape[-2], 1 if y.dim() == 2 else 0
        need_x, need_y = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx = torch.empty_like(x) if need_x else None
        dy = torch.empty_like(y) if need_y else None
        grad_loss = grad_loss.contiguous().float()
        ws = _ws(L.gm_sinkhorn_batched_backward_workspace_bytes(bsz, n, m, shared if need_y else 0), x.device)
        if a is None and b is None:
            check(L.gm_sinkhorn_divergence_batched_backward(ptr(x), bsz, n, ptr(y), m, shared, ctx.loss.blur, ctx.loss.scaling,
                                                            ptr(grad_loss), ptr(dx), ptr(dy), ptr(ctx.ws), ctx.ws.numel(), ptr(ws),
                                                            ws.numel(), current_stream()))
        else:
            check(L.gm_sinkhorn_divergence_weighted_backward(ptr(a), ptr(x), bsz, n, ptr(b), ptr(y), m, shared, ctx.loss.blur, ctx.loss.scaling,
                                                             ptr(grad_loss), ptr(dx), ptr(dy), ptr(ctx.ws), ctx.ws.numel(), ptr(ws),
                                                             ws.numel(), current_stream()))
        ctx.ws = None
        return None, dx, dy, None, None


def _weights(w, name, shape, like):
    """A cloud's weights as the library takes them: None, or a float32 tensor of `shape` on the cloud's device (a constant)."""
    if w is None:
        return None
    if not torch.is_tensor(w) or w.dtype != torch.float32 or w.device != like.device or tuple(w.shape) != tuple(shape):
        raise ValueError(f"SamplesLoss: weights {name} must be a float32 tensor of shape {list(shape)} on the clouds' device {like.device}")
    if w.requires_grad:
        raise ValueError(f"SamplesLoss: weights {name} are constants (no gradient with respect to the weights): detach them")
    return w.contiguous()


class SamplesLoss:
    """Callable with geomloss' constructor keywords; only what the reference uses is served (loudly otherwise).

    ``loss(x, y)`` is the reference's call (traj_utils.py:279): one pair, a 0-dim tensor.  ``loss.batched(X, y)`` takes the
    final clouds of a whole block of candidates, X [B, N, 3], against the desired cloud y [M, 3] (or one per candidate,
    [B, M, 3]) in ONE launch sequence and returns the B losses as a device tensor -- element b bit-equal to ``loss(X[b], y)``.
    ``diameter`` (geomloss keyword, default None = bounding box of each pair): given, no host synchronisation happens at all;
    otherwise one per call (the launch count is the longest epsilon schedule of the batch).

    ``loss(a, x, b, y)`` is geomloss's weighted call: a [N] and b [M] are the masses of the points (float32, on the clouds'
    device; either may be None = uniform), and ``loss.batched(X, y, a=, b=)`` takes a [B, N] and b [M] with a shared y, [B, M]
    otherwise.  As in geomloss the weights are used as given -- not normalised, no mass-balance check -- and are constants: no
    gradient flows to them.  A zero weight drops its point (its gradient row is exactly 0), so clouds of different sizes share a
    batch by padding with zero-weight points; the default diameter is still the bounding box of ALL points, so pad with copies of
    real points or give ``diameter=``.  A weight that is negative or not finite, or a cloud whose weights sum to 0, raises GMError
    on the default path and gives a NaN loss when ``diameter=`` is given (nothing is read back then).

    Both calls are differentiable with respect to x and y (see the module docstring for the convention); with y shared by the
    batch, its gradient is the sum over the pairs.  Under grad (grad mode on and x or y requiring grad) a call runs in a
    workspace of its own, kept until its backward; otherwise calls reuse one workspace per SamplesLoss, as the planner's do."""

    def __init__(self, loss="sinkhorn", p=2, blur=0.05, scaling=0.5, debias=True, diameter=None, **unsupported):
        if loss != "sinkhorn" or p != 2 or not debias or unsupported:
            raise NotImplementedError("SamplesLoss: only loss='sinkhorn', p=2, debias=True (the reference's configuration, "
                                      "traj_utils.py:69) runs on the HIP device")
        self.blur, self.scaling = float(blur), float(scaling)
        self.diameter = 0.0 if diameter is None else float(diameter)
        self._ws = None

    def batched(self, x, y, a=None, b=None):
        """x [B, N, 3], y [M, 3] or [B, M, 3] float32 CUDA tensors -> [B] float32 tensor on the device.  a [B, N], b [M] (y shared)
        or [B, M]: the points' weights, None = uniform."""
        _need_cuda(x, "x")
        _need_cuda(y, "y")
        x = x.contiguous().float()
        y = y.contiguous().float()
        if x.dim() != 3 or x.shape[2] != 3 or y.shape[-1] != 3 or y.dim() not in (2, 3) or (y.dim() == 3 and y.shape[0] != x.shape[0]):
            raise ValueError("SamplesLoss.batched: point clouds must be [B, N, 3] and [M, 3] or [B, M, 3]")
        a = _weights(a, "a", x.shape[:2], x)
        b = _weights(b, "b", y.shape[:-1], x)
        if torch.is_grad_enabled() and (x.requires_grad or y.requires_grad):
            return _SinkhornFunction.apply(self, x, y, a, b)
        need = _workspace_bytes(x, y, a, b)
        if self._ws is None or self._ws.numel() < need or self._ws.device != x.device:
            self._ws = _ws(need, x.device)
        return _forward(self, x, y, self._ws, a, b)

    def __call__(self, *args):
        """``loss(x, y)``: x [N, 3], y [M, 3] float32 CUDA tensors with uniform weights -> 0-dim float32 tensor on the device.
        ``loss(a, x, b, y)``: the same clouds with the weights a [N] and b [M] (either may be None)."""
        if len(args) not in (2, 4):
            raise TypeError(f"SamplesLoss: call loss(x, y) or loss(a, x, b, y), not with {len(args)} positional arguments")
        a, x, b, y = args if len(args) == 4 else (None, args[0], None, args[1])
        _need_cuda(x, "x")
        _need_cuda(y, "y")
        if x.dim() != 2 or y.dim() != 2 or x.shape[1] != 3 or y.shape[1] != 3:
            raise ValueError("SamplesLoss: point clouds must be [N, 3] and [M, 3]")
        a = _weights(a, "a", x.shape[:1], x)
        return self.batched(x.unsqueeze(0), y, None if a is None else a.unsqueeze(0), b)[0]
