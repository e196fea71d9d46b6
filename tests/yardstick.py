"""The project's accuracy rule for gradients, stated once -- a plain helper module of the GPU tests and of the CPU tests of their
references (tests/test_yardstick.py checks the rule itself).

Per tensor:  max |g - g64| <= max(GRAD_TOL, 4 x the error of the SAME plain-PyTorch computation run in float32) x max |g64|,  g64 the
float64 reference (oracle/torch_epd.py for the model, tests/*_cases.py for a step or a rollout).  The float32 term exists because the
gradient of a ReLU network is discontinuous: one pre-activation whose sign differs between float32 and float64 arithmetic moves a
whole row's contribution (~1e-3 of a tensor at the sizes tested) -- plain PyTorch float32 shows exactly the same deviations on the
same tensors.

The only fallback is the ReLU flip allowance (oracle/torch_epd.py: near_zero_units, flip_bounds): what toggling the units of THIS
input whose float64 pre-activation lies within 1e-5 of its Linear's rms of zero can change, computed only where the plain bound
fails, never assumed, and added to the bound: |g - g64| <= tol x max |g64| + allowance.  The allowance is taken as given and
broadcast: a scalar per tensor (parameter gradients, which sum over rows) holds the tensor's largest error to tol + allowance; an
array (input gradients, where one unit moves the rows of one edge and its two nodes and nothing else) holds every element to its
own.  Every figure is printed before it is asserted."""
import numpy as np

GRAD_TOL = 2e-4


def lazy(fn):
    """fn() evaluated at most once: the tensors of one run share one allowance."""
    box = []

    def get():
        if not box:
            box.append(fn())
        return box[0]
    return get


def bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def tolerance(g64, g32):
    """Of one tensor: (tol, max |g64|, float32 torch's own error), the first and the last relative to the second."""
    scale = max(np.abs(g64).max(), 1e-12)
    e32 = np.abs(g32 - g64).max() / scale
    return max(GRAD_TOL, 4.0 * e32), scale, e32


def excess(what, got, g64, g32, allow=0.0):
    """One tensor against the rule, everything relative to max |g64|: (worst |got - g64| / (tol + allow), max error, tol, the
    errors unscaled, max |g64|, float32 torch's error).  At most 1 means within the rule.  allow: a scalar or an array of the
    tensor's shape, in the tensor's own units."""
    got, g64, g32 = (np.asarray(a, np.float64) for a in (got, g64, g32))
    assert got.shape == g64.shape, (what, got.shape, g64.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    tol, scale, e32 = tolerance(g64, g32)
    err = np.abs(got - g64)
    return ((err / scale) / (tol + allow / scale)).max(), err.max() / scale, tol, err, scale, e32


def within(what, got, g64, g32, allow=None, part=None, tag="[input grads]"):
    """The rule on one tensor.  allow: a function returning (the allowance, the number of units behind it), called only where the
    plain bound fails; part: the slice of the allowance that `got` is."""
    ratio, e, tol, err, scale, e32 = excess(what, got, g64, g32)
    print(f"\n{tag} {what}: err {e:.3e} tol {tol:.3e} (float32 torch {e32:.3e}), max |g64| {scale:.3e}")
    if ratio <= 1.0:
        return
    assert allow is not None, (what, e, tol)
    a, n_units = allow()
    a = a if part is None else a[part]
    over = err > tol * scale
    worst = float(excess(what, got, g64, g32, a)[0])
    print(f"{tag} {what}: {int(over.sum())} elements in {int(over.reshape(len(over), -1).any(axis=1).sum())} rows beyond the plain bound; "
          f"relu flip allowance over {n_units} units: worst err / (tol + allowance) {worst:.3e}")
    assert worst <= 1.0, (what, e, tol, worst, n_units)


def worst_tensor(got, ref64, ref32, allow=None):
    """The rule on every tensor of ref64 (got: the same names): the worst (name, err / (tol + allowance), err, tol), err and tol
    relative to the tensor's maximum (a per-tensor allowance is part of the tol reported).  allow: {name: allowance} or None."""
    worst = ("", 0.0, 0.0, 0.0)
    for name, r in ref64.items():
        a = allow[name] if allow else 0.0
        ratio, e, tol, _, scale, _ = excess(name, got[name], r, ref32[name], a)
        if allow and np.ndim(a) == 0:
            tol = tol + a / scale
        if ratio > worst[1]:
            worst = (name, ratio, e, tol)
    return worst


# What each caller's log shows of a comparison of many tensors (w: the worst tensor, w2: the same with the allowance).
_PLAIN = {"[regimes]": "\n[regimes] {what}: worst err/tol {w[1]:.3f} at {w[0]!r}"}
_FALLBACK = {"[regimes]": "[regimes] {what}: relu-flip fallback ran ({n_units} units): worst with allowance {w2[1]:.3f} at {w2[0]!r}",
             "[offsets]": "[offsets] gradient {w[0]}: err {w[2]:.3e} of its maximum against tol {w[3]:.3e}; with the ReLU flip allowance "
                          "the worst is {w2[0]}: err / (tol + allowance) {w2[1]:.3f}"}


def compare(got, ref64, ref32, allowance=None, tag=None, what=""):
    """Every tensor of ref64 within the rule; one beyond it is allowed only what `allowance()` -- ({name: allowance}, number of
    units), computed when needed -- adds.  Returns (the worst tensor without the allowance, the same with it -- or None where it was
    not needed)."""
    assert set(ref64) <= set(got), (what, sorted(set(ref64) - set(got)))
    worst = worst_tensor(got, ref64, ref32)
    if tag in _PLAIN:
        print(_PLAIN[tag].format(what=what, w=worst))
    if worst[1] <= 1.0:
        return worst, None
    assert allowance is not None, (what, worst)
    allow, n_units = allowance()
    worst2 = worst_tensor(got, ref64, ref32, allow)
    if tag in _FALLBACK:
        print(_FALLBACK[tag].format(what=what, w=worst, w2=worst2, n_units=n_units))
    assert worst2[1] <= 1.0, (what, worst, worst2, n_units)
    return worst, worst2
