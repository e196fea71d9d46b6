"""CPU: the restatements of tests/train_accum_cases.py against torch, and the regimes of the GPU cases.

Bounds.  The clip coefficient: 1e-12 relative against torch.nn.utils.clip_grad_norm_ in float64 (two float64 summation orders of
about 2000 squares, a square root and a division).  Several updates of mean + clip + Adam: per kind of tensor, the restatement's
error against float64 clip_grad_norm_ + torch.optim.Adam is at most 4 x what the same float32 torch loop shows, the bar
tests/test_train_step_cases.py holds Adam to.  The regimes: the clip of the GPU cases lies a factor 1.5 on the side of the oracle's
norm it is meant to lie on."""
import math

import numpy as np
import pytest
import torch

import train_accum_cases as ac
import train_step_cases as sc


def _torch_update(params, sample_grads, max_norm, dtype):
    """The mean of the samples' gradients into p.grad, then clip_grad_norm_: (total norm, clip coefficient applied)."""
    for p, *gs in zip(params, *sample_grads):
        total = torch.zeros_like(p)
        for g in gs:
            total = total + torch.tensor(g, dtype=dtype)
        p.grad = total / len(gs)
    before = [p.grad.clone() for p in params]
    norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    ratios = [float((p.grad.abs().max() / b.abs().max())) for p, b in zip(params, before) if float(b.abs().max()) > 0]
    return norm, ratios


def test_table_sits_on_the_reductions_edges():
    c = ac.SUMSQ_COUNTS
    wg, grid = ac.SUMSQ_WG, ac.SUMSQ_GRID_MAX
    assert (wg, grid) == (sc.LOSS_WG, sc.LOSS_GRID_MAX)
    assert {1, 3, 4, 5} <= set(c)                                                        # the tail alone, one float4, a float4 and a tail
    assert {wg - 1, wg, wg + 1, 4 * wg - 1, 4 * wg, 4 * wg + 1} <= set(c)                  # one workgroup's threads, its float4 groups
    assert {wg * grid - 1, wg * grid, wg * grid + 1} <= set(c)                           # one element per thread of a full grid
    assert {4 * wg * grid - 1, 4 * wg * grid, 4 * wg * grid + 5} <= set(c)               # one float4 per thread, then a second pass
    for n in c:
        x = ac.sumsq_case(n)
        assert x.dtype == np.float32 and len(x) == n and np.isfinite(x).all()
    big = max(sc.flat_count(d) for d in sc.STEP_MODELS.values())
    per_thread = -(-6_000_000 // (wg * grid))
    assert per_thread == 184 and (per_thread + 8 + 7) * 2.0 ** -53 < 3e-14 < ac.SUMSQ_RTOL and big < 6_000_000
    # squares of float32 extremes are float64 numbers, and sum exactly where the test says so
    assert float(np.float32(1e-30)) ** 2 > 0 and math.isfinite(float(np.float32(1e30)) ** 2)


def test_clip_coefficient_is_torchs():
    grads, p0 = ac.stub_gradients()
    seen = set()
    for u, sample_grads in enumerate(grads):
        params = [torch.nn.Parameter(torch.tensor(p, dtype=torch.float64)) for p in p0]
        norm, ratios = _torch_update(params, sample_grads, ac.STUB_MAX_NORM, torch.float64)
        total = [np.sum([g[i] for g in sample_grads], axis=0, dtype=np.float64).astype(np.float64) for i in range(len(p0))]
        mine = math.sqrt(sum(float((t ** 2).sum()) for t in total)) / ac.STUB_SAMPLES
        assert abs(mine - norm) <= 1e-12 * norm, (u, mine, norm)
        coef = ac.clip_coef(norm, ac.STUB_MAX_NORM)
        seen.add(coef < 1.0)
        for r in ratios:
            assert abs(r - coef) <= 1e-12, (u, r, coef)
        # ... and the restated norm of the float32 sum is that norm to float32 rounding of the sum
        sum32 = [np.sum([g[i] for g in sample_grads], axis=0, dtype=np.float32) for i in range(len(p0))]
        assert abs(ac.norm_of(sum32, ac.STUB_SAMPLES) - norm) <= 1e-6 * norm
    assert seen == {True, False}                                      # both regimes among the updates
    # no clip: the three spellings
    for off in (None, 0.0, -1.0, float("inf")):
        assert ac.clip_coef(123.0, off) == 1.0 and not ac.clipping(off)
    assert ac.scale_of(123.0, 1, None) == np.float32(1.0) and ac.scale_of(1.0, 4, None) == np.float32(0.25)
    assert ac.scale_of(2.0, 2, 1.0) == np.float32(min(1.0, 1.0 / (2.0 + 1e-6)) / 2.0)


def test_mean_clip_and_adam_against_float64_torch():
    grads, p0 = ac.stub_gradients()

    def torch_run(dtype):
        params = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in p0]
        opt = torch.optim.Adam(params, lr=ac.STUB_LR)
        for sample_grads in grads:
            _torch_update(params, sample_grads, ac.STUB_MAX_NORM, dtype)
            opt.step()
        return [[opt.state[p][k].detach().numpy().astype(np.float64) if k else p.detach().numpy().astype(np.float64) for p in params]
                for k in (None, "exp_avg", "exp_avg_sq")]

    ref64, ref32 = torch_run(torch.float64), torch_run(torch.float32)
    state = sc.adam_state(p0)
    p = p0
    scales = []
    for sample_grads in grads:
        total = [np.zeros_like(a) for a in p0]
        for g in sample_grads:                                         # the device's float32 accumulation
            total = [t + gi for t, gi in zip(total, g)]
        scale = ac.scale_of(ac.norm_of(total, ac.STUB_SAMPLES), ac.STUB_SAMPLES, ac.STUB_MAX_NORM)
        scales.append(float(scale))
        p = ac.scaled_adam_restated(p, total, state, ac.STUB_LR, scale)
    third = float(np.float32(1.0 / 3.0))
    assert scales[0] == third and scales[-1] < 0.5 * third and state["steps"] == ac.STUB_UPDATES
    for name, got, r64, r32 in zip(("weights", "exp_avg", "exp_avg_sq"), (p, state["m"], state["v"]), ref64, ref32):
        scale = max(np.abs(r).max() for r in r64)
        err = max(np.abs(a.astype(np.float64) - r).max() for a, r in zip(got, r64)) / scale
        e32 = max(np.abs(a - r).max() for a, r in zip(r32, r64)) / scale
        print(f"\n[accum adam] {name}: err {err:.3e}, float32 torch {e32:.3e}, ratio {err / e32:.2f}")
        assert e32 > 0 and err <= 4.0 * e32, (name, err, e32)


def test_mean_loss_is_the_running_sum():
    l = [0.1, 0.7, 1e-17]
    assert ac.mean_loss(l) == ((0.1 + 0.7) + 1e-17) / 3.0 and ac.mean_loss([2.5]) == 2.5
    assert math.isnan(ac.mean_loss([1.0, float("nan")]))


def test_the_gpu_cases_regimes():
    sizes = [s[0] for s in ac.SAMPLES]
    assert sorted(sizes) == [64, 257, 300] and any(n % 256 == 1 for n in sizes) and ac.DIMS == (25, 4, 3, 64, 2, 2)
    for i, n in enumerate(sizes):
        nodes, ea, ei, target = ac.sample(i)
        assert nodes.shape == (n, 25) and ei.shape[1] == len(ea) > 4 * n and 0 <= ei.min() and ei.max() < n and target.shape == (n, 3)
    losses, g = ac.oracle_gradients()
    assert all(math.isfinite(v) and v > 0 for v in losses)
    norm = ac.oracle_norm()
    print(f"\n[accum] the oracle's mean-gradient norm {norm:.6f}; clips {ac.CLIP_ACTIVE} / {ac.CLIP_INACTIVE}")
    assert norm / ac.CLIP_ACTIVE >= 1.5 and ac.CLIP_INACTIVE / norm >= 1.5
    assert ac.clip_coef(norm, ac.CLIP_ACTIVE) < 1 / 1.5 and ac.clip_coef(norm, ac.CLIP_INACTIVE) == 1.0
    assert sum(int(np.prod(v.shape)) for v in g.values()) <= sc.flat_count(ac.DIMS)


def test_python_surface():
    import inspect
    from gnn_manip_amd.train import Trainer
    assert Trainer.max_grad_norm is None and "max_grad_norm" not in inspect.signature(Trainer.__init__).parameters    # an attribute, like lr
    assert inspect.signature(Trainer.fit_epoch).parameters["accumulate"].default == 1
    sig = inspect.signature(Trainer.fit_rollout_epoch).parameters
    assert list(sig)[:7] == ["self", "dataset", "engine", "steps", "starts", "seed", "pos_scale"]
    assert (sig["batch_size"].default, sig["shuffle"].default) == (1, False)
    for name in ("zero_grad", "accumulate", "accumulate_rollout", "apply", "accum_record", "last_grad_norm"):
        assert hasattr(Trainer, name), name
    assert list(inspect.signature(Trainer.accumulate_rollout).parameters)[:4] == ["self", "engine", "obs0", "frames"]
    assert inspect.signature(Trainer.apply).parameters["loss_out"].default is None
