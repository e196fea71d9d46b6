"""The optimiser on the MI355X on CHOSEN gradients (csrc/train_step.hip: rank_sum_kernel, the sum of squares, apply_prepare_kernel,
adam_flat_kernel; gm_trainer_import's beta powers), driven through the contribution door: Trainer.zero_grad(), reduce(gathered,
samples_total), apply() on caller-made contributions -- no forward, no backward -- against the numpy restatement of
tests/optim_cases.py (whose regimes tests/test_optim_cases.py checks on the CPU first).

Bounds.  No new tolerance.  The merged gradient, the weights and both moments of every tensor: bit equality with the restatement,
a NaN where the restatement holds a NaN (train_dp_cases.same_bits_or_nan).  Step counts and beta powers: equal.  scale: equal bits.
grad_norm: train_accum_cases.SUMSQ_RTOL.  The mean loss: 1e-12.  The import at the top of the accepted step range: no more than
3 x the wall time of the import at step 2,000,000, plus 0.5 s -- both run the host loop to the same fixed point.

Every drive prints the words it compared."""
import math
import time

import numpy as np
import pytest
import torch

from oracle import epd_oracle as orc
import optim_cases as oc
import train_accum_cases as ac
import train_dp_cases as dp
from gpu_support import dev, load_model, rank_sum, to_dev

pytestmark = pytest.mark.gpu

LR = 1e-3
CLIP = {"mixed": 1.0, "tiny": 1e-7}       # active on that schedule: below its norm (hundreds), below norm + 1e-6 (the formula's 1e-6)


# ------------------------------------------------------------------------------------------ the shared drive
class _Run:
    """A trainer on `dims`, the restatement's state beside it, and the words compared so far."""

    def __init__(self, dims, dev, betas=(0.9, 0.999), eps=1e-8, seed=870):
        from gnn_manip_amd import Trainer, train
        self.dev, self.lay, self.betas, self.eps = dev, oc.Layout(dims), betas, eps
        self.t = Trainer(load_model(orc.init_params(*dims, seed), dims, dev), lr=LR, betas=betas, eps=eps)
        self.kinds = (("p", train.PARAMS), ("m", train.EXP_AVG), ("v", train.EXP_AVG_SQ))
        self.grads = train.GRADS
        self.state = oc.start_state(self.lay, weights=self.lay.to_flat([a.cpu().numpy() for a in self.t.export(train.PARAMS)]), betas=betas)
        self.words = 0

    def packed(self, what):
        return torch.cat([a.reshape(-1) for a in self.t.export(what)]).cpu().numpy()

    def arrays(self):
        return {key: self.packed(what) for key, what in self.kinds}

    def load_moments(self, m, v, steps):
        """gm_trainer_import of both moments at step `steps`; the restatement starts from the same state."""
        self.t._import(self.kinds[1][1], [torch.from_numpy(a.copy()) for a in self.lay.from_flat(m)], steps)
        self.t._import(self.kinds[2][1], [torch.from_numpy(a.copy()) for a in self.lay.from_flat(v)])
        self.state = oc.start_state(self.lay, weights=self.state["p"], m=m, v=v, steps=steps, betas=self.betas)

    def step(self, rows, samples_total=1, max_grad_norm=None, want_norm=False, lr=LR, what=""):
        """zero_grad, reduce of the packed contributions, apply; then everything the device holds against the restated drive."""
        t, lay, state = self.t, self.lay, self.state
        rows = np.ascontiguousarray(rows, np.float32).reshape(-1, lay.alloc)
        world = rows.shape[0]
        tails = oc.tails_of(samples_total, world, state["steps"])
        t.max_grad_norm, t.lr = max_grad_norm, lr
        t.zero_grad()
        gathered = to_dev(np.stack([dp.pack_contribution(rows[r], tails[r]) for r in range(world)]), self.dev)
        assert gathered.shape == (world, t.contribution_bytes())
        t.reduce(gathered, samples_total)
        slot = torch.full((1,), 7.0, dtype=torch.float64, device=self.dev)
        t.apply(loss_out=slot, want_norm=want_norm)
        rec = oc.drive_restated(state, rows, tails, samples_total, lr, max_grad_norm, self.betas, self.eps, want_norm)
        got = self.arrays()
        got["grad"] = self.packed(self.grads)
        for key in ("grad", "p", "m", "v"):
            w = lay.packed(rec["grad"] if key == "grad" else state[key])
            differing = oc.words_differing(got[key], w)
            self.words += w.size
            assert dp.same_bits_or_nan(got[key], w), (what, key, f"{differing} of {w.size} words differ", np.nonzero(got[key].view(np.uint32) != w.view(np.uint32))[0][:8])
        r, a = t.record(), t.accum_record()
        assert (r["steps_applied"], r["steps_skipped"]) == (state["steps"], state["skipped"]), (what, r, state["steps"], state["skipped"])
        assert _bits(r["beta1_pow"]) == _bits(state["b1p"]) and _bits(r["beta2_pow"]) == _bits(state["b2p"]), (what, r, state["b1p"], state["b2p"])
        assert (a["samples"], a["bad"]) == (rec["samples"], rec["bad"]) and a["loss_sum"] == rec["loss_sum"], (what, a, rec["samples"], rec["bad"])
        assert _bits(np.float32(a["scale"])) == _bits(np.float32(rec["scale"])) and a["scale"] == float(np.float32(a["scale"])), (what, a["scale"], rec["scale"])
        if math.isfinite(rec["grad_norm"]):
            assert abs(a["grad_norm"] - rec["grad_norm"]) <= ac.SUMSQ_RTOL * rec["grad_norm"], (what, a["grad_norm"], rec["grad_norm"])
        else:
            assert _bits(a["grad_norm"]) == _bits(rec["grad_norm"]) or (math.isnan(a["grad_norm"]) and math.isnan(rec["grad_norm"])), (what, a, rec["grad_norm"])
        loss = float(slot)
        assert (math.isnan(loss) and math.isnan(rec["loss"])) or abs(loss - rec["loss"]) <= 1e-12 * abs(rec["loss"]), (what, loss, rec["loss"])
        return rec

    def done(self, what):
        self.t.status()
        print(f"\n[gpu optim] {what}: {self.words} words compared, 0 differing; state (denormal, inf, NaN) {oc.census(self.state, self.lay)}")


def _bits(x):
    """The word of a float32 (a numpy float32) or of a float64 (anything else)."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        x = x.astype(np.float64)
    return int(x.reshape(1).view(np.uint32 if x.dtype == np.float32 else np.uint64)[0])


# ------------------------------------------------------------------------------------------ 1. schedules x tails
@pytest.mark.parametrize("od", [1, 2, 3, 4])
@pytest.mark.parametrize("name", ["mixed", "tiny", "huge", "decay"])
def test_schedules_on_every_scalar_tail(dev, name, od):
    run = _Run(oc.TAIL_MODELS[od - 1], dev)
    assert run.t.contribution_bytes() == 4 * run.lay.alloc + 32 and run.lay.count % 4 == od % 4
    g = oc.schedule(name, run.lay)
    for k in range(oc.STEPS):
        rec = run.step(g[k], what=(name, od, k))
        assert rec["scale"] == 1.0 and not rec["skipped"]
    run.done(f"{name}, out_dim {od}, {oc.STEPS} steps")


@pytest.mark.parametrize("name,od", [("mixed", 3), ("tiny", 2)])
def test_schedules_over_three_ranks_with_an_active_clip(dev, name, od):
    run = _Run(oc.TAIL_MODELS[od - 1], dev)
    rows = oc.rank_rows(name, run.lay, oc.STEPS, 3)
    for k in range(oc.STEPS):
        rec = run.step(rows[k], samples_total=5, max_grad_norm=CLIP[name], what=(name, od, k))
        assert 0.0 < rec["scale"] < 0.5 * (1.0 / 5.0) and not rec["skipped"], rec["scale"]            # the clip bites: coef below a half
    run.done(f"{name}, out_dim {od}, 3 ranks, 5 samples, clip {CLIP[name]}")


# ------------------------------------------------------------------------------------------ 2. past one grid pass
@pytest.mark.parametrize("world,clip", [(3, CLIP["mixed"]), (1, None)])
def test_the_apply_path_past_one_grid_pass(dev, world, clip):
    run = _Run(oc.BIG, dev)
    lay = run.lay
    beyond = lay.beyond(oc.GRID_PASS)
    assert oc.GRID_PASS < lay.count < 2 * oc.GRID_PASS and lay.count % 4 == 3 and len(beyond) >= 4
    w0 = lay.from_flat(run.state["p"])
    rows = oc.rank_rows("mixed", lay, 3, world)
    for k in range(3):
        rec = run.step(rows[k], samples_total=world, max_grad_norm=clip, what=("big", world, k))
        assert not rec["skipped"]
        if clip is None:
            assert _bits(np.float32(run.t.accum_record()["scale"])) == _bits(np.float32(1.0))
        else:
            assert rec["scale"] < 0.5 / world
    got = [a.cpu().numpy() for a in run.t.export(run.kinds[0][1])]
    want = lay.from_flat(run.state["p"])
    for i in beyond:                                                      # what only a second trip of the grid-stride loops reaches
        assert (got[i] != w0[i]).mean() > 0.9, ("did not move", i, lay.shapes[i])
        assert np.array_equal(got[i].view(np.uint32), want[i].view(np.uint32)), i
    run.done(f"{lay.count} floats ({lay.count - oc.GRID_PASS} past one grid pass), world {world}, clip {clip}, 3 steps")


# ------------------------------------------------------------------------------------------ 4. gm_rank_sum around the line
@pytest.mark.parametrize("count", [oc.GRID_PASS - 1, oc.GRID_PASS, oc.GRID_PASS + 1, oc.GRID_PASS + 7, 2 * oc.GRID_PASS + 5])
def test_rank_sum_around_one_grid_pass(dev, count):
    words = 0
    for world in (1, 3):
        stride = (count + 3) // 4 * 4 + 8
        rows = dp.rank_sum_case(world, count, stride)
        want = dp.rank_sum_restated(rows[:, :count])
        got = rank_sum(rows, count, dev)                                   # asserts that the guard words behind dst stayed untouched
        assert np.isfinite(want).all() and np.abs(want).max() < 1e30       # the sentinel behind `count` stayed out
        differing = int((got.view(np.uint32) != want.view(np.uint32)).sum())
        assert differing == 0, (count, world, differing, np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0][:8])
        words += count
    print(f"\n[gpu optim] rank sum, count {count}: {words} words compared, 0 differing")


# ------------------------------------------------------------------------------------------ 5. eps and betas
@pytest.mark.parametrize("eps", [0.0, 1e-40, 1e-30, 1e-3])
def test_eps_and_betas(dev, eps):
    for betas in ((0.0, 0.0), (0.5, 0.5), (0.8, 0.99)):
        run = _Run(oc.OD3, dev, betas=betas, eps=eps)
        g = oc.schedule("mixed", run.lay, 6)
        for k in range(6):
            run.step(g[k], what=(eps, betas, k))
        nans = oc.census(run.state, run.lay)["p"][2]
        assert (nans >= oc.ALWAYS_ZERO) if eps == 0.0 else nans == 0          # 0 / (0 + 0) where a gradient has been zero from the start
        run.done(f"eps {eps}, betas {betas}, 6 steps")


# ------------------------------------------------------------------------------------------ 6. clip corners
@pytest.mark.parametrize("corner", ["zeros", "tiny_max_norm", "inf_max_norm", "max_norm_1e308", "million_samples", "lr_zero"])
def test_clip_corners(dev, corner):
    run = _Run(oc.OD3, dev)
    lay = run.lay
    g = oc.schedule("mixed", lay, 1)[0]
    if corner == "zeros":
        rec = run.step(np.zeros_like(g), max_grad_norm=1.0, what=corner)
        assert rec["grad_norm"] == 0.0 and rec["scale"] == 1.0 and run.t.accum_record()["grad_norm"] == 0.0
        assert not run.state["m"].any() and not run.state["v"].any() and run.state["steps"] == 1
    elif corner == "tiny_max_norm":
        rec = run.step(g, max_grad_norm=1e-30, what=corner)
        assert oc.denormals(rec["g1"]) > 1000 and 0.0 < rec["scale"] < 1e-31        # the scaled gradients underflow
    elif corner == "inf_max_norm":
        rec = run.step(g, max_grad_norm=float("inf"), what=corner)
        assert rec["scale"] == 1.0 and math.isnan(run.t.accum_record()["grad_norm"])    # no clip, and no norm either
    elif corner == "max_norm_1e308":
        rec = run.step(g, max_grad_norm=1e308, what=corner)
        assert rec["scale"] == 1.0 and rec["grad_norm"] > 100.0                       # a clip that never bites
    elif corner == "million_samples":
        rows = oc.rank_rows("mixed", lay, 1, 2)[0]
        rec = run.step(rows, samples_total=1_000_000, what=corner)
        assert rec["samples"] == 1_000_000 and rec["scale"] == float(np.float32(1e-6))
    else:
        before = run.arrays()
        rec = run.step(g, lr=0.0, what=corner)
        after = run.arrays()
        assert np.array_equal(after["p"].view(np.uint32), before["p"].view(np.uint32))       # the weights keep their bits
        assert (after["m"] != before["m"]).mean() > 0.8 and (after["v"] != before["v"]).mean() > 0.8 and run.state["steps"] == 1
    assert not rec["skipped"]
    run.done(corner)


# ------------------------------------------------------------------------------------------ 7. the skip rule
@pytest.mark.parametrize("request_norm", ["clip", "want_norm"])
def test_a_spike_with_a_requested_norm_is_skipped(dev, request_norm):
    kw = dict(max_grad_norm=1e4) if request_norm == "clip" else dict(want_norm=True)
    run, twin = _Run(oc.OD3, dev), _Run(oc.OD3, dev)
    g = oc.schedule("spike", run.lay, oc.SPIKE_STEP + 2)
    for k in range(oc.SPIKE_STEP):
        for r in (run, twin):
            assert not r.step(g[k], what=("before", k), **kw)["skipped"]
    before, rec0 = run.arrays(), run.t.record()
    rec = run.step(g[oc.SPIKE_STEP], what="the spike", **kw)
    assert rec["skipped"] and math.isnan(rec["loss"]) and not math.isfinite(rec["grad_norm"])
    after = run.arrays()
    for key in before:
        assert np.array_equal(after[key].view(np.uint32), before[key].view(np.uint32)), key
    assert run.t.record() == dict(rec0, steps_skipped=rec0["steps_skipped"] + 1)
    for r in (run, twin):
        assert not r.step(g[oc.SPIKE_STEP + 1], what="the next good step", **kw)["skipped"]
    a, b = run.arrays(), twin.arrays()
    for key in a:
        assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
    assert run.t.record() == dict(twin.t.record(), steps_skipped=1)
    twin.t.status()
    run.done(f"spike, norm requested by {request_norm}")


def test_a_spike_without_a_requested_norm_goes_through(dev):
    run = _Run(oc.OD3, dev)
    g = oc.schedule("spike", run.lay, oc.SPIKE_STEP + 2)
    for k in range(oc.SPIKE_STEP + 2):
        rec = run.step(g[k], what=("spike, no norm", k))
        assert not rec["skipped"] and math.isnan(rec["grad_norm"])
    c = oc.census(run.state, run.lay)
    assert c["p"][2] == 2 and c["m"][2] >= 1 and c["v"][1] + c["v"][2] == 2 and run.t.record()["steps_skipped"] == 0, c
    run.done("spike, no norm requested")


# ------------------------------------------------------------------------------------------ 8. late steps
@pytest.mark.parametrize("step_count", [1000, 100_000, 2_000_000])
def test_steps_after_an_import_at_a_late_step(dev, step_count):
    run = _Run(oc.OD3, dev)
    m, v = oc.late_moments(run.lay)
    assert (v[run.lay.used] > 0).all() and v[run.lay.used].min() < 1e-11 and v.max() > 10.0
    run.load_moments(m, v, step_count)
    rec = run.t.record()
    want = oc.running_powers(0.9, 0.999, step_count)                      # the plain loop
    assert rec["steps_applied"] == step_count and (_bits(rec["beta1_pow"]), _bits(rec["beta2_pow"])) == (_bits(want[0]), _bits(want[1])), (rec, want)
    assert (run.state["b1p"], run.state["b2p"]) == want
    got = run.arrays()
    assert np.array_equal(got["m"].view(np.uint32), run.lay.packed(m).view(np.uint32)) and np.array_equal(got["v"].view(np.uint32), run.lay.packed(v).view(np.uint32))
    g = oc.schedule("mixed", run.lay, 2)
    for k in range(2):
        assert not run.step(g[k], what=("late", step_count, k))["skipped"]
    assert run.state["steps"] == step_count + 2
    run.done(f"two steps after an import at step {step_count}")


# ------------------------------------------------------------------------------------------ 9. the top of the accepted range
def test_import_at_the_top_of_the_step_range_returns(dev):
    """gm_trainer_import rebuilds the beta powers with a host loop that ends at the products' fixed point (737,741 steps for the
    default betas), whatever step_count is."""
    run = _Run(oc.OD3, dev)
    m, v = oc.late_moments(run.lay)
    times = {}
    for step_count in (2_000_000, (1 << 40) - 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run.load_moments(m, v, step_count)
        torch.cuda.synchronize()
        times[step_count] = time.perf_counter() - t0
        rec = run.t.record()
        want = oc.running_powers_fixed(0.9, 0.999, step_count)
        assert rec["steps_applied"] == step_count and (_bits(rec["beta1_pow"]), _bits(rec["beta2_pow"])) == (_bits(want[0]), _bits(want[1])), (rec, want)
        assert want == (2.47e-323, 2.465e-321)
    small, big = times[2_000_000], times[(1 << 40) - 1]
    print(f"\n[gpu optim] import at step 2,000,000: {small:.4f} s; at step 2^40 - 1: {big:.4f} s")
    assert big <= 3.0 * small + 0.5, (small, big)
    g = oc.schedule("mixed", run.lay, 1)                                  # and the trainer steps on from there
    assert not run.step(g[0], what="after the import at 2^40 - 1")["skipped"]
    assert run.t.record()["steps_applied"] == 1 << 40
    run.done("one step after an import at step 2^40 - 1")
