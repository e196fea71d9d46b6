"""CPU: the cases of dataset_stats_cases.py are in the regimes they exist for, and the references they carry agree with each other
within bounds that are derived, not tuned.

The bound used throughout is numpy's own worst case (``dc.summation_bound``): a float64 sum of n terms, in whatever order, is off
by at most n * u * sum|x| (u = 2^-53), so a mean by n * u * mean|x|; doubled for the terms' own rounding and the division.  The
exactly rounded form (``math.fsum``) is the side that carries no such error: it is what the GPU is held to, at 1e-12."""
import json
import os
import re

import numpy as np
import pytest

import dataset_stats_cases as dc
from conftest import GOLDEN, ROOT

GPU_BAR = 1e-12      # test_gpu_dataset_stats.py: M2 and standard deviations relative, means relative to mean|x|
SWEEP = [(t, n) for t in dc.T_SIZES for n in dc.N_SIZES]


def test_assumed_launch_shape_is_the_headers():
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    const = lambda name: int(re.search(r"#define\s+%s\s+(\d+)\b" % name, text).group(1))
    assert const("GM_RECORDING_STATS_MAX_WORKGROUPS") == dc.MAX_WORKGROUPS == 1024
    assert const("GM_RECORDING_STATS_DOUBLES") == dc.RECORD_DOUBLES == 24
    assert dc.ONE_PASS == 262144 and dc.ONE_PASS < dc.N_PAST_ONE_PASS < dc.ONE_PASS + dc.THREADS     # a second pass for some threads only
    assert set(dc.T_SIZES) == {3, 4, 9} and set(dc.N_SIZES) == {1, 63, 64, 65, 255, 256, 257, 1000}
    assert len({t for t, _ in dc.MERGE_SIZES}) == 3 and len({n for _, n in dc.MERGE_SIZES}) == 3


@pytest.mark.parametrize("kind", sorted(dc.KINDS))
def test_recordings_are_what_the_kind_says(kind):
    k = dc.KINDS[kind]
    assert 1 <= k.dim <= 3 and 0 <= k.cart0 and k.cart0 + k.dim <= dc.D
    for t, n in ((3, 1), (4, 65), (9, 1000)):
        rec = dc.recording(kind, t, n)
        assert rec.dtype == np.float32 and rec.shape == (t, n, dc.D) and np.isfinite(rec).all()
        assert rec is dc.recording(kind, t, n) and not rec.flags.writeable                    # one reference, shared and unchanged
        rows = dc.selected_rows(kind, rec)
        if k.block and n >= 10:
            rigid = rec[0, :, dc.MAT_COL] == 1.0
            assert 0 < rigid.sum() < n and rigid[-1] and not rigid[0]
            assert rows.sum() == {None: n, 0.0: n - rigid.sum(), 1.0: rigid.sum()}[k.material]
            vel, _ = dc.samples(rec, k.cart0, k.dim)
            vel = vel.reshape(t - 1, n, k.dim)
            assert np.abs(vel[:, rigid]).min() > 1e-3 > 1e-4 > np.abs(vel[:, ~rigid]).max()   # a moving block beside still sand
        elif k.material is None:
            assert rows.all()
    assert dc.KINDS["first_column"].cart0 == 0 and dc.KINDS["last_column"].cart0 + 3 == dc.D
    assert dc.KINDS["last_column_dim1"].cart0 + 1 == dc.D and {dc.KINDS[q].dim for q in ("dim1", "dim2")} == {1, 2}


def test_scales_differ_by_axis():
    ref = dc.reference("scales", 9, 1000)
    s = ref["vel_std"]
    assert s[1] / s[0] > 1e3 and s[2] / s[1] > 1e2


@pytest.mark.parametrize("t,n", SWEEP)
def test_drift_has_its_mean_far_above_its_spread(t, n):
    ref = dc.reference("drift", t, n)
    _, mean, _, _ = ref["vel"]
    assert (np.abs(mean) / ref["vel_std"] > 1e2).all(), (np.abs(mean) / ref["vel_std"])


def _within_summation_bound(got, ref, what):
    """A recipe result (numpy sums) against the fsum form: means within the bound, variances within the same bound relative."""
    for q in ("vel", "acc"):
        n, mean, m2, mabs = ref[q]
        err = np.abs(got[q + "_mean"] - mean)
        assert (err <= dc.summation_bound(n, mabs)).all(), (what, q, "mean", err, dc.summation_bound(n, mabs))
        var, var_ref = got[q + "_var"], m2 / n
        assert (np.abs(var - var_ref) <= 2.0 * n * dc.U * var_ref).all(), (what, q, "variance", var, var_ref)


@pytest.mark.parametrize("kind", sorted(dc.KINDS))
def test_recipe_agrees_with_the_fsum_form(kind):
    k = dc.KINDS[kind]
    for t, n in SWEEP:
        rec = dc.recording(kind, t, n)
        rows = dc.selected_rows(kind, rec)
        if not rows.any():
            assert dc.reference(kind, t, n)["vel"][0] == 0       # the filter keeps nothing here (a block of one row, sand asked for)
            continue
        _within_summation_bound(dc.recipe([rec], k.cart0, k.dim, [rows]), dc.reference(kind, t, n), (kind, t, n))


def test_one_pass_sum_of_squares_misses_the_gpu_bar_on_drift():
    """sumsq - n * mean^2 in float64 loses about (mean / std)^2 * u of the variance: far outside the bar the kernel is held to, on
    the very case the kernel is held to it -- the case tells the two schemes apart."""
    k = dc.KINDS["drift"]
    vel, _ = dc.samples(dc.recording("drift", 9, 1000), k.cart0, k.dim)
    _, _, m2, _ = dc.reference("drift", 9, 1000)["vel"]
    rel = np.abs(dc.one_pass_m2(vel) - m2) / m2
    assert (rel > 100 * GPU_BAR).any() and (rel > GPU_BAR).all(), rel
    # ... and not on ordinary jitter, where it is a fine scheme: the drift is what separates them
    vel, _ = dc.samples(dc.recording("jitter", 9, 1000), 2, 3)
    _, _, m2, _ = dc.reference("jitter", 9, 1000)["vel"]
    assert (np.abs(dc.one_pass_m2(vel) - m2) / m2 < GPU_BAR).all()


@pytest.mark.parametrize("kind", ["jitter", "drift", "scales", "block_all"])
def test_chans_merge_of_three_recordings_is_the_recipe_on_their_concatenation(kind):
    """The merged means are float64 numbers: each carries u |mean|, and the merge squares differences of them.  That is inside the
    bound while |mean| / std stays below about 1e4 (drift: 1e3); block_rigid (3e5: rows that differ by float32 rounding alone) is
    beyond what a merge of float64 records can hold and is not merged here -- within one recording the kernel's shift covers it."""
    from gnn_manip_amd.dataset import chan_merge
    k = dc.KINDS[kind]
    recs = [dc.recording(kind, t, n) for t, n in dc.MERGE_SIZES]
    rows = [dc.selected_rows(kind, r) for r in recs]
    whole = dc.fsum_moments(recs, k.cart0, k.dim, rows)
    for merge in (chan_merge, dc.chan):
        got = {}
        for q in ("vel", "acc"):
            acc = (0.0, np.zeros(k.dim), np.zeros(k.dim))
            for t, n in dc.MERGE_SIZES:
                cnt, mean, m2, _ = dc.reference(kind, t, n)[q]
                acc = merge(acc, (float(cnt), mean, m2)) if acc[0] else (float(cnt), mean, m2)
            assert acc[0] == whole[q][0]
            got[q + "_mean"], got[q + "_var"] = acc[1], acc[2] / acc[0]
        _within_summation_bound(got, whole, (kind, merge.__name__))
        _within_summation_bound(dc.recipe(recs, k.cart0, k.dim, rows), whole, (kind, "recipe"))


@pytest.mark.parametrize("kind", dc.FIXTURE_KINDS)
def test_restatement_is_the_references_own_script(kind):
    """tests/golden/dataset_stats_metadata.json is what simulation/generate_metadata.py wrote for these recordings as CSV files
    (make_dataset_stats_golden.py).  Both sides are numpy sums of the same numbers, in the order the script happened to list
    the files: twice the summation bound.  The script read decimal text: a position may be one float64 ulp off the float32 it
    stands for, a velocity two, so a mean moves by at most 4 u max|p| and a standard deviation (1-Lipschitz in the largest
    change of a sample; accelerations: four ulps) by 8 u max|p|."""
    k = dc.KINDS[kind]
    with open(os.path.join(GOLDEN, "dataset_stats_metadata.json")) as fp:
        fix = json.load(fp)[kind]
    recs = [dc.recording(kind, t, n) for t, n in dc.FIXTURE_SIZES]
    assert fix["sequence_length"] == dc.FIXTURE_SIZES[0][0] and fix["data_dim"] == dc.D and fix["dim"] == k.dim
    assert fix["cartesian_idx"] == list(range(k.cart0, k.cart0 + k.dim))
    got, exact = dc.recipe(recs, k.cart0, k.dim), dc.fsum_moments(recs, k.cart0, k.dim)
    pmax = max(float(np.abs(r[:, :, k.cart0:k.cart0 + k.dim]).max()) for r in recs)
    for q in ("vel", "acc"):
        n, _, m2, mabs = exact[q]
        parse = 8.0 * dc.U * pmax
        assert (np.abs(got[q + "_mean"] - np.asarray(fix[q + "_mean"])) <= 2.0 * dc.summation_bound(n, mabs) + parse).all(), (kind, q)
        std = np.sqrt(m2 / n)
        assert (np.abs(got[q + "_std"] - np.asarray(fix[q + "_std"])) <= 2.0 * (2.0 * n + 2.0) * dc.U * std + parse).all(), (kind, q)


def test_clump_is_past_the_cap_and_clear_of_the_radius():
    p = dc.clump()
    assert p.dtype == np.float32 and p.shape == (600, 3) and np.unique(p, axis=0).shape[0] == 600         # coincident-free
    assert dc.clump_margin(p) > dc.CLUMP_MARGIN                                                             # no d2 within 1e-6 of r * r
    counts = dc.brute_counts(p, dc.CLUMP_R)
    assert (counts[100:300] >= 200).all() and counts.max() > 160 and counts.min() >= 1
    assert (counts <= 20).any() and (counts <= 255).all()
    rec = dc.clump_recording()
    assert np.array_equal(rec[0, :, 2:5], p) and dc.brute_counts(rec[-1, :, 2:5], dc.CLUMP_R).max() < counts.max()
