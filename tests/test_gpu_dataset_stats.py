"""Dataset statistics and the neighbour census on the device (cases: dataset_stats_cases.py; their CPU side:
test_dataset_stats_cases.py, test_abi_dataset_stats.py).

Moments are held to the exactly summed restatement (``dc.fsum_moments``) at the project's bar for double sums (gm_grad_sumsq,
gm_rollout_errors): means within 1e-12 * mean|x|, M2 and standard deviations within 1e-12 relative; counts and the positions' range
are exact.  The census returns integers and is compared bit for bit: with gm_radius_graph_build, which predates it, wherever the
cap allows, and with a float64 brute force past the cap on geometry that keeps clear of the radius."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

import dataset_stats_cases as dc
import graph_cases as gc
from conftest import BOUNDS, ROOT
from gpu_support import dev, to_dev as _t

pytestmark = pytest.mark.gpu

BAR = 1e-12
SWEEP = [(t, n) for t in dc.T_SIZES for n in dc.N_SIZES]


# ------------------------------------------------------------------------------------------ gm_recording_stats through ctypes
def _stats(rec_t, cart0, dim, mcol, mval, dev, ws=None):
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    t, n, d = (int(v) for v in rec_t.shape)
    need = L.gm_recording_stats_workspace_bytes(t, n)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    out = torch.full((dc.RECORD_DOUBLES + 4,), -7.0, dtype=torch.float64, device=dev)
    check(L.gm_recording_stats(ptr(rec_t), t, n, d, cart0, dim, mcol, mval, ptr(out), ptr(ws), need, current_stream(dev)))
    out = out.cpu().numpy()
    assert (out[dc.RECORD_DOUBLES:] == -7.0).all(), "written past the record"
    return out[:dc.RECORD_DOUBLES].reshape(3, 8)


def _stats_of_kind(kind, t, n, dev, ws=None):
    k = dc.KINDS[kind]
    mcol, mval = (-1, 0.0) if k.material is None else (dc.MAT_COL, k.material)
    return _stats(_t(dc.recording(kind, t, n), dev), k.cart0, k.dim, mcol, mval, dev, ws)


def _hold(rec, ref, dim, what):
    """A device record [3, 8] against dc.fsum_moments' result.  Prints the worst fraction of the bar it used."""
    worst = 0.0
    for q, c in (("vel", 0), ("acc", 3)):
        n, mean, m2, mabs = ref[q]
        assert (rec[:dim, c] == n).all(), (what, q, "count", rec[:dim, c], n)
        if n == 0:
            assert (rec[:dim, c + 1:c + 3] == 0).all(), (what, q, "empty")
            continue
        e_mean = np.abs(rec[:dim, c + 1] - mean)
        e_m2 = np.abs(rec[:dim, c + 2] - m2)
        std, std_ref = np.sqrt(rec[:dim, c + 2] / n), np.sqrt(m2 / n)
        frac = max(float((e_mean / np.maximum(BAR * mabs, 1e-300)).max()), float((e_m2 / np.maximum(BAR * m2, 1e-300)).max()))
        worst = max(worst, frac)
        assert (e_mean <= BAR * mabs).all(), (what, q, "mean", e_mean, BAR * mabs)
        assert (e_m2 <= BAR * m2).all(), (what, q, "M2", e_m2, BAR * m2)
        assert (np.abs(std - std_ref) <= BAR * std_ref).all(), (what, q, "std")
    if ref["vel"][0]:
        assert np.array_equal(rec[:dim, 6:8], ref["position_range"].astype(np.float64)), (what, "range")
        assert np.array_equal(rec[:dim, 6:8].astype(np.float32).astype(np.float64), rec[:dim, 6:8])       # exact float32 values
    else:
        assert (rec[:dim, 6] == np.inf).all() and (rec[:dim, 7] == -np.inf).all()
    assert (rec[dim:] == 0).all(), (what, "axes past dim")
    return worst


def test_launch_shape_is_the_one_the_cases_assume():
    from gnn_manip_amd._lib import lib
    text = open(os.path.join(ROOT, "include", "gnn_manip_hip.h")).read()
    assert int(re.search(r"#define\s+GM_RECORDING_STATS_MAX_WORKGROUPS\s+(\d+)", text).group(1)) == dc.MAX_WORKGROUPS
    q = lib().gm_recording_stats_workspace_bytes
    rec = dc.RECORD_DOUBLES * 8
    assert q(3, dc.ONE_PASS) == q(3, dc.N_PAST_ONE_PASS) == 256 + dc.MAX_WORKGROUPS * rec         # the grid stops growing at ONE_PASS nodes
    assert q(3, dc.ONE_PASS - dc.THREADS) == 256 + (dc.MAX_WORKGROUPS - 1) * rec


@pytest.mark.parametrize("kind", sorted(dc.KINDS))
def test_moments_match_the_exactly_summed_form(kind, dev):
    worst = 0.0
    for t, n in SWEEP:
        worst = max(worst, _hold(_stats_of_kind(kind, t, n, dev), dc.reference(kind, t, n), dc.KINDS[kind].dim, (kind, t, n)))
    print(f"{kind}: worst fraction of the 1e-12 bar over {len(SWEEP)} sizes: {worst:.3g}")


def test_moments_past_one_pass_of_the_grid(dev):
    """N_PAST_ONE_PASS nodes: the first 77 threads of the grid walk a second node; the drift case, where a lost or doubled node
    cannot hide in the rounding."""
    t, n = 3, dc.N_PAST_ONE_PASS
    worst = _hold(_stats_of_kind("drift", t, n, dev), dc.reference("drift", t, n), 3, ("drift", t, n))
    print(f"drift at N = {n}: worst fraction of the 1e-12 bar: {worst:.3g}")


@pytest.mark.parametrize("kind,t,n", [("drift", 9, 1000), ("block_sand", 4, 257), ("jitter", 3, dc.N_PAST_ONE_PASS)])
def test_same_bits_at_every_call_and_in_a_poisoned_workspace(kind, t, n, dev):
    from gnn_manip_amd._lib import lib
    first = _stats_of_kind(kind, t, n, dev)
    again = _stats_of_kind(kind, t, n, dev)
    ws = torch.full((lib().gm_recording_stats_workspace_bytes(t, n) + 512,), 0xFF, dtype=torch.uint8, device=dev)
    poisoned = _stats_of_kind(kind, t, n, dev, ws)
    assert np.array_equal(first.view(np.uint64), again.view(np.uint64))
    assert np.array_equal(first.view(np.uint64), poisoned.view(np.uint64))
    assert (ws[-512:] == 0xFF).all(), "written past the queried size"


def test_material_filter_is_the_restatement_on_the_selected_rows(dev):
    """The same recording read three ways; the filter looks at frame 0 alone."""
    t, n = 9, 1000
    rec = dc.recording("block_all", t, n).copy()
    rec[1:, :, dc.MAT_COL] = 5.0                       # later frames say something else: not looked at
    rec_t = _t(rec, dev)
    rigid = rec[0, :, dc.MAT_COL] == 1.0
    for mcol, mval, rows in ((-1, 0.0, np.ones(n, bool)), (dc.MAT_COL, 0.0, ~rigid), (dc.MAT_COL, 1.0, rigid)):
        got = _stats(rec_t, 2, 3, mcol, mval, dev)
        assert got[0, 0] == (t - 1) * rows.sum()
        _hold(got, dc.fsum_moments([rec], 2, 3, [rows]), 3, ("filter", mcol, mval))
    empty = _stats(rec_t, 2, 3, dc.MAT_COL, 7.0, dev)           # a value no row carries
    assert (empty[:, [0, 3]] == 0).all() and (empty[:, 1:3] == 0).all() and (empty[:, 6] == np.inf).all()
    from gnn_manip_amd import recording_statistics
    with pytest.raises(ValueError, match="no row counted"):
        recording_statistics(rec_t, material_id=dc.MAT_COL, material=7.0)
    stats, info = recording_statistics(rec_t, material_id=dc.MAT_COL, material=0.0)
    assert info["velocity_count"] == (t - 1) * (~rigid).sum() and np.array_equal(info["records"][0], _stats(rec_t, 2, 3, dc.MAT_COL, 0.0, dev))


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_position_spoils_its_axis_only(bad, dev):
    from gnn_manip_amd import recording_statistics
    t, n = 9, 257
    clean = dc.recording("jitter", t, n)
    want = _stats(_t(clean, dev), 2, 3, -1, 0.0, dev)
    for frame, row, axis in ((0, 0, 0), (4, 130, 1), (8, 256, 2)):
        rec = clean.copy()
        rec[frame, row, 2 + axis] = bad
        got = _stats(_t(rec, dev), 2, 3, -1, 0.0, dev)
        assert np.array_equal(got[:, [0, 3]], want[:, [0, 3]])                                   # the counts stay
        assert not np.isfinite(got[axis, [1, 2, 4, 5, 6, 7]]).any(), (frame, row, axis, got[axis])
        others = [a for a in range(3) if a != axis]
        assert np.array_equal(got[others].view(np.uint64), want[others].view(np.uint64)), (frame, row, axis)
        with pytest.raises(ValueError, match=r"recording 1: non-finite statistics on axis \[%d\]" % axis):
            recording_statistics([_t(clean, dev), _t(rec, dev)])


# ------------------------------------------------------------------------------------------ the Python surface
@pytest.mark.parametrize("kind", ["jitter", "drift", "scales", "dim2", "last_column"])
def test_recording_statistics_over_three_recordings(kind, dev):
    from gnn_manip_amd import recording_statistics
    k = dc.KINDS[kind]
    recs = [dc.recording(kind, t, n) for t, n in dc.MERGE_SIZES]
    ref = dc.fsum_moments(recs, k.cart0, k.dim)
    stats, info = recording_statistics([_t(r, dev) for r in recs], cartesian_idx=list(range(k.cart0, k.cart0 + k.dim)))
    rec = np.zeros((3, 8))
    rec[:k.dim, 0], rec[:k.dim, 1], rec[:k.dim, 2] = info["velocity_count"], info["velocity_mean"], info["velocity_m2"]
    rec[:k.dim, 3], rec[:k.dim, 4], rec[:k.dim, 5] = info["acceleration_count"], info["acceleration_mean"], info["acceleration_m2"]
    rec[:k.dim, 6:8] = info["position_range"]
    worst = _hold(rec, ref, k.dim, (kind, "merged"))
    print(f"{kind}: three recordings merged: worst fraction of the 1e-12 bar: {worst:.3g}")
    for q, key in (("vel", "velocity"), ("acc", "acceleration")):
        assert (np.abs(info[key + "_std"] - ref[q + "_std"]) <= BAR * ref[q + "_std"]).all()
        assert info[key + "_mean"].dtype == np.float64 and info[key + "_std"].dtype == np.float64
        for part in ("_mean", "_std"):
            assert stats[key + part].dtype == torch.float32 and stats[key + part].shape == (k.dim,)
            assert torch.equal(stats[key + part], torch.tensor([float(v) for v in info[key + part]]))
    assert sorted(stats) == ["acceleration_mean", "acceleration_std", "velocity_mean", "velocity_std"]
    one, info_one = recording_statistics(_t(recs[2], dev), cartesian_idx=list(range(k.cart0, k.cart0 + k.dim)))      # one tensor, no list
    assert np.array_equal(info_one["records"][0], info["records"][2])


def test_metadata_round_trip(dev, tmp_path):
    from gnn_manip_amd import read_metadata, recording_statistics, write_metadata
    recs = [_t(dc.recording("jitter", t, n), dev) for t, n in dc.FIXTURE_SIZES]
    path = str(tmp_path / "metadata.json")
    written = write_metadata(path, recs, BOUNDS, [2, 3, 4], [5, 6, 7], 1)
    assert list(json.load(open(path))) == ["cartesian_idx", "control_idx", "material_id", "bounds", "sequence_length", "dim", "data_dim",
                                           "vel_mean", "vel_std", "acc_mean", "acc_std"] == list(written)
    data_dim, time_steps, cart, ctrl, mat, bounds, stats = read_metadata(path)
    assert (data_dim, time_steps, cart, ctrl, mat) == (dc.D, 9, [2, 3, 4], [5, 6, 7], 1)
    assert torch.equal(bounds["lower_bounds"], torch.tensor(BOUNDS["lower_bounds"])) and torch.equal(bounds["upper_bounds"], torch.tensor(BOUNDS["upper_bounds"]))
    want, info = recording_statistics(recs)
    for key in want:
        assert stats[key].dtype == want[key].dtype == torch.float32 and torch.equal(stats[key], want[key]), key
        assert np.array_equal(stats[key].numpy(), info[key].astype(np.float32)), key                # the float32 of the float64 values
    # ... in the file the reference script wrote for these recordings (tests/golden): the same keys in the same order, the same settings
    fix = json.load(open(os.path.join(ROOT, "tests", "golden", "dataset_stats_metadata.json")))["jitter"]
    assert list(fix) == list(written)
    for key in ("cartesian_idx", "control_idx", "material_id", "bounds", "sequence_length", "dim", "data_dim"):
        assert written[key] == fix[key], key
    for key, name in (("vel_mean", "velocity_mean"), ("vel_std", "velocity_std"), ("acc_mean", "acceleration_mean"), ("acc_std", "acceleration_std")):
        assert written[key] == [float(v) for v in info[name]]


def test_from_recordings_computes_its_statistics(dev):
    from gnn_manip_amd import CoffeeDataset, recording_statistics, scene
    sims = [_t(scene.make_scene(n, seed=s, k=9), dev) for n, s in ((200, 3), (300, 4))]
    stats, _ = recording_statistics(sims)
    kw = dict(k=6, conn_r=scene.CONN_R, bounds=BOUNDS, noise=3e-4)
    given = CoffeeDataset.from_recordings(sims, stats=stats, **kw)
    computed = CoffeeDataset.from_recordings(sims, stats=None, **kw)
    assert sorted(computed.stats) == sorted(stats)
    for key in stats:
        assert torch.equal(computed.graph_attr.stats[key].cpu(), given.graph_attr.stats[key].cpu()), key
        assert torch.equal(computed.stats[key].cpu(), stats[key]), key
    a, b = given.batch([0, 2, 4], seed=5), computed.batch([0, 2, 4], seed=5)         # samples of both recordings: a ragged batch
    for name in ("x", "edge_attr", "edge_index", "y"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.x.shape[0] == 200 + 200 + 300 and a.edge_index.shape[1] > 0


# ------------------------------------------------------------------------------------------ the census
def _census(pos_t, n, stride, r, dev, ws=None):
    from gnn_manip_amd._lib import check, current_stream, lib, ptr
    L = lib()
    need = L.gm_neighbour_census_workspace_bytes(n)
    assert need > 0
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.full((n + 8,), -3, dtype=torch.int32, device=dev)
    check(L.gm_neighbour_census(ptr(pos_t), stride, n, float(r), ptr(counts), ptr(ws), need, current_stream(dev)))
    counts = counts.cpu().numpy()
    assert (counts[n:] == -3).all(), "written past counts[n]"
    return counts[:n].astype(np.int64)


def _out_degree(pos_t, r, cap):
    from gnn_manip_amd import get_connectivity
    s, _ = get_connectivity(pos_t, r, cap)
    return np.bincount(s.cpu().numpy(), minlength=pos_t.shape[0])


def _against_the_build(pos, r, dev, what):
    pos_t = _t(np.ascontiguousarray(pos, np.float32), dev)
    n = pos_t.shape[0]
    counts = _census(pos_t, n, 3, r, dev)
    assert counts.min() >= 1, what                                  # a node lies within its own radius, as in the build
    for cap in (1, 20, 160):
        assert np.array_equal(np.minimum(counts, cap), _out_degree(pos_t, r, cap)), (what, cap)
    if counts.max() <= 160:
        assert np.array_equal(counts, _out_degree(pos_t, r, 160)), what
    return counts


SINGLE_GRAPH_GEOMETRY = ["a1_lattice12", "a2_exactly_r", "a2_just_below_r", "a3_cluster150", "a3_cluster60", "a4_one_point", "a4_line",
                         "a4_plane", "a5_lattice12_at_minus3", "a5_lattice12_at_1000", "a5_cloud_at_1000", "a6_gap_1e6", "a6_gap_1e30",
                         "a6_outlier", "a7_straddle_cap96", "a7_over160_cap160"]


@pytest.mark.parametrize("name", SINGLE_GRAPH_GEOMETRY)
def test_census_is_the_builds_out_degree_on_ties_and_degenerate_geometry(name, dev):
    c = gc.geometry(name)
    c.check()
    assert not c.n_per
    counts = _against_the_build(c.pos, c.r, dev, name)
    assert counts.max() == c.props["max_in_radius"] and counts.min() == c.props["min_in_radius"]
    assert int((counts > c.cap).sum()) == c.props["cap_binds"]


@pytest.mark.parametrize("n", [1, 17, 256, 257, 1000])
def test_census_is_the_builds_out_degree_on_scenes(n, dev):
    from gnn_manip_amd import scene
    counts = _against_the_build(scene.make_scene(n, seed=n)[-1, :, 2:5], scene.CONN_R, dev, n)
    assert counts.max() <= 160


def test_census_past_the_cap_is_the_brute_force(dev):
    p = dc.clump()
    assert dc.clump_margin(p) > dc.CLUMP_MARGIN
    want = dc.brute_counts(p, dc.CLUMP_R)
    assert want.max() > 160
    rec_t = _t(dc.clump_recording(), dev)                           # positions in columns 2..4 of rows of 8 floats
    n = p.shape[0]
    from gnn_manip_amd._lib import lib
    frame0 = rec_t[0].contiguous()
    assert np.array_equal(_census_strided(frame0, n, dc.CLUMP_R, dev), want)
    ws = torch.full((lib().gm_neighbour_census_workspace_bytes(n),), 0xFF, dtype=torch.uint8, device=dev)
    assert np.array_equal(_census_strided(frame0, n, dc.CLUMP_R, dev, ws), want)          # the workspace is written before it is read
    assert np.array_equal(_census(frame0[:, 2:5].contiguous(), n, 3, dc.CLUMP_R, dev), want)     # the same rows packed: stride 3


def _census_strided(frame_t, n, r, dev, ws=None):
    """The census over columns 2..4 of a [n, D] frame: the pointer at column 2, the stride D."""
    from gnn_manip_amd._lib import check, current_stream, lib
    L = lib()
    need = L.gm_neighbour_census_workspace_bytes(n)
    if ws is None:
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    counts = torch.full((n,), -3, dtype=torch.int32, device=dev)
    check(L.gm_neighbour_census(C.c_void_p(frame_t.data_ptr() + 8), dc.D, n, float(r), C.c_void_p(counts.data_ptr()), C.c_void_p(ws.data_ptr()),
                                need, current_stream(dev)))
    return counts.cpu().numpy().astype(np.int64)


def test_neighbour_census_summary(dev):
    from gnn_manip_amd import neighbour_census
    rec = dc.clump_recording()
    rec_t = _t(rec, dev)
    t_all, n = rec.shape[0], rec.shape[1]
    counts = np.stack([_census_strided(rec_t[t].contiguous(), n, dc.CLUMP_R, dev) for t in range(t_all)])
    assert np.array_equal(counts[0], dc.brute_counts(dc.clump(), dc.CLUMP_R))

    def hold(summary, c, cap):
        assert summary["max_count"] == c.max() and summary["rows"] == c.size and summary["frames"] == c.shape[0]
        assert summary["mean_count"] == pytest.approx(c.mean(), rel=1e-15)
        assert summary["rows_over_cap"] == (c > cap).sum() and summary["frames_over_cap"] == (c > cap).any(axis=1).sum()
        assert summary["fraction_over_cap"] == (c > cap).sum() / c.size
        assert np.array_equal(summary["histogram"], np.bincount(c.ravel())) and summary["histogram"].sum() == c.size
        assert len(summary["histogram"]) - 1 == c.max()             # the smallest cap that truncates nothing

    s20 = neighbour_census(rec_t, dc.CLUMP_R, 20)
    hold(s20, counts, 20)
    assert s20["rows_over_cap"] > 0 and s20["frames_over_cap"] >= 1
    s255 = neighbour_census([rec_t], dc.CLUMP_R, 255)
    hold(s255, counts, 255)
    assert s255["rows_over_cap"] == 0 and s255["frames_over_cap"] == 0 and s255["fraction_over_cap"] == 0.0
    hold(neighbour_census(rec_t, dc.CLUMP_R, 20, frames=range(1, t_all, 2)), counts[1::2], 20)
    hold(neighbour_census(rec_t, dc.CLUMP_R, 20, frames=[t_all - 1]), counts[-1:], 20)
    # two recordings of different sizes: the summary is over both
    small = _t(np.ascontiguousarray(rec[:2, :300]), dev)
    c_small = np.stack([_census_strided(small[t].contiguous(), 300, dc.CLUMP_R, dev) for t in range(2)])
    both = neighbour_census([rec_t, small], dc.CLUMP_R, 20)
    flat = np.concatenate((counts.ravel(), c_small.ravel()))
    assert both["rows"] == flat.size and both["max_count"] == flat.max() and np.array_equal(both["histogram"], np.bincount(flat))
    assert both["rows_over_cap"] == (flat > 20).sum() and both["frames_over_cap"] == (counts > 20).any(axis=1).sum() + (c_small > 20).any(axis=1).sum()
    with pytest.raises(IndexError):
        neighbour_census(rec_t, dc.CLUMP_R, 20, frames=[t_all])
