"""CPU: the cases of f16_rollout_cases.py are in the regimes they were built for, and their references tell right from wrong -- the
restatement (precision_cases) standing in for the device.

What the envelopes can and cannot see (figures printed by the tests below; hidden 128):
  * Rule B (err / 4 .. 4 err of a whole forward) catches a wrong OPERAND: every edge given its neighbour's attributes puts the
    prediction 3e-2 (part 1's scene) and 0.11 .. 0.15 (part 2's steps) of its maximum away, 19 and 100 times the restatement's error.
  * It cannot see a single MLP left unrounded.  The variant that rounds everything but encoder.phi_edge has 0.77 .. 1.02 of the
    restatement's error on the graphs of part 1 and 0.86 .. 0.98 on the steps of part 2: the edge encoder is one of nine MLPs whose
    rounding noise adds up, and a factor 4 does not resolve a ninth.  No whole-forward case can: device and restatement are two
    draws of one noise, and the bar has to leave room for that.  The smallest case that tells is one MLP deep -- the encoder block of
    part 5 on the scene ("encoder_e", check A's bar): the variant is 3.4e-4 away from the restatement, 3 g is 2.2e-5.  The systolic
    edge encoder has no entry point that returns its output, so on the sorted route an unrounded operand of it is NOT caught; a
    wrong one is.
  * Raw rows.  The rounding at the kernels' scales and the rounding of the unscaled values differ where a value is below 2^-14 at
    one of the two scales.  Two cases tell them apart at check A's bar: the scene times 1e-4 (rows below 2^-14: the unscaled
    restatement is 3e-4 away, 13 times the bar) and times 1e3 (first-Linear weights below 2^-14: 1e-4 .. 2e-4 away).  The wide rows
    do NOT: their small entries are rounded differently (971 of 1600), but what an entry 2^-16 .. 2^-26 below the maximum carries is
    that far below what the maximum carries, and the two restatements end 1e-8 apart.  Weights large enough to make such entries
    count put the weights of the maximum's column below 2^-14 at the weights' common scale, where fp16 has lost them either way.
    The wide rows are a domain case on the device (finite, inside the bar against both restatements)."""
import numpy as np
import pytest

import f16_rollout_cases as fc
import layernorm_cases as lc
import precision_cases as pc
from oracle import epd_oracle as orc


# ================================================================== part 1: sorted attributes
@pytest.mark.parametrize("name", fc.SORTED_GRAPHS)
def test_sorted_graphs_are_in_destination_order_and_the_same_graphs(name):
    p, dims, nodes, ea, ei = fc.sorted_graph(name)
    assert dims == pc.SYS_DIMS and dims[3:5] == (128, fc.NL)
    assert (np.diff(ei[1]) >= 0).all()
    un_nodes, un_ea, un_ei = lc.scene() if name == "scene" else pc.sys_case(name)
    assert np.array_equal(nodes, un_nodes)
    key = lambda e_i, e_a: sorted(zip(e_i[0].tolist(), e_i[1].tolist(), map(tuple, e_a.tolist())))
    assert key(ei, ea) == key(un_ei, un_ea)
    if name != "scene":
        assert not (np.diff(un_ei[1]) >= 0).all() or ei.shape[1] == 1   # generated unsorted: the sort is needed
        # stable: the edges of a destination keep the order they came in, which is the order the library's sort gives them
        for d in np.unique(ei[1])[:50]:
            assert np.array_equal(ea[ei[1] == d], un_ea[un_ei[1] == d])
    sizes = {"e1": 1, "e33": 33, "e129": 129, "e513": 513}
    if name in sizes:
        assert ei.shape[1] == sizes[name]       # just past 0, 1, 4 and 16 blocks of 32 edges
    if name == "hub":
        assert int(np.bincount(ei[1]).max()) >= 200 > 128   # the hub's segment crosses the 128-edge group


def _shifted(ea):
    return np.ascontiguousarray(np.roll(ea, 1, axis=0))


def test_the_envelope_of_part_1_catches_a_wrong_operand_and_not_one_unrounded_mlp():
    print()
    for name in fc.SORTED_GRAPHS:
        ref, err_r = fc.sorted_reference(name)
        _, err_v = fc.sorted_reference(name, variant=True)
        print(f"[f16 rollout cases] sorted {name}: err(restatement) {err_r:.2e}, err(edge encoder unrounded) {err_v:.2e}, ratio {err_v / err_r:.2f}")
        assert 4e-5 < err_r / 4 and err_r < 2e-2          # at the mode's precision: a library that ignores the switch is outside
    p, dims, nodes, ea, ei = fc.sorted_graph("scene")
    ref, err_r = fc.sorted_reference("scene")
    err_w = pc.max_err(pc.epd_forward(p, nodes, _shifted(ea), ei, dims[4], dims[5]), ref, pc.B_FLOOR)
    print(f"[f16 rollout cases] sorted scene: every edge with its neighbour's attributes: err {err_w:.2e}, {err_w / err_r:.0f} times the restatement's")
    assert err_w > 4 * 4 * err_r


# ================================================================== part 2: the scenes and every step
@pytest.mark.parametrize("name", list(fc.SCENES))
def test_rollout_scenes_are_in_their_regime(name):
    obs, traj = fc.rollout_scene(name)
    n = obs.shape[1]
    assert abs(n - {"n300": 300, "n700": 700}[name]) == 0 and traj.shape == (fc.HORIZON, n // 10, 3)
    rigid = ~fc.sand_rows(obs)
    assert rigid.sum() == n // 10 >= 1 and rigid[-(n // 10):].all()
    (_, frames64), _ = fc.compound_reference(name)
    for s, (pos, ei) in enumerate(frames64):
        e = ei.shape[1]
        print(f"[f16 rollout cases] {name} frame {s}: {e} edges, {e / n - 1:.1f} neighbours per node")
        assert 3000 <= e <= 10000 and 10 <= e / n - 1 <= 14
        assert orc.connectivity_is_tie_free(pos, fc.R, fc.K_NB), (name, s)


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_the_envelope_of_part_2_catches_a_wrong_operand_and_not_one_unrounded_mlp(name):
    obs, traj = fc.rollout_scene(name)
    p = fc.params(128)
    ref, err_r, edges, seen = fc.step_reference(p, obs, traj[0])
    _, err_v, _, _ = fc.step_reference(p, obs, traj[0], **fc.EDGE_ENCODER_UNROUNDED)
    err_w = pc.max_err(pc.epd_forward(p, seen["nodes"], _shifted(seen["ea"]), seen["ei"], fc.NL, fc.MS), ref, pc.B_FLOOR)
    print(f"\n[f16 rollout cases] step {name}: {edges} edges, max |ref| {np.abs(ref).max():.2f}, err(restatement) {err_r:.2e}, "
          f"err(edge encoder unrounded) {err_v:.2e} (ratio {err_v / err_r:.2f}), err(neighbour's attributes) {err_w:.2e}")
    assert 4e-5 < err_r / 4 and err_r < 2e-2
    assert float(np.abs(ref).max()) > 0.1                  # the decoder is not damped: a prediction of order 1
    assert err_w > 4 * 4 * err_r
    # the step's features are the oracle's own: the reference is the float64 forward of what `process` gives for this window
    nodes, ea, s, r, _ = orc.process(np.array(obs), None, fc.STATS, fc.BOUNDS, fc.R, fc.CART, fc.MAT, fc.CTRL, fc.K_NB)
    assert np.array_equal(seen["ei"], np.stack((s, r))) and np.array_equal(seen["ea"], ea)


def test_one_mlp_deep_is_where_an_unrounded_edge_encoder_shows():
    for hidden in fc.RAW_HIDDEN:
        p, nodes, ea, _ = fc.raw_case(hidden, "scene")
        r64, g = fc.raw_reference(hidden, "scene")
        _, e_v = pc.graph_independent(p, "encoder", nodes, ea, fc.NL, **fc.EDGE_ENCODER_UNROUNDED)
        d = pc.rel_rms(e_v, r64["encoder_e"])
        print(f"[f16 rollout cases] hidden {hidden}: edge encoder unrounded {d:.2e} from the restatement, 3 g = {3 * g['encoder_e']:.2e}")
        assert 3 * g["encoder_e"] <= 0.5 * d


# ================================================================== part 3: compounding
@pytest.mark.parametrize("name", list(fc.SCENES))
def test_no_edge_is_about_to_change_and_the_references_keep_one_edge_set(name):
    """In every frame a graph is built on (float64 rollout): no pair within 1e-5 R of R, and neither a pair's distance to R nor the
    gap between a node's 20th and 21st neighbour -- where the cap of 20 binds -- is within fc.MARGIN times the restatement's own
    largest deviation in that frame: a rollout with the restatement's noise meets the float64 rollout's edges.  The restatement's
    rollout does."""
    obs, _ = fc.rollout_scene(name)
    (end64, frames64), (end_r, frames_r) = fc.compound_reference(name)
    for s, ((pos64, ei64), (pos_r, ei_r)) in enumerate(zip(frames64, frames_r)):
        (radius, rank), dev = fc.graph_margins(pos64), float(np.abs(pos_r.astype(np.float64) - pos64).max())
        print(f"[f16 rollout cases] {name} frame {s}: nearest pair to the radius {radius:.2e} = {radius / fc.R:.2e} R, smallest gap at the "
              f"neighbour cap {rank:.2e}, restatement's deviation {dev:.2e}")
        assert radius > 1e-5 * fc.R
        assert min(radius, rank) > fc.MARGIN * dev
        assert fc.edge_set(ei64) == fc.edge_set(ei_r), (name, s)
    d_r = fc.end_deviation(end_r, end64, obs)
    print(f"[f16 rollout cases] {name}: d(restatement) {d_r:.2e}")
    assert 1e-5 < d_r < 1e-2
    assert fc.end_deviation(end64, end64, obs) == 0


# ================================================================== part 4: the ranking
def test_the_ranking_is_decided_by_the_references_alone():
    l64, nu, decided = fc.rank_reference()
    obs, trajs, desired = fc.rank_case()
    assert trajs.shape[:2] == (fc.RANK_B, fc.RANK_H) and 9 < fc.RANK_STEP_SIZES[-1] / fc.RANK_STEP_SIZES[0] < 11
    print("\n".join(fc.rank_table("float64 rollouts", l64)[0]))
    print(f"[f16 rollout cases] losses {l64}, nu {nu}, {len(decided)} of 15 pairs decided")
    assert (l64 > 1e-6).all() and (l64 < 1e-4).all()
    assert len(decided) >= 12
    best = int(np.argmin(l64))
    assert all((min(best, c), max(best, c)) in decided for c in range(fc.RANK_B) if c != best)
    assert fc.rank_table("float64 rollouts", l64)[1] == []
    flipped = l64.copy()
    i, j = decided[0]
    flipped[[i, j]] = flipped[[j, i]]
    assert fc.rank_table("two losses exchanged", flipped)[1]            # the table sees an exchanged pair


# ================================================================== part 5: raw rows at the kernels' scale
def _both_normal(x, cap=np.inf):
    x = np.abs(np.asarray(x, np.float64))
    return (x >= 2.0 ** -14) & (x * fc.row_scale(x, cap) >= 2.0 ** -14) | (x == 0)


def test_the_two_roundings_differ_where_claimed_and_only_there():
    arrays = {"standard normal": pc.a_inputs(128, 2)[0]}
    for name in fc.RAW_CASES:
        _, nodes, ea, _ = fc.raw_case(128, name)
        arrays[f"{name} nodes"], arrays[f"{name} edges"] = nodes, ea
    for what, x in arrays.items():
        a, b, ok = fc.round_rows(x), pc.r16(x), _both_normal(x)
        print(f"[f16 rollout cases] {what}: {int((a != b).sum())} of {x.size} entries rounded differently, {int((~ok).sum())} subnormal at one of the scales")
        assert np.array_equal(a[ok], b[ok]), what
        assert (a != b).sum() <= (~ok).sum()
    _, nodes, ea, _ = fc.raw_case(128, "wide")
    for x in (nodes, ea):
        a, b = fc.round_rows(x), pc.r16(x)
        rows = fc.raw_rows_by_depth(8)
        assert np.array_equal(a[rows], b[rows])                            # 2^-10 of the maximum at the least: normal at both scales
        for depth in (16, 22, 26):
            rows = fc.raw_rows_by_depth(depth)
            assert (a[rows, 1:] != b[rows, 1:]).mean() > 0.5
            # a maximum of 1 .. 2: these entries are below 2^-14 as they stand, and r16 is the coarser rounding
            assert np.abs(b[rows, 1:] - x[rows, 1:]).max() > 4 * np.abs(a[rows, 1:] - x[rows, 1:]).max()
        for depth, bits in ((22, 8), (26, 4)):                             # subnormal at the kernels' scale too: 11 - (depth - 19) bits
            rows = fc.raw_rows_by_depth(depth)
            rel = np.abs(a[rows, 1:] - x[rows, 1:]) / np.abs(x[rows, 1:])
            assert 2.0 ** -(bits + 3) < rel.max() <= 2.0 ** -bits, (depth, rel.max())
        assert np.array_equal(a[list(fc.WIDE_SINGLE + fc.WIDE_ZERO)], b[list(fc.WIDE_SINGLE + fc.WIDE_ZERO)])
        assert (np.abs(x[list(fc.WIDE_SINGLE)]) > 0).sum(axis=1).tolist() == [1] * 4 and not x[list(fc.WIDE_ZERO)].any()
    _, nodes, ea, _ = fc.raw_case(128, "scene_x1e-4")
    for x in (nodes, ea):
        a, b = fc.round_rows(x), pc.r16(x)
        assert np.abs(x).max() < 2.0 ** -10 and (a != b).mean() > 0.3      # rows of magnitude about 2^-14 and below
        low = np.abs(x) < 2.0 ** -16                                       # there the unscaled rounding is the coarser one
        assert low.mean() > 0.1 and np.abs(b - x)[low].mean() > 4 * np.abs(a - x)[low].mean()


def test_the_cap_decides_no_row_of_any_case():
    for hidden in fc.RAW_HIDDEN:
        for name in fc.RAW_CASES:
            p, nodes, ea, _ = fc.raw_case(hidden, name)
            for prefix, x in (("encoder.phi_node", nodes), ("encoder.phi_edge", ea)):
                cap = fc.row_cap(p, prefix, fc.NL)
                s = fc.row_scale(x)[np.abs(x).max(axis=1) > 0]
                print(f"[f16 rollout cases] hidden {hidden} {name} {prefix}: cap 2^{np.log2(cap):.0f}, largest row scale 2^{np.log2(s.max()):.0f}")
                assert 2 * s.max() <= cap


def test_standard_normal_rows_keep_the_meaning_of_check_a():
    """On precision_cases' own inputs the rounding at the kernels' scale changes nothing check A could see."""
    for hidden, nl in pc.A_CASES:
        p = pc.a_params(hidden, nl)
        nodes, ea = pc.a_inputs(hidden, nl)[:2]
        r64, g = pc.a_reference(hidden, nl)
        how = fc.raw_rounding(p, nl)
        h, e = pc.graph_independent(p, "encoder", nodes, ea, nl, how["enc_node"], how["enc_edge"])
        for name, out in (("encoder_h", h), ("encoder_e", e)):
            d = pc.rel_rms(out, r64[name])
            print(f"[f16 rollout cases] standard normal hidden {hidden} layers {nl} {name}: the two restatements {d:.2e} apart, 3 g = {3 * g[name]:.2e}")
            assert d <= 0.1 * 3 * g[name]


@pytest.mark.parametrize("hidden", fc.RAW_HIDDEN)
def test_which_raw_cases_tell_the_two_roundings_apart(hidden):
    print()
    for name in fc.RAW_CASES:
        r64, g = fc.raw_reference(hidden, name)
        natural = fc.raw_restate(hidden, name, natural=True)
        for out in fc.RAW_OUTPUTS:
            d = pc.rel_rms(natural[out], r64[out])
            print(f"[f16 rollout cases] hidden {hidden} {name} {out}: g {g[out]:.2e}, rows rounded as they stand {d:.2e} away (3 g = {3 * g[out]:.2e})")
            assert g[out] > 0 and np.isfinite(r64[out]).all()
            if name in ("scene_x1e-4", "scene_x1e3"):
                assert d > 2 * 3 * g[out]                   # the unscaled restatement would fail check A's bar
            else:
                assert d <= 0.1 * 3 * g[out]                # see the module docstring: the wide rows do not reach the bar
