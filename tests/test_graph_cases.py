"""The cases of graph_cases.py on the CPU: each one is in the regime it was built for, and the reference side is right on it -- the
oracle's cell-list path equals its brute-force path (a dense float64 distance matrix) on ties, coincident points, degenerate
extents and far-away coordinates, not only on the random data test_oracle_golden.py uses."""
import numpy as np
import pytest

import graph_cases as gc
from oracle import epd_oracle as orc


@pytest.mark.parametrize("name", list(gc.GEOMETRY))
def test_geometry_case_is_in_its_regime(name):
    gc.geometry(name).check()


def _brute(pos, r, cap):
    """orc.get_connectivity's brute-force branch, whatever n is (the function itself switches to the cell list past 4096 rows)."""
    s, rcv = [], []
    for a in range(0, pos.shape[0], 4096):
        d2 = orc._sq_dists_f64(pos[a:a + 4096], pos)
        for row in range(d2.shape[0]):
            idx = np.nonzero(d2[row] <= r * r)[0]
            idx = idx[np.lexsort((idx, d2[row, idx]))][:cap]
            s.append(np.full(idx.shape[0], a + row, np.int64))
            rcv.append(idx.astype(np.int64))
    return np.concatenate(s), np.concatenate(rcv)


@pytest.mark.parametrize("name", [k for k in gc.GEOMETRY if not k.startswith("a7_straddle") or k.endswith(("cap2", "cap96", "cap160"))])
def test_oracle_cell_list_equals_brute_force(name):
    """Per graph of a batch.  Extents of 1e6 and more are left to the brute-force path alone: the oracle's cell list is never
    coarsened (edge r * 1.001), so it has no grid for them, and get_connectivity never takes it below 4097 rows."""
    c = gc.geometry(name)
    if not c.cells_ok:
        assert c.props["n"] <= 4096 and max(c.props["extent"]) >= 9.0e5
        return
    n_per = c.n_per or c.props["n"]
    graphs = range(0, c.props["n"], n_per)
    if c.n_per and c.n_per <= 7:
        graphs = list(graphs)[::50]    # 60 of the 3000 tiny graphs
    for g0 in graphs:
        p = c.pos[g0:g0 + n_per]
        sb, rb = _brute(p, c.r, c.cap)
        sc, rc = orc._get_connectivity_cells(p, c.r, c.cap)
        assert np.array_equal(sb, sc) and np.array_equal(rb, rc), (name, g0)
        if p.shape[0] <= 4096:
            so, ro = orc.get_connectivity(p, c.r, c.cap)
            assert np.array_equal(sb, so) and np.array_equal(rb, ro), (name, g0)


def test_tie_rule_is_the_smaller_index():
    """The contract on the two cases where it is visible by eye: an interior lattice row keeps, of its 8 corner neighbours at
    s * sqrt(3), the one with the smallest index; a row of a coincident cluster keeps the 20 smallest indices of the cluster, which
    leaves its own self edge out unless it is one of them."""
    c = gc.geometry("a1_lattice12")
    s, r = orc.get_connectivity(c.pos, c.r, c.cap)
    d2 = orc._sq_dists_f64(c.pos, c.pos)
    corner = 3 * gc.S7 * gc.S7
    interior = np.flatnonzero((d2 <= c.r * c.r).sum(axis=1) == 27)
    assert interior.shape[0] == 1000
    for q in interior[:50]:
        kept = r[s == q]
        assert kept.shape[0] == 20 and kept[0] == q
        assert kept[-1] == np.flatnonzero(d2[q] == corner).min() and (d2[q, kept[:-1]] < corner).all()
    c = gc.geometry("a3_cluster150")
    s, r = orc.get_connectivity(c.pos, c.r, c.cap)
    cluster = np.arange(400, 550)
    same = np.flatnonzero((c.pos == c.pos[400]).all(axis=1))     # the cluster and the row it was put on
    for q in cluster[::10]:
        assert np.array_equal(r[s == q], same[:20])
    assert sum(q in r[s == q] for q in cluster) == int(np.isin(cluster, same[:20]).sum()) < 20


@pytest.mark.parametrize("name", list(gc.SCENES))
def test_scene_case_is_in_its_regime(name):
    sc = gc.scene_case(name)
    sc.geo.check()
    obs = sc.obs
    assert obs.dtype == np.float32 and obs.shape[0] == 6 and obs.shape[2] == 8
    assert np.array_equal(obs[-1, :, 2:5], sc.geo.pos)
    rows = list(sc.cluster_rows)
    if rows:
        assert (obs[:, rows, 2:5] == obs[-1, rows[0], 2:5]).all()        # coincident in every frame
    assert 0.1 < obs[:, :, 2:5].min() and obs[:, :, 2:5].max() < 0.9    # inside the scenes' bounds
    assert (obs[-1, :, 1] == 1).sum() == round(obs.shape[1] * 0.1)


@pytest.mark.parametrize("name", list(gc.DEGREES))
def test_degree_case_is_in_its_regime(name):
    gc.degree_case(name).check()


def test_hub_cases_sit_where_the_block_tables_change_value():
    """The two 384-row hubs against the restated tables: starting ON a group boundary the hub's first group has no head (the two that
    follow are its run); starting one row behind a boundary all three groups that follow are head partials of one run, the two in the
    middle entirely the hub's."""
    for name, heads in (("c_hub384_at_group_plus_0", [-1, "h", "h", -1]), ("c_hub384_at_group_plus_1", [-1, "h", "h", "h"])):
        c = gc.degree_case(name)
        hub, start = c.props["hubs"][0], c.props["hub_start"][0]
        t = gc.block_tables(np.sort(c.edge_index[1], kind="stable"), c.n)
        g0 = start // gc.GROUP
        assert [int(x) for x in t["head"][g0:g0 + 4]] == [hub if h == "h" else (int(t["head"][g0]) if i == 0 else -1) for i, h in enumerate(heads)]
        assert t["head"][g0] != hub and t["stitch"][hub] == g0 + 1
        assert (t["stitch"] >= 0).sum() == np.unique(t["head"][t["head"] >= 0]).shape[0]
    t = gc.block_tables(np.zeros(0, np.int64), 70)
    assert t["n_blocks"] == 0
    t = gc.block_tables(np.asarray([41]), 70)
    assert t["n_blocks"] == 4 and t["blk"][0].tolist() == [0, 1 | (1 << 8)] and t["seg"][0].tolist() == [0, 1] and t["blk"][3].tolist() == [1, 2 << 8]
