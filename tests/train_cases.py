"""Graphs of the training tests -- a plain helper module shared by tests/test_gpu_train.py, tests/test_gpu_train_regimes.py and the
gradient tests built on them: radius graphs of seeded scenes, the benchmark's collated batch, and the hub multigraph."""
import functools

import numpy as np

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc

KW = dict(stats=STATS, bounds=BOUNDS, conn_r=0.015, cartesian_idx=CART, material_idx=MAT)


def graph(n, side, seed):
    """(nodes, edge_attr, edge_index [2, E]) of the radius graph of make_scene(n, seed, side)."""
    from gnn_manip_amd import scene
    obs = scene.make_scene(n, seed=seed, side=side)
    nodes, ea, s, r, _ = orc.process(obs, None, control_idx=CTRL, **KW)
    return nodes, ea, np.stack((s, r))


@functools.lru_cache(maxsize=1)
def benchmark_graph():
    """bench.py extra_train's batch: two make_scene(5000, side=0.152 * 0.8) scenes, seeds 100 / 101, collated."""
    from gnn_manip_amd import scene
    batch = [(scene.make_scene(5000, seed=100 + b, side=0.152 * 0.8), None) for b in range(2)]
    nodes, ea, ei, _ = orc.process_collate(batch, control_idx=CTRL, **KW)
    return nodes, ea, ei


HUB_N, HUB_E = 400, 9000
HUB_DST, HUB_DST2, HUB_SRC2 = 17, 201, 333     # node 17 is a hub destination AND a hub source
SEND_ONLY, RECV_ONLY, ISOLATED = (390, 391, 392), (393, 394, 395), (396, 397, 398, 399)


def hub_graph(seed=73):
    """edge_index [2, HUB_E] of a random multigraph over the nodes 0 .. 389 (in the style of
    test_scatter_add_is_deterministic_with_hub_nodes) with, all at once: destinations of in-degree >= 700 and >= 300, sources of
    out-degree >= 700 (the first hub destination) and >= 300, a block of exact duplicates, a block of self loops, nodes that only
    send, only receive, or are in no edge -- and the columns in random order.  Every one of these properties is asserted on the
    graph that was built."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ei = rng.integers(0, 390, size=(2, HUB_E)).astype(np.int64)
    ei[1, :700] = HUB_DST
    ei[1, 700:1000] = HUB_DST2
    ei[0, 1000:1700] = HUB_DST
    ei[0, 1700:2000] = HUB_SRC2
    ei[:, 2000:2064] = ei[:, 2100:2164]                 # 64 edges twice
    ei[:, 2064:2072] = ei[:, 2100:2101]                 # ... and one of them ten times in all
    ei[0, 2200:2300] = ei[1, 2200:2300]                 # self loops
    ei[0, 2300:2320] = np.resize(SEND_ONLY, 20)
    ei[1, 2320:2340] = np.resize(RECV_ONLY, 20)
    order = rng.permutation(HUB_E)
    ei = np.ascontiguousarray(ei[:, order])
    # the properties the cases are there for, on the graph that was built
    indeg, outdeg = np.bincount(ei[1], minlength=HUB_N), np.bincount(ei[0], minlength=HUB_N)
    assert indeg[HUB_DST] >= 700 and indeg[HUB_DST2] >= 300 and outdeg[HUB_DST] >= 700 and outdeg[HUB_SRC2] >= 300, "hub degrees"
    rest = np.ones(HUB_N, bool)
    rest[[HUB_DST, HUB_DST2, HUB_SRC2]] = False
    assert indeg[rest].max() < 100 and outdeg[rest].max() < 100, "a node that is not a hub has a hub's degree"
    assert indeg[HUB_DST] != outdeg[HUB_DST] and indeg[HUB_SRC2] < 100 and outdeg[HUB_DST2] < 100, "hub roles"
    assert all(indeg[v] == 0 and outdeg[v] > 0 for v in SEND_ONLY), "send-only nodes"
    assert all(outdeg[v] == 0 and indeg[v] > 0 for v in RECV_ONLY), "receive-only nodes"
    assert all(indeg[v] == 0 and outdeg[v] == 0 for v in ISOLATED), "isolated nodes"
    _, counts = np.unique(ei.T, axis=0, return_counts=True)
    assert (counts >= 2).sum() >= 64 and counts.max() >= 10, "duplicate edges"
    assert (ei[0] == ei[1]).sum() >= 100, "self loops"
    dst_sorted = np.argsort(ei[1], kind="stable")
    assert not np.array_equal(dst_sorted, np.arange(HUB_E)), "the destination sort has nothing to undo"
    return ei
