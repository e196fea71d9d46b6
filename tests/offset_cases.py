"""Block-diagonal graphs of small copies, large enough that the kernels' buffer offsets cross 2 GiB and 4 GiB -- a plain helper
module shared by test_offset_cases.py (CPU) and test_gpu_offsets.py (GPU).

K = 5 "class" graphs of N0 = 1021 nodes each are built on the host (seeded numpy scenes through the oracle's process).  A tiling
of T copies holds, as copy t, the data of class t mod K: node rows back to back, edge indices offset by t * N0, edges concatenated
copy by copy.  Only the K classes ever exist on the host; the tiling is made on the device with torch operations, and every
reference (float64 oracle forward, float64 / float32 torch gradients) is computed once per class and assembled.

Wrap safety: an address that wraps at a power of two lands a power-of-two number of bytes away, i.e. a power-of-two number of rows
(the row strides are powers of two).  The content repeats with the node period K * N0 and the edge period sum(e0): both must be odd,
so that no power-of-two shift maps a row onto a row with the same content (`Family.check`).

Every case carries the regime it exists for -- the bytes of the arrays it names and the side of 2^31 / 2^32 each lies on, the
library's route switch (edge_sys_fits of csrc/hedge.hip restated) and the weight-gradient kernel's 4 GiB guard (csrc/train.hip
restated) -- computed from the shapes actually built and asserted (`OffsetCase.check`) before the GPU is touched."""
import functools
from dataclasses import dataclass, field

import numpy as np

K = 5
N0 = 1021          # prime
DENSE_SIDE = 0.05  # ~20 edges per node: the cap of 20 neighbours binds almost everywhere
SPARSE_SIDE = 0.25  # a dilute scene: mean in-degree 1.4 after thinning (sparse_family)
GIB2, GIB4 = 1 << 31, 1 << 32

# restated from csrc/hedge.hip (the systolic edge kernel: hidden 128 only)
SYS_H = 128
BE = 32            # edges of one block
SINK_ROWS = 1024   # kSinkRows (csrc/hedge.h): rows behind the side buffer for the masked-off lanes of the row stores


def padded_hidden(hidden):
    return 64 if hidden <= 64 else 128 if hidden <= 128 else 256


def edge_groups_max(n, cap):
    """Rows of the side buffer (csrc/hedge.hip: max_blocks_of / edge_groups_max)."""
    max_blocks = -(-cap // BE) + 4 * n + 4
    return max_blocks // 4 + 1 + SINK_ROWS


def edge_sys_fits(n, cap):
    """csrc/hedge.hip edge_sys_fits restated: the systolic edge kernel's P gathers and agg / side-buffer stores use 32-bit byte
    offsets, so the P table (n rows of 2H floats) and agg + side buffer (n + groups rows of H floats) must each stay below 4 GiB."""
    return n * 2 * SYS_H * 4 < GIB4 and (n + edge_groups_max(n, cap)) * SYS_H * 4 < GIB4


def wgrad_guard_ok(rows, ld):
    """csrc/train.hip launch_wgrad restated: an indexed operand of `rows` rows of `ld` floats is addressed with unsigned byte
    offsets and must stay below 4 GiB (GM_ERR_UNSUPPORTED otherwise)."""
    return rows * ld * 4 < GIB4


def side_of(nbytes):
    """Which of the three ranges a byte count lies in."""
    return "<2GiB" if nbytes < GIB2 else ("[2,4)GiB" if nbytes < GIB4 else ">=4GiB")


# ------------------------------------------------------------------------------------------ the class graphs
@dataclass
class Family:
    name: str
    nodes: list        # K x float32 [N0, 25]
    edge_attr: list    # K x float32 [e0_c, 4]
    edge_index: list   # K x int64 [2, e0_c]  (senders, receivers), local node numbers
    n0: int = N0

    @property
    def e0(self):
        return [int(ei.shape[1]) for ei in self.edge_index]

    @property
    def node_period(self):
        return len(self.nodes) * self.n0

    @property
    def edge_period(self):
        return sum(self.e0)

    def check(self):
        """Wrap safety, and the classes are what a tiling needs: equal node counts, local indices, pairwise different content."""
        k = len(self.nodes)
        assert k >= 2 and all(x.shape[0] == self.n0 for x in self.nodes), self.name
        assert self.node_period % 2 == 1, (self.name, "node period must be odd", self.node_period)
        assert self.edge_period % 2 == 1, (self.name, "edge period must be odd", self.edge_period)
        for c in range(k):
            ei = self.edge_index[c]
            assert ei.dtype == np.int64 and ei.shape[0] == 2 and self.edge_attr[c].shape == (ei.shape[1], 4), (self.name, c)
            assert ei.size == 0 or (ei.min() >= 0 and ei.max() < self.n0), (self.name, c)
            for d in range(c):
                assert not np.array_equal(self.nodes[c], self.nodes[d]), (self.name, "classes", c, d, "hold the same rows")
        return self

    def degrees(self):
        """Over all classes: (mean in-degree, isolated nodes, nodes that only send)."""
        indeg = np.concatenate([np.bincount(ei[1], minlength=self.n0) for ei in self.edge_index])
        outdeg = np.concatenate([np.bincount(ei[0], minlength=self.n0) for ei in self.edge_index])
        return float(indeg.mean()), int(((indeg == 0) & (outdeg == 0)).sum()), int(((indeg == 0) & (outdeg > 0)).sum())

    def sizes(self, t):
        """(nodes, edges) of a tiling of t copies."""
        e0 = self.e0
        k = len(e0)
        return t * self.n0, (t // k) * sum(e0) + sum(e0[:t % k])

    def copies_for_edges(self, e_min):
        """The smallest number of copies whose tiling has at least e_min edges."""
        k = len(self.e0)
        t = max(0, e_min // self.edge_period - 1) * k
        while self.sizes(t)[1] < e_min:
            t += 1
        return t


def _make_family(name, side, n0, seeds, keep=None):
    from gnn_manip_amd import scene
    from oracle import epd_oracle as orc
    nodes, eas, eis = [], [], []
    for c, seed in enumerate(seeds):
        obs = scene.make_scene(n0, seed=seed, side=side)
        x, ea, s, r, _ = orc.process(obs, None, scene.STATS, scene.BOUNDS, scene.CONN_R, scene.CART, scene.MAT, scene.CTRL)
        ei = np.stack((s, r)).astype(np.int64)
        if keep is not None:
            m = keep(c, ei)
            ea, ei = ea[m], ei[:, m]
        nodes.append(np.ascontiguousarray(x, np.float32))
        eas.append(np.ascontiguousarray(ea, np.float32))
        eis.append(np.ascontiguousarray(ei))
    if sum(e.shape[1] for e in eis) % 2 == 0:   # an even edge period: drop the last edge of class 0
        eas[0], eis[0] = np.ascontiguousarray(eas[0][:-1]), np.ascontiguousarray(eis[0][:, :-1])
    return Family(name, nodes, eas, eis, n0)


@functools.lru_cache(maxsize=None)
def dense_family():
    """The five radius graphs of 1021-particle scenes (seeds 900 .. 904, side 0.05): about 20.4k edges each."""
    return _make_family("dense", DENSE_SIDE, N0, [900 + c for c in range(K)]).check()


def _sparse_keep(c, ei):
    """The radius graph of a dilute scene is mostly self edges, and it is symmetric.  Drop the self edge of one node in three and
    every incoming edge of one node in ten (both seeded): a node without a neighbour that lost its self edge is isolated, a node
    with a neighbour that lost its incoming edges only sends."""
    rng = np.random.Generator(np.random.PCG64(7000 + c))
    n = int(ei.max()) + 1
    drop_self = rng.random(n) < 1.0 / 3.0
    deaf = rng.random(n) < 0.1                 # nodes whose incoming edges are all dropped: they only send (if they have a neighbour)
    s, r = ei
    return ~(((s == r) & drop_self[r]) | deaf[r])


@functools.lru_cache(maxsize=None)
def sparse_family():
    """E about n: the same 1021 particles in a box of side 0.25 (mean in-degree between 1 and 2), thinned so that
    it has isolated nodes and nodes that only send."""
    f = _make_family("sparse", SPARSE_SIDE, N0, [900 + c for c in range(K)], keep=_sparse_keep).check()
    mean_in, isolated, send_only = f.degrees()
    assert 0.8 <= mean_in <= 2.0 and isolated > 0 and send_only > 0, (mean_in, isolated, send_only)
    return f


# ------------------------------------------------------------------------------------------ tiling
def tile_host(fam, t):
    """The tiled graph as numpy arrays (tiny T only: the CPU tests)."""
    k = len(fam.nodes)
    nodes = np.concatenate([fam.nodes[i % k] for i in range(t)])
    ea = np.concatenate([fam.edge_attr[i % k] for i in range(t)])
    ei = np.concatenate([fam.edge_index[i % k] + i * fam.n0 for i in range(t)], axis=1)
    return nodes, ea, ei


def tile_rows(rows, t, torch):
    """Rows of the K classes (list of [r_c, w] tensors on one device) laid out copy by copy for t copies."""
    k = len(rows)
    period = torch.cat(rows)
    full, rem = divmod(t, k)
    parts = [period.repeat(full, *([1] * (period.dim() - 1)))] if full else []
    if rem:
        parts.append(torch.cat(rows[:rem]))
    return torch.cat(parts) if len(parts) != 1 else parts[0]


def tile_device(fam, t, dev):
    """(nodes [t * n0, 25], edge_attr [E, 4], edge_index [2, E] int64) on `dev`, made there from the K classes."""
    import torch
    k = len(fam.nodes)
    nodes = tile_rows([torch.from_numpy(x).to(dev) for x in fam.nodes], t, torch)
    ea = tile_rows([torch.from_numpy(x).to(dev) for x in fam.edge_attr], t, torch)
    # edge indices: class c of period q sits at node offset (q * k + c) * n0
    local = [torch.from_numpy(ei.T.copy()).to(dev) + c * fam.n0 for c, ei in enumerate(fam.edge_index)]   # [e0_c, 2]
    ei = tile_rows(local, t, torch)
    e0 = torch.tensor(fam.e0, device=dev)
    per = int(e0.sum())
    full, rem = divmod(t, k)
    n_e = full * per + int(e0[:rem].sum())
    period_of_edge = torch.arange(n_e, device=dev) // per
    ei = (ei + (period_of_edge * (k * fam.n0))[:, None]).T.contiguous()
    return nodes, ea, ei


def copies_view(x, fam, t):
    """Node rows of a tiling [t * n0, w] -> [t, n0, w]."""
    return x.reshape(t, fam.n0, *x.shape[1:])


def worst_copy_error(out, refs, fam, t):
    """max |out - class reference| over all copies, per class: out [t * n0, w] (torch, device), refs K x [n0, w] (torch, same
    device, float64).  Returns a list of K floats (classes without a copy: 0)."""
    v = copies_view(out, fam, t)
    k = len(refs)
    return [float((v[c::k].double() - refs[c][None]).abs().max()) if c < t else 0.0 for c in range(k)]


def edge_rows_error(e_out, refs, fam, t):
    """The same for edge rows [E, w] laid out copy by copy: refs K x [e0_c, w]."""
    import torch
    k = len(refs)
    full, rem = divmod(t, k)
    per_ref = torch.cat(refs)
    per = per_ref.shape[0]
    worst = 0.0
    if full:
        worst = float((e_out[:full * per].reshape(full, per, -1).double() - per_ref[None]).abs().max())
    if rem:
        tail = torch.cat(refs[:rem])
        worst = max(worst, float((e_out[full * per:].double() - tail).abs().max()))
    return worst


# ------------------------------------------------------------------------------------------ references by class
def multiplicity(t, k=K):
    return [t // k + (1 if c < t % k else 0) for c in range(k)]


def class_targets(fam, out_dim=3, seed=4100):
    return [np.random.default_rng(seed + c).standard_normal((fam.n0, out_dim)).astype(np.float32) for c in range(len(fam.nodes))]


def class_forward_refs(fam, params, num_layers, m_steps):
    """The float64 numpy oracle's prediction of every class."""
    from oracle import epd_oracle as orc
    return [orc.epd_forward(params, fam.nodes[c], fam.edge_attr[c], fam.edge_index[c], num_layers, m_steps) for c in range(len(fam.nodes))]


def class_grad_refs(fam, params, targets, num_layers, m_steps, dtype=None, inputs=False):
    """oracle/torch_epd.py per class, for the loss sum |out - target| / n0 of ONE class graph: a list of K dicts with `out`, `loss`,
    `grads` (per parameter) and, with inputs=True, `d_nodes` / `d_edge_attr`."""
    import torch
    from oracle import torch_epd
    dtype = dtype or torch.float64
    res = []
    for c in range(len(fam.nodes)):
        p = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in params.items()}
        x = torch.tensor(fam.nodes[c], dtype=dtype, requires_grad=inputs)
        a = torch.tensor(fam.edge_attr[c], dtype=dtype, requires_grad=inputs)
        out = torch_epd.epd_forward(p, x, a, torch.tensor(fam.edge_index[c]), num_layers, m_steps)
        loss = torch.nn.functional.l1_loss(out, torch.tensor(targets[c], dtype=dtype), reduction="sum") / out.shape[0]
        loss.backward()
        r = dict(out=out.detach().numpy(), loss=float(loss.detach()), grads={k: v.grad.numpy() for k, v in p.items()})
        if inputs:
            r.update(d_nodes=x.grad.numpy(), d_edge_attr=a.grad.numpy())
        res.append(r)
    return res


def assemble_param_grads(class_refs, t):
    """Parameter gradients of the tiled loss sum_over_all_nodes |out - target| / (t * n0) from the class gradients (each of
    sum |.| / n0 on one class): the multiplicity-weighted mean, accumulated in float64."""
    mult = multiplicity(t, len(class_refs))
    return {name: sum(m * class_refs[c]["grads"][name].astype(np.float64) for c, m in enumerate(mult)) / t
            for name in class_refs[0]["grads"]}


def assemble_loss(class_refs, t):
    mult = multiplicity(t, len(class_refs))
    return sum(m * class_refs[c]["loss"] for c, m in enumerate(mult)) / t


def input_grad_scale(t):
    """Input gradients of copy t under the tiled loss are its class's times n0 / (t * n0)."""
    return 1.0 / t


def assembled_flip_allowance(fam, params, targets, num_layers, m_steps, t):
    """relu_flip_allowance per class, assembled like the gradients (a sum of per-class bounds bounds the sum)."""
    from oracle import torch_epd
    mult = multiplicity(t, len(fam.nodes))
    total = None
    for c, m in enumerate(mult):
        if not m:
            continue
        allow, _ = torch_epd.relu_flip_allowance(params, fam.nodes[c], fam.edge_attr[c], fam.edge_index[c], targets[c], num_layers, m_steps)
        total = {k: (total[k] if total else 0.0) + m * v / t for k, v in allow.items()}
    return total


# ------------------------------------------------------------------------------------------ a case and its regime
@dataclass
class OffsetCase:
    name: str
    family: Family
    copies: int
    hidden: int
    expect: dict = field(default_factory=dict)   # regime key -> the value it must have
    regime: dict = field(default_factory=dict)

    def measure(self):
        n, e = self.family.sizes(self.copies)
        hp = padded_hidden(self.hidden)
        arrays = dict(edge_rows=e * hp * 4, node_rows=n * hp * 4, p_table=n * 2 * hp * 4, agg=n * hp * 4,
                      cat3_rows=e * 3 * hp * 4)
        self.regime = dict(n=n, e=e, hidden=self.hidden, bytes=arrays, **{k: side_of(v) for k, v in arrays.items()},
                           edge_floats_beyond_int=bool(e * hp >= GIB2),   # a row index times the row width, formed in int, wraps
                           edge_sys_fits=bool(hp == SYS_H and e > 0 and edge_sys_fits(n, e)),
                           agg_side_bytes=(n + edge_groups_max(n, e)) * hp * 4,
                           wgrad_guard_ok=bool(wgrad_guard_ok(e, hp) and wgrad_guard_ok(n, hp)))
        return self

    def check(self):
        """The case is wrap-safe and in the regime it was built for."""
        self.family.check()
        assert self.expect, self.name
        n, e = self.regime["n"], self.regime["e"]
        assert 0 < n < GIB2 and 0 <= e < GIB2, (self.name, n, e)   # the library's documented range
        for key, want in self.expect.items():
            assert self.regime[key] == want, (self.name, key, self.regime[key], want)
        return self

    def describe(self):
        r = self.regime
        arrays = ", ".join(f"{k} {v / 2 ** 30:.3f} GiB ({r[k]})" for k, v in r["bytes"].items())
        return (f"{self.name}: T={self.copies} n={r['n']} E={r['e']} hidden={r['hidden']} | {arrays} | edge_sys_fits={r['edge_sys_fits']} "
                f"(agg+side {r['agg_side_bytes'] / 2 ** 30:.3f} GiB) wgrad_guard_ok={r['wgrad_guard_ok']}")


def make_case(name, family, copies, hidden, **expect):
    return OffsetCase(name, family, int(copies), int(hidden), expect).measure()


# ------------------------------------------------------------------------------------------ the cases of tests/test_gpu_offsets.py
def largest_systolic_tiling(fam, t_max):
    """The largest number of copies <= t_max whose tiling the systolic edge kernel still takes (edge_sys_fits)."""
    t = t_max
    while t > 0 and not edge_sys_fits(*fam.sizes(t)):
        t -= 1
    return t


@functools.lru_cache(maxsize=None)
def gpu_cases():
    """name -> OffsetCase, measured.  The copies are chosen for the regime named; `expect` is what each case exists for."""
    d, s = dense_family(), sparse_family()
    mid, high = "[2,4)GiB", ">=4GiB"
    cases = [
        # inference forward, streamed kernels at hidden 256
        make_case("F1", d, 108, 256, edge_rows=mid, edge_sys_fits=False),
        make_case("F1s2", d, 108, 256, edge_rows=mid, edge_sys_fits=False),
        make_case("F2", d, 211, 256, edge_rows=high, edge_sys_fits=False, edge_floats_beyond_int=False),
        make_case("F2c", d, 412, 256, edge_rows=high, edge_floats_beyond_int=True),
        # inference forward, hidden 128: the systolic route
        make_case("F3", d, 211, 128, edge_rows=mid, edge_sys_fits=True),
        make_case("F3s2", d, 211, 128, edge_rows=mid, edge_sys_fits=True),
        make_case("F4", d, 417, 128, edge_rows=high, edge_sys_fits=True),
        # the sparse family: the route switch.  F5: the last tiling the systolic kernel takes (its P rows and its side-buffer rows at
        # 32-bit offsets beyond 2 GiB); F5b: the P table still below 4 GiB, agg + side buffer not; F6: the P table beyond 4 GiB, agg
        # beyond 2 GiB (n >= 2^22 is where both happen: a P row is two agg rows)
        make_case("F5", s, largest_systolic_tiling(s, 4108), 128, p_table=mid, edge_sys_fits=True),
        make_case("F5b", s, 4108, 128, p_table=mid, agg="<2GiB", edge_sys_fits=False),
        make_case("F6", s, 4109, 128, p_table=high, agg=mid, edge_sys_fits=False),
        # the stand-alone block's inference forward, edges in a random order
        make_case("B1", d, 108, 256, edge_rows=mid),
        # training steps
        make_case("T0", d, 211, 128, edge_rows=mid, wgrad_guard_ok=True),
        make_case("T1", d, 204, 256, edge_rows=mid, wgrad_guard_ok=True),
        make_case("T2", d, 206, 256, edge_rows=high, wgrad_guard_ok=False),
        make_case("T2g", d, 206, 256, edge_rows=high, wgrad_guard_ok=False),
        make_case("T1g", d, 204, 256, edge_rows=mid, wgrad_guard_ok=True),
        # rollout step of a batch of candidates: 211 x 1021 nodes (the edge count is the scene's: test_gpu_offsets.py asserts it)
        make_case("R1", d, 211, 128, edge_rows=mid, edge_sys_fits=True),
    ]
    return {c.name: c for c in cases}
