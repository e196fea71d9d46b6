"""GPU: the training-batch path (gm_train_batch_build / gm_train_batch_edges, CoffeeDataset.batch, GraphLoader(fused=True)) held
to the existing chain of torch calls and HIP entry points bit for bit, to the float32 oracle at the bars of
tests/test_gpu_dataset.py, and -- the draw -- to the numpy restatement of tests/train_batch_cases.py.

With an injected draw the existing torch chain (torch.cumsum over the outer dimension adds left to right) agrees bit for bit on the
MI355X too, so that comparison is held to equality like the one with the oracle."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from conftest import BOUNDS, STATS
from oracle import epd_oracle as orc
from gpu_support import dev, to_dev
import train_batch_cases as tc

pytestmark = pytest.mark.gpu
F32 = np.float32


# ------------------------------------------------------------------------------------------ plumbing
def _bits(a):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else a


def assert_same_bits(got, want, what=""):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    bad = np.argwhere(g != w)
    assert bad.size == 0, (what, len(bad), bad[:4].tolist())


def fdesc(k, control):
    from gnn_manip_amd.graph import make_feature_desc
    return make_feature_desc(tc.R, STATS, BOUNDS, tc.CART, [tc.MAT], tc.CTRL if control else None, k, tc.REC_DIM + (3 if control else 0))


def graph_attr(control, noise=None, max_nb=20):
    from gnn_manip_amd import GraphBoundedMultimaterial, GraphBoundedMultimaterialControl
    if control:
        return GraphBoundedMultimaterialControl(tc.R, STATS, tc.CART, [tc.MAT], tc.CTRL, BOUNDS, noise=noise, max_neighbours=max_nb)
    return GraphBoundedMultimaterial(tc.R, STATS, tc.CART, [tc.MAT], BOUNDS, noise=noise, max_neighbours=max_nb)


class Build:
    """The two phases through ctypes.  frames: [(recording tensor [T, N, 5], first frame)]."""

    def __init__(self, dev, frames, k, control, max_nb, ws=None, noise_std=0.0, seed=0, first_stream=0, noise_sample=None, windows=True):
        from gnn_manip_amd._lib import check, current_stream, lib, ptr
        self.L, self.dev, self.b, self.n, self.k_nb = lib(), dev, len(frames), int(frames[0][0].shape[1]), max_nb
        self.fd = fdesc(k, control)
        d, f = tc.REC_DIM + (3 if control else 0), 3 * (k - 1) + 7 + (3 if control else 0)
        need = self.L.gm_train_batch_workspace_bytes(C.byref(self.fd), self.b, self.n, max_nb)
        assert need > 0
        self.ws = torch.empty(need, dtype=torch.uint8, device=dev) if ws is None else ws
        assert self.ws.numel() >= need
        self.keep = [r for r, _ in frames]
        ptrs = (C.c_void_p * self.b)(*[r.data_ptr() + t * r.shape[1] * r.shape[2] * 4 for r, t in frames])
        nan = float("nan")
        self.nodes = torch.full((self.b * self.n, f), nan, device=dev)
        self.target = torch.full((self.b * self.n, 3), nan, device=dev)
        self.windows = torch.full((self.b, k, self.n, d), nan, device=dev) if windows else None
        check(self.L.gm_train_batch_build(ptrs, self.b, self.n, tc.REC_DIM, C.byref(self.fd), max_nb, float(noise_std), seed, first_stream,
                                          ptr(noise_sample), ptr(self.nodes), ptr(self.target), ptr(self.windows), ptr(self.ws), need,
                                          current_stream(dev)))

    def record(self, pinned_row):
        """Asynchronous copy of the 16-byte record, and the event behind it."""
        pinned_row.copy_(self.ws[:16].view(torch.int32), non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        return ev

    def count(self):
        from gnn_manip_amd._lib import current_stream
        e = C.c_int64(-1)
        rc = self.L.gm_train_batch_num_edges(C.c_void_p(self.ws.data_ptr()), C.byref(e), current_stream(self.dev))
        return rc, int(e.value)

    def edges(self, e):
        from gnn_manip_amd._lib import check, current_stream, ptr
        self.edge_index = torch.full((2, e), -7, dtype=torch.int64, device=self.dev)
        self.edge_attr = torch.full((e, 4), float("nan"), device=self.dev)
        check(self.L.gm_train_batch_edges(ptr(self.ws), self.b, self.n, C.byref(self.fd), self.k_nb, e, ptr(self.edge_index),
                                          ptr(self.edge_attr), current_stream(self.dev)))
        return self

    def finish(self):
        rc, e = self.count()
        assert rc == 0 and 0 < e <= self.b * self.n * self.k_nb, (rc, e)
        return self.edges(e)

    def outputs(self):
        return dict(nodes=self.nodes, target=self.target, windows=self.windows, edge_index=self.edge_index, edge_attr=self.edge_attr)


_REC = {}


def case_frames(name, dev):
    """The case's recordings on the device (once per module) and its samples as Build takes them."""
    c = tc.CASES[name]
    if name not in _REC:
        _REC[name] = [to_dev(r, dev) for r in c.recordings()]
    return c, [(_REC[name][r], t) for r, t in c.samples]


def torch_samples(c, frames):
    """sample()'s arithmetic (gnn_manip_amd/dataset.py) on the case's frames: [(obs_seq [k, N, D], next_pos [N, 3])]."""
    out = []
    for data, t in frames:
        obs = data[t:t + c.k]
        nxt = data[t + c.k][:, 2:5]
        if c.control:
            ctr = nxt.unsqueeze(0) - obs[:, :, 2:5]
            ctr = torch.where((obs[:, :, tc.MAT] != 1).unsqueeze(-1), torch.zeros_like(ctr), ctr)
            obs = torch.cat((obs, ctr), dim=-1)
        out.append((obs.clone().contiguous(), nxt.clone().contiguous()))
    return out


def dataset_of(recordings, k, control, dev, noise=None, max_nb=20):
    """A CoffeeDataset over resident recordings (possibly of different N), without the files."""
    from gnn_manip_amd import CoffeeDataset
    return CoffeeDataset.from_recordings(list(recordings), k, tc.R, STATS, BOUNDS, tc.CART, tc.MAT, tc.CTRL, noise=noise, use_control=control,
                                         max_neighbours=max_nb)


def assert_outputs_follow_windows(out, c, nxt_noisy, max_nb, dev, what):
    """nodes, target, edge_index and edge_attr are, bit for bit, what the existing entry points make of `windows`."""
    from gnn_manip_amd import get_connectivity, get_edges_displacement
    ga = graph_attr(c.control)
    w = out["windows"]
    assert_same_bits(out["nodes"], torch.cat([ga.compute_nodes(w[b]) for b in range(c.B)]), what + " nodes")
    assert_same_bits(out["target"], torch.cat([ga.compute_target(w[b], nxt_noisy[b]) for b in range(c.B)]), what + " target")
    last = w[:, -1, :, 2:5].reshape(-1, 3).contiguous()
    s, r = get_connectivity(last, tc.R, max_nb, nodes_per_graph=c.n)
    assert_same_bits(out["edge_index"], torch.stack((s, r)), what + " edge_index")
    assert_same_bits(out["edge_attr"], get_edges_displacement(last, s, r, tc.R), what + " edge_attr")
    ei = out["edge_index"].cpu().numpy()
    assert (ei[0] // c.n == ei[1] // c.n).all() and (np.diff(ei[0]) >= 0).all()          # no edge crosses graphs; grouped by sender


# ------------------------------------------------------------------------------------------ 1. no noise
@pytest.mark.parametrize("name", tc.ALL_CASES)
def test_no_noise_is_the_existing_chain(dev, name):
    c, frames = case_frames(name, dev)
    out = Build(dev, frames, c.k, c.control, 20).finish().outputs()
    samples = torch_samples(c, frames)
    nodes, ea, ei, tgt = graph_attr(c.control).process_collate(samples)
    assert_same_bits(out["windows"], torch.stack([o for o, _ in samples]), "windows")
    for key, want in (("nodes", nodes), ("edge_attr", ea), ("edge_index", ei), ("target", tgt)):
        assert_same_bits(out[key], want, key)
    # ... through CoffeeDataset.batch, whose noise-free graph has 20 neighbours whatever max_neighbours says
    ds = dataset_of(_REC[name], c.k, c.control, dev, noise=None, max_nb=c.max_nb)
    idx = [ds.index.index(s) for s in c.samples]
    got = ds.batch(idx)
    for key, want in (("x", nodes), ("edge_attr", ea), ("edge_index", ei), ("y", tgt)):
        assert_same_bits(getattr(got, key), want, "batch " + key)
    # ... and the oracle
    o_nodes, o_ea, o_ei, o_tgt = orc.process_collate(c.windows(), **c.graph_kw(20))
    np.testing.assert_array_equal(out["edge_index"].cpu().numpy(), o_ei)
    np.testing.assert_allclose(out["nodes"].cpu().numpy(), o_nodes, rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(out["edge_attr"].cpu().numpy(), o_ea, rtol=2e-6, atol=1e-6)
    np.testing.assert_allclose(out["target"].cpu().numpy(), o_tgt, rtol=1e-5, atol=2e-4)
    assert_same_bits(out["windows"], np.stack([o for o, _ in c.windows()]), "windows / oracle")
    # without `windows` nothing else changes
    lean = Build(dev, frames, c.k, c.control, 20, windows=False).finish().outputs()
    for key in ("nodes", "target", "edge_index", "edge_attr"):
        assert_same_bits(lean[key], out[key], "no windows " + key)


# ------------------------------------------------------------------------------------------ 2. injected noise
@pytest.mark.parametrize("name", tc.INJECTED_CASES)
def test_injected_noise(dev, name):
    c, frames = case_frames(name, dev)
    ns = np.stack([tc.noise_sample32(77, 5 + b, c.n, c.k, tc.NOISE_STD) for b in range(c.B)])
    out = Build(dev, frames, c.k, c.control, c.max_nb, noise_sample=to_dev(ns, dev)).finish().outputs()
    # the oracle's obs + noise: a float32 left-to-right double running sum and one add
    assert_same_bits(out["windows"], tc.noisy_windows(c, ns), "windows")
    clean = c.windows()
    seq_last = [orc.random_walk_noise(clean[b][0][:, :, tc.CART], None, ns[b])[-1] for b in range(c.B)]
    nxt = [to_dev(clean[b][1] + seq_last[b], dev) for b in range(c.B)]
    assert_outputs_follow_windows(out, c, nxt, c.max_nb, dev, name)
    # the oracle's noisy path at the bars of test_gpu_dataset.py::test_noise_path_golden
    o_nodes, o_ea, o_ei, o_tgt = tc.collate([orc.process_noisy(clean[b][0], clean[b][1], ns[b], **c.graph_kw()) for b in range(c.B)])
    np.testing.assert_array_equal(out["edge_index"].cpu().numpy(), o_ei)
    np.testing.assert_allclose(out["nodes"].cpu().numpy(), o_nodes, rtol=2e-6, atol=3e-5)
    np.testing.assert_allclose(out["edge_attr"].cpu().numpy(), o_ea, rtol=2e-6, atol=4e-6)
    np.testing.assert_allclose(out["target"].cpu().numpy(), o_tgt, rtol=1e-5, atol=6e-4)
    if name == "cap5":
        cnt = np.bincount(o_ei[0], minlength=c.B * c.n)
        assert cnt.max() == c.max_nb and (cnt == c.max_nb).sum() > c.n                       # the cap binds
    # the existing chain with the same draw: torch's scan adds left to right too
    ga = graph_attr(c.control, noise=tc.NOISE_STD, max_nb=c.max_nb)
    parts = [ga.process(o, t, noise_sample=to_dev(ns[b], dev)) for b, (o, t) in enumerate(torch_samples(c, frames))]
    off = 0
    for b, (nodes, ea, s, r, tgt) in enumerate(parts):
        rows = slice(b * c.n, (b + 1) * c.n)
        mine = (out["edge_index"][0] >= b * c.n) & (out["edge_index"][0] < (b + 1) * c.n)
        assert_same_bits(out["nodes"][rows], nodes, "chain nodes")
        assert_same_bits(out["target"][rows], tgt, "chain target")
        assert_same_bits(out["edge_index"][:, mine], torch.stack((s, r)) + off, "chain edge_index")
        assert_same_bits(out["edge_attr"][mine], ea, "chain edge_attr")
        off += c.n


# ------------------------------------------------------------------------------------------ 3. seeded noise on zeros
def test_seeded_noise_is_the_headers_draw(dev):
    """On positions that are exactly 0 the window's xyz IS the noise sequence.  Every element lies within
    4 x F32_DRAW_ERR x noise_std x (sum of the running-sum weights of its frame) of the float64 restatement; the worst ratio to
    that bound is printed (MI355X: 0.080 in frame 1, falling to 0.040 in frame 5, with F32_DRAW_ERR = 1.53e-6)."""
    c, frames = case_frames("zeros", dev)
    seed, stream = (0x1234 << 32) | 0x9abc, (1 << 32) + 3          # both words of both in use
    out = Build(dev, frames, c.k, c.control, c.max_nb, noise_std=tc.NOISE_STD, seed=seed, first_stream=stream).finish().outputs()
    w = out["windows"].cpu().numpy()[0]
    got = w[:, :, tc.CART]
    assert not got[0].any()
    want = tc.noise_sequence64(tc.noise_sample64(seed, stream, c.n, c.k, tc.NOISE_STD))
    bound = 4 * tc.F32_DRAW_ERR * tc.NOISE_STD * tc.running_sum_weights(c.k)
    err = np.abs(got.astype(np.float64) - want).max(axis=(1, 2))
    print("seeded draw: worst |error| / bound per frame", (err[1:] / bound[1:]).round(4).tolist(), "F32_DRAW_ERR", tc.F32_DRAW_ERR)
    assert (err[1:] <= bound[1:]).all(), (err, bound)
    vel = (got[-1].astype(np.float64) - got[-2].astype(np.float64)).ravel()
    n = vel.size
    assert abs(vel.std() / tc.NOISE_STD - 1.0) <= 6.0 / np.sqrt(2 * n)
    assert abs(vel.mean()) <= 6.0 * tc.NOISE_STD / np.sqrt(n)
    # the other columns are the recording's, the control of rows that do not move is 0, and the rest follows the window
    assert_same_bits(np.delete(w, tc.CART, axis=2), np.delete(c.windows()[0][0], tc.CART, axis=2), "other columns")
    assert_outputs_follow_windows(out, c, [out["windows"][0, -1, :, 2:5].contiguous()], c.max_nb, dev, "zeros")   # next = 0: next' = seq[-1]


def device_sequences(dev, c, seed, first_stream):
    """[B, k, N, 3] float32: the noise sequences the device adds for (seed, first_stream + b) -- the windows of all-zero recordings
    of the same shape (a sample's noise depends on seed, stream and particle alone)."""
    zero = torch.zeros((c.k + 1, c.n, tc.REC_DIM), device=dev)
    b = Build(dev, [(zero, 0)] * c.B, c.k, False, c.max_nb, noise_std=tc.NOISE_STD, seed=seed, first_stream=first_stream)
    return b.windows[:, :, :, 2:5].cpu().numpy()


# ------------------------------------------------------------------------------------------ 4. seeded noise on a scene
def test_seeded_noise_on_a_scene(dev):
    c, frames = case_frames("three97", dev)
    seed, stream = 5, 40
    out = Build(dev, frames, c.k, c.control, c.max_nb, noise_std=tc.NOISE_STD, seed=seed, first_stream=stream).finish().outputs()
    w = out["windows"].cpu().numpy()
    clean = c.windows()
    seq_dev = device_sequences(dev, c, seed, stream)
    nxt = []
    for b in range(c.B):
        ref = clean[b][0][:, :, tc.CART].astype(np.float64) + tc.noise_sequence64(tc.noise_sample64(seed, stream + b, c.n, c.k, tc.NOISE_STD))
        err = np.abs(w[b][:, :, tc.CART].astype(np.float64) - ref)
        assert (err <= np.spacing(np.abs(ref).astype(F32))).all(), (b, float(err.max()))
        assert_same_bits(w[b][:, :, tc.CART], clean[b][0][:, :, tc.CART] + seq_dev[b], "xyz + the device's sequence")
        assert_same_bits(np.delete(w[b], tc.CART, axis=2), np.delete(clean[b][0], tc.CART, axis=2), "other columns")
        nxt.append(to_dev(clean[b][1] + seq_dev[b][-1], dev))
    assert not np.array_equal(w[:, 1], np.stack([o for o, _ in clean])[:, 1])                 # there IS noise from frame 1 on
    assert_outputs_follow_windows(out, c, nxt, c.max_nb, dev, "three97 seeded")


# ------------------------------------------------------------------------------------------ 5. streams
def _graph_of(out, b, n):
    mine = (out["edge_index"][0] >= b * n) & (out["edge_index"][0] < (b + 1) * n)
    return out["edge_index"][:, mine] - b * n, out["edge_attr"][mine]


def test_streams_do_not_depend_on_the_batch(dev):
    c, frames = case_frames("three97", dev)
    seed, s0 = 9, (1 << 32) - 1                                  # the stream's low word wraps inside the batch
    kw = dict(noise_std=tc.NOISE_STD, seed=seed)
    full = Build(dev, frames, c.k, c.control, c.max_nb, first_stream=s0, **kw).finish().outputs()
    for b in range(c.B):
        one = Build(dev, [frames[b]], c.k, c.control, c.max_nb, first_stream=s0 + b, **kw).finish().outputs()
        rows = slice(b * c.n, (b + 1) * c.n)
        assert_same_bits(full["windows"][b], one["windows"][0], "windows")
        assert_same_bits(full["nodes"][rows], one["nodes"], "nodes")
        assert_same_bits(full["target"][rows], one["target"], "target")
        ei, ea = _graph_of(full, b, c.n)
        assert_same_bits(ei, one["edge_index"], "edge_index")
        assert_same_bits(ea, one["edge_attr"], "edge_attr")
    # the workspace's old contents play no part
    need = full_ws_bytes = Build(dev, frames, c.k, c.control, c.max_nb).ws.numel()
    for fill in (lambda: torch.full((need,), 0xff, dtype=torch.uint8, device=dev),
                 lambda: torch.full((need // 4 + 1,), 0x7fc00000, dtype=torch.int32, device=dev).view(torch.uint8)):
        again = Build(dev, frames, c.k, c.control, c.max_nb, ws=fill(), first_stream=s0, **kw).finish().outputs()
        for key in full:
            assert_same_bits(again[key], full[key], "poisoned workspace " + key)
    assert full_ws_bytes > 0
    other = Build(dev, frames, c.k, c.control, c.max_nb, first_stream=s0, noise_std=tc.NOISE_STD, seed=seed + 1).finish().outputs()
    assert not np.array_equal(other["windows"][:, 1:].cpu().numpy(), full["windows"][:, 1:].cpu().numpy())
    assert_same_bits(other["windows"][:, 0], full["windows"][:, 0], "frame 0 carries no noise")


# ------------------------------------------------------------------------------------------ 6. two batches in flight
def test_two_batches_in_flight(dev):
    ca, fa = case_frames("three97", dev)
    cb, fb = case_frames("cap5", dev)
    kwa = dict(noise_std=tc.NOISE_STD, seed=3, first_stream=0)
    kwb = dict(noise_std=tc.NOISE_STD, seed=3, first_stream=ca.B)
    alone_a = Build(dev, fa, ca.k, ca.control, ca.max_nb, **kwa).finish()
    alone_b = Build(dev, fb, cb.k, cb.control, cb.max_nb, **kwb).finish()
    pinned = torch.zeros((2, 4), dtype=torch.int32).pin_memory()
    a = Build(dev, fa, ca.k, ca.control, ca.max_nb, **kwa)                   # phase 1 of A into workspace 0
    ev_a = a.record(pinned[0])
    b = Build(dev, fb, cb.k, cb.control, cb.max_nb, **kwb)                   # phase 1 of B into workspace 1, A's phase 2 still to come
    ev_b = b.record(pinned[1])
    counts = []
    for ev, row in ((ev_a, pinned[0]), (ev_b, pinned[1])):
        ev.synchronize()
        e = C.c_int64(-1)
        assert a.L.gm_train_batch_status(C.c_void_p(row.data_ptr()), C.byref(e)) == 0
        counts.append(int(e.value))
    a.edges(counts[0])
    b.edges(counts[1])
    assert (0, counts[0]) == a.count() and (0, counts[1]) == b.count()
    assert counts == [alone_a.edge_index.shape[1], alone_b.edge_index.shape[1]] and counts[0] != counts[1]
    for got, want in ((a, alone_a), (b, alone_b)):
        for key, v in want.outputs().items():
            assert_same_bits(got.outputs()[key], v, "in flight " + key)


def test_non_finite_recording_is_reported(dev):
    c, frames = case_frames("one64", dev)
    for frame, row in ((0, 5), (c.k, 63), (c.k - 1, 0)):        # the first frame, the frame behind the window, the last frame
        bad = frames[0][0].clone()
        bad[frame, row, 3] = float("nan")
        b = Build(dev, [(bad, 0)], c.k, c.control, c.max_nb)
        pinned = torch.zeros((1, 4), dtype=torch.int32).pin_memory()
        b.record(pinned[0]).synchronize()
        assert b.L.gm_train_batch_status(C.c_void_p(pinned.data_ptr()), None) == -5
        assert b"non-finite position" in b.L.gm_last_error()
        rc, _ = b.count()
        assert rc == -5
    good = Build(dev, frames, c.k, c.control, c.max_nb)          # and the flag does not outlive its build
    assert good.count()[0] == 0


# ------------------------------------------------------------------------------------------ 7. the loader
def _write_dataset(g, root):
    """The synthetic dataset fixture G9 was generated from, as tests/test_gpu_dataset.py writes it."""
    os.makedirs(root + "train")
    with open(root + "metadata.json", "w") as fp:
        fp.write(bytes(g["meta_json"]).decode())
    with open(root + "train/sim_data.csv", "w") as fp:
        for sid in (1, 2):
            fp.write(f"{sid},0\n")
    for sid, d in zip((1, 2), g["sims"]):
        np.savetxt(root + f"train/particles_{sid:06d}.csv", d.reshape(-1, 5).astype(np.float64), delimiter=",", fmt="%.9g")


@pytest.fixture(scope="module")
def g9_root(golden, tmp_path_factory):
    root = str(tmp_path_factory.mktemp("g9")) + "/"
    _write_dataset(golden("g9_dataset.npz"), root)
    return root


def assert_same_batches(got, want, what):
    assert len(got) == len(want) > 0
    for i, (a, b) in enumerate(zip(got, want)):
        for key in ("x", "edge_attr", "edge_index", "y"):
            assert_same_bits(getattr(a, key), getattr(b, key), f"{what} batch {i} {key}")


@pytest.mark.parametrize("use_control", [True, False])
def test_loader_without_noise_is_the_unfused_loader(dev, g9_root, use_control):
    from gnn_manip_amd import CoffeeDataset, GraphLoader
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", device=dev, use_control=use_control, max_neighbours=7)
    want = list(GraphLoader(ds, batch_size=2, shuffle=True, seed=4))
    assert len(want) == 3
    for prefetch in (0, 1):
        assert_same_batches(list(GraphLoader(ds, batch_size=2, shuffle=True, seed=4, fused=True, prefetch=prefetch)), want, f"prefetch={prefetch}")
    # a ragged last batch, and batches of one
    assert_same_batches(list(GraphLoader(ds, batch_size=4, fused=True)), list(GraphLoader(ds, batch_size=4)), "batch_size=4")
    assert_same_batches(list(GraphLoader(ds, batch_size=1, fused=True)), list(GraphLoader(ds, batch_size=1)), "batch_size=1")


def test_loader_noise_prefetch_and_seeds(dev, g9_root):
    from gnn_manip_amd import CoffeeDataset, GraphLoader
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=tc.NOISE_STD, device=dev, use_control=True, max_neighbours=9)

    def two_epochs(**kw):
        loader = GraphLoader(ds, batch_size=2, shuffle=False, fused=True, **kw)
        return [list(loader), list(loader)]

    e0 = two_epochs(seed=8, prefetch=0)
    e1 = two_epochs(seed=8, prefetch=1)
    for ep in range(2):
        assert_same_batches(e1[ep], e0[ep], f"prefetch 1 against 0, epoch {ep}")
    assert_same_batches(two_epochs(seed=8, prefetch=1)[1], e1[1], "the same seed again")
    first, again = e1[0][0], e1[1][0]
    assert_same_bits(first.x[:, -4], again.x[:, -4], "material column")                        # the same samples ...
    assert not np.array_equal(first.x.cpu().numpy(), again.x.cpu().numpy())                    # ... under another epoch's noise
    assert not np.array_equal(two_epochs(seed=9, prefetch=1)[0][0].x.cpu().numpy(), first.x.cpu().numpy())
    # batch i of the run holds samples 2 i, 2 i + 1 on streams 2 i, 2 i + 1 of the seed: CoffeeDataset.batch gives the same
    assert_same_batches([ds.batch([2, 3], seed=8, first_stream=2)], [e1[0][1]], "CoffeeDataset.batch")
    assert_same_batches([ds.batch([0, 1], seed=8, first_stream=len(ds))], [e1[1][0]], "epoch 2 continues the streams")
    n = ds.sims[0].shape[1]
    cnt = np.bincount(first.edge_index[0].cpu().numpy(), minlength=2 * n)
    assert cnt.max() <= 9                                                                        # the noisy path honours max_neighbours
    none = GraphLoader(ds, batch_size=2, fused=True)                                             # seed None: drawn from the loader's rng
    assert isinstance(none.noise_seed, int) and none.noise_seed != GraphLoader(ds, batch_size=2, fused=True).noise_seed


def test_loader_mixed_sizes(dev):
    from gnn_manip_amd import GraphLoader
    from gnn_manip_amd.dataset import collate_graphs
    recs = [to_dev(tc.Case("mixed", n, 6, [(0, 1)], seed=7 + n).recordings()[0], dev) for n in tc.MIXED_N]
    assert [int(r.shape[1]) for r in recs] == [64, 97]
    ds = dataset_of(recs, 6, True, dev, noise=tc.NOISE_STD, max_nb=12)
    assert len(ds) == 4                                                    # T = 8: two windows per recording
    loader = GraphLoader(ds, batch_size=3, shuffle=False, seed=21, fused=True)
    batches = list(loader)
    assert [b.num_nodes for b in batches] == [64 + 64 + 97, 97]
    want = collate_graphs([ds.batch([i], seed=21, first_stream=i) for i in range(3)])
    assert_same_batches([batches[0]], [want], "mixedN")
    assert_same_batches([batches[1]], [ds.batch([3], seed=21, first_stream=3)], "mixedN tail")
    ei = batches[0].edge_index.cpu().numpy()
    graph = np.searchsorted([64, 128, 225], ei, side="right")
    assert (graph[0] == graph[1]).all() and set(graph[0]) == {0, 1, 2}


def test_loader_does_not_synchronise(dev, g9_root, monkeypatch):
    from gnn_manip_amd import CoffeeDataset, GraphLoader, _lib
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=tc.NOISE_STD, device=dev, use_control=True)
    want = list(GraphLoader(ds, batch_size=1, seed=2, fused=True, prefetch=1))
    calls = []
    L = _lib.lib()

    def spy(name, fn):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped

    for name in _lib.PROTOTYPES:
        if name.endswith("_num_edges"):
            monkeypatch.setattr(L, name, spy(name, getattr(L, name)))
    monkeypatch.setattr(torch.cuda, "synchronize", spy("torch.cuda.synchronize", torch.cuda.synchronize))
    monkeypatch.setattr(torch.cuda.Stream, "synchronize", spy("Stream.synchronize", torch.cuda.Stream.synchronize))
    built = []
    orig_build = L.gm_train_batch_build
    monkeypatch.setattr(L, "gm_train_batch_build", lambda *a: (built.append(len(got)), orig_build(*a))[1])
    got = []
    for batch in GraphLoader(ds, batch_size=1, seed=2, fused=True, prefetch=1):
        got.append(batch)
    assert calls == [], calls
    assert built == [0, 0, 1, 2, 3, 4]            # batch i + 1 was built before batch i was handed out
    assert_same_batches(got, want, "under the spies")


def test_training_loop_with_the_fused_loader(dev, g9_root):
    """The loop of tests/test_gpu_dataset.py::test_training_loop_over_noisy_dataset with fused=True: its loss falls."""
    from gnn_manip_amd import CoffeeDataset, EncProcDecGNN, GraphLoader
    ds = CoffeeDataset(g9_root, 6, 0.015, split="train", noise=1e-7, device=dev, use_control=True)
    loader = GraphLoader(ds, batch_size=2, shuffle=True, seed=1, fused=True)
    torch.manual_seed(0)
    model = EncProcDecGNN(25, 4, 3, 128, 2, 2).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    crit = torch.nn.L1Loss(reduction="sum")
    first = last = None
    for epoch in range(6):
        tot = 0.0
        for batch in loader:
            pred = model.forward(batch.x, batch.edge_attr, batch.edge_index)
            loss = crit(pred, batch.y) / pred.shape[0]
            opt.zero_grad()
            loss.backward()
            opt.step()
            tot += float(loss.detach())
        first = tot if first is None else first
        last = tot
    assert np.isfinite(last) and last < first, (first, last)
