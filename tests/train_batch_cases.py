"""Cases and numpy restatements of the training-batch path (gm_train_batch_build / gm_train_batch_edges, CoffeeDataset.batch,
GraphLoader(fused=True)).  tests/test_train_batch_cases.py holds the restatements to published vectors and to fixture G9 on the
CPU, tests/test_gpu_train_batch.py holds the HIP kernel to them.

What is restated HERE is the draw alone: Philox4x32-10 and the Box-Muller normals of include/gnn_manip_hip.h, as float64 normals
and as a float32 variant with every operation rounded.  Everything else -- the samples, the random walk, the noisy features, the
collate -- is the oracle's (oracle/epd_oracle.py: dataset_samples, random_walk_noise, process_noisy, process_collate), float32
numpy already."""
import numpy as np

from conftest import BOUNDS, STATS
from gnn_manip_amd import scene
from oracle import epd_oracle as orc

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
R = 0.015
GM_TRAIN_BATCH_MAX = 64
NOISE_STD = 3e-4
REC_DIM = 5
CART, MAT, CTRL = [2, 3, 4], 1, [5, 6, 7]          # make_scene's columns; the dataset appends the control columns at rec_dim


class Case:
    """B samples (recording, first frame) of N particles and windows of k frames."""

    def __init__(self, name, n, k, samples, control=True, max_nb=20, zero=False, seed=0):
        self.name, self.n, self.k, self.samples, self.control, self.max_nb, self.zero = name, n, k, samples, control, max_nb, zero
        self.seed = seed
        self.T = k + 1 + max(t for _, t in samples)
        self.B = len(samples)
        self.D = REC_DIM + (3 if control else 0)
        self.F = 3 * (k - 1) + 7 + (3 if control else 0)

    def recordings(self):
        """The case's recordings [T, N, 5] float32, read-only: rigid (the last tenth of the rows) and granular rows, drifting."""
        out = []
        for r in range(1 + max(r for r, _ in self.samples)):
            rec = np.ascontiguousarray(scene.make_scene(self.n, seed=4100 + 17 * self.seed + r, k=self.T)[:, :, :REC_DIM])
            if self.zero:
                rec[:, :, CART] = 0.0
            rec.setflags(write=False)
            out.append(rec)
        return out

    def windows(self):
        """[(obs [k, N, D], next [N, 3])] of the samples, clean: the oracle's dataset_samples."""
        per_rec = [orc.dataset_samples([rec.reshape(-1, REC_DIM)], self.T, REC_DIM, self.k, CART, MAT, self.control)
                   for rec in self.recordings()]
        return [(per_rec[r][0][t], per_rec[r][1][t]) for r, t in self.samples]

    def graph_kw(self, max_nb=None):
        return dict(stats=STATS, bounds=BOUNDS, conn_r=R, cartesian_idx=CART, material_idx=[MAT],
                    control_idx=CTRL if self.control else None, max_neighbours=self.max_nb if max_nb is None else max_nb)


CASES = {c.name: c for c in (
    Case("one64", 64, 6, [(0, 0)], seed=1),
    Case("three97", 97, 6, [(0, 0), (0, 2), (1, 1)], seed=2),     # two recordings; samples 0 and 1 overlap in frames 2..6
    Case("k2", 130, 2, [(0, 0), (0, 1)], seed=3),
    Case("cap5", 300, 6, [(0, 0), (0, 1)], max_nb=5, seed=4),
    Case("noctl", 97, 6, [(0, 0), (1, 0)], control=False, seed=5),
    Case("zeros", 4096, 6, [(0, 0)], zero=True, seed=6),
)}
ALL_CASES = tuple(CASES)
INJECTED_CASES = ("three97", "k2", "cap5", "noctl")
MIXED_N = (64, 97)                     # `mixedN`: samples of both sizes in one loader batch


def collate(parts):
    """(nodes, edge_attr, senders, receivers, target) per graph -> the collated batch, offsets N * i (collate_utils.py:68-87)."""
    off, nl, el, il, tl = 0, [], [], [], []
    for nodes, ea, s, r, t in parts:
        nl.append(nodes)
        el.append(ea)
        il.append(np.stack((s, r)) + off)
        tl.append(t)
        off += nodes.shape[0]
    return np.concatenate(nl), np.concatenate(el), np.concatenate(il, axis=1), np.concatenate(tl)


def noisy_windows(case, samples):
    """[B, k, N, D]: the oracle's obs + noise of every sample, samples [B, k - 1, N, 3] the scaled draws."""
    out = []
    for (obs, _), ns in zip(case.windows(), samples):
        noise = np.zeros_like(obs)
        noise[:, :, CART] = orc.random_walk_noise(obs[:, :, CART], None, ns)
        out.append(obs + noise)
    return np.stack(out)


# ------------------------------------------------------------------------------------------ the draw
PHILOX_M = (0xD2511F53, 0xCD9E8D57)
PHILOX_W = (0x9E3779B9, 0xBB67AE85)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3, SC'11): counter [..., 4],
    key [..., 2] (or [2]) uint32 -> [..., 4] uint32."""
    c = [np.asarray(counter, U64)[..., i] & U64(0xffffffff) for i in range(4)]
    key = np.broadcast_to(np.asarray(key, U64), c[0].shape + (2,))
    k = [key[..., 0] & U64(0xffffffff), key[..., 1] & U64(0xffffffff)]
    mask = U64(0xffffffff)
    for _ in range(10):
        p0, p1 = U64(PHILOX_M[0]) * c[0], U64(PHILOX_M[1]) * c[2]
        c = [(p1 >> U64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> U64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + U64(PHILOX_W[0])) & mask, (k[1] + U64(PHILOX_W[1])) & mask]
    return np.stack(c, axis=-1).astype(U32)


def draw_words(seed, stream, n, k):
    """uint32 [N, calls, 4]: the Philox outputs a sample of N particles and k frames consumes (header: counter = (particle, j,
    stream low, stream high), key = (seed low, seed high))."""
    calls = (3 * (k - 1) + 3) // 4
    ctr = np.zeros((n, calls, 4), U64)
    ctr[:, :, 0] = np.arange(n, dtype=U64)[:, None]
    ctr[:, :, 1] = np.arange(calls, dtype=U64)[None, :]
    ctr[:, :, 2] = int(stream) & 0xffffffff
    ctr[:, :, 3] = (int(stream) >> 32) & 0xffffffff
    return philox4x32_10(ctr, np.array([int(seed) & 0xffffffff, (int(seed) >> 32) & 0xffffffff], U64))


def uniforms(words):
    """(u1 in (0, 1], u2 in [0, 1)) of the word pairs (0, 1) and (2, 3), float64 -- both exact in float32 too."""
    w = np.asarray(words, U32).reshape(words.shape[:-1] + (2, 2))
    u1 = ((w[..., 0] >> U32(8)).astype(F64) + 1.0) * 2.0 ** -24
    u2 = (w[..., 1] >> U32(8)).astype(F64) * 2.0 ** -24
    return u1, u2


def normals64(words):
    """float64 [..., 4]: lanes (0, 1) the Box-Muller pair of words (0, 1), lanes (2, 3) of words (2, 3)."""
    u1, u2 = uniforms(words)
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * np.pi * u2
    return np.stack((rad * np.cos(ang), rad * np.sin(ang)), axis=-1).reshape(words.shape)


def normals32(words):
    """The same in float32 with every operation rounded, as the kernel states it (2 pi = 6.2831855f)."""
    u1, u2 = (u.astype(F32) for u in uniforms(words))
    rad = np.sqrt(F32(-2.0) * np.log(u1))
    ang = F32(2.0 * np.pi) * u2
    out = np.stack((rad * np.cos(ang), rad * np.sin(ang)), axis=-1).reshape(words.shape)
    assert out.dtype == F32
    return out


def _as_sample(z, k):
    """normals [N, calls, 4] -> [k - 1, N, 3]: number q = 3 (t - 1) + a is lane q % 4 of call q / 4."""
    n = z.shape[0]
    return np.ascontiguousarray(z.reshape(n, -1)[:, :3 * (k - 1)].reshape(n, k - 1, 3).transpose(1, 0, 2))


def noise_sample64(seed, stream, n, k, noise_std):
    """float64 [k - 1, N, 3]: n_t = z * (float)(noise_std / sqrt(k - 1))."""
    return _as_sample(normals64(draw_words(seed, stream, n, k)), k) * F64(F32(noise_std / np.sqrt(k - 1)))


def noise_sample32(seed, stream, n, k, noise_std):
    """float32: what the kernel's draw is, up to the last bits of its logf / sincosf."""
    return _as_sample(normals32(draw_words(seed, stream, n, k)), k) * F32(noise_std / np.sqrt(k - 1))


def noise_sequence64(sample):
    """[k, N, 3] float64: the double running sum with the zero first frame."""
    seq = np.cumsum(np.cumsum(np.asarray(sample, F64), axis=0), axis=0)
    return np.concatenate((np.zeros((1,) + seq.shape[1:], F64), seq), axis=0)


def running_sum_weights(k):
    """[k]: seq_t = sum_u (t - u + 1) n_u over u = 1..t -- the sum of the weights of frame t is t (t + 1) / 2."""
    return np.array([t * (t + 1) // 2 for t in range(k)], F64)


def _f32_draw_err(calls=250000):
    """Worst distance of the float32 restatement of a normal from the float64 one on the same integers, in units of sigma."""
    w = draw_words(0x5eed, 9, calls, 2)[:, 0, :]            # k = 2: one call per particle, 4 normals
    return float(np.abs(normals32(w).astype(F64) - normals64(w)).max())


F32_DRAW_ERR = _f32_draw_err()
