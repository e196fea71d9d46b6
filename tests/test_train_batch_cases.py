"""CPU: the restated draw of tests/train_batch_cases.py against the published Philox vectors and the normal distribution, the
regimes its cases were built for, and the oracle's noisy path -- the yardstick of tests/test_gpu_train_batch.py -- against the
reference's own outputs in fixture G9."""
import numpy as np
import pytest

from conftest import BOUNDS, CART, CTRL, MAT, STATS
from oracle import epd_oracle as orc
import train_batch_cases as tc

# Random123's kat_vectors for philox4x32 at 10 rounds: (counter, key, output)
PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", PHILOX_KAT)
def test_philox_known_answers(counter, key, want):
    got = tc.philox4x32_10(np.array(counter, np.uint64), np.array(key, np.uint64))
    assert got.dtype == np.uint32 and [int(v) for v in got] == list(want)


def test_philox_is_vectorised_over_counters_and_words_follow_the_header():
    w = tc.draw_words(seed=(7 << 32) | 5, stream=(3 << 32) | 9, n=4, k=6)
    assert w.shape == (4, 4, 4)                              # 15 normals: four calls of four
    for i in range(4):
        for j in range(4):
            one = tc.philox4x32_10(np.array([i, j, 9, 3], np.uint64), np.array([5, 7], np.uint64))
            assert np.array_equal(w[i, j], one)
    assert tc.draw_words(1, 0, 3, 2).shape == (3, 1, 4)      # k = 2: three normals, one call


def test_restated_draw_is_standard_normal():
    c = tc.CASES["zeros"]
    words = tc.draw_words(11, 0, c.n, c.k)
    u1, _ = tc.uniforms(words)
    assert u1.min() > 0.0 and u1.max() <= 1.0
    z = tc.normals64(words).reshape(c.n, -1)[:, :3 * (c.k - 1)]
    n = z.size
    assert n == 4096 * 15
    assert abs(z.mean()) <= 6.0 / np.sqrt(n)
    assert abs(z.var() - 1.0) <= 6.0 * np.sqrt(2.0 / n)
    # the smallest u1 there is, 2^-24, still has a logarithm: the largest normal is sqrt(48 ln 2)
    top = tc.normals64(np.array([[0, 0, 255, 0]], np.uint32))
    assert np.isfinite(top).all() and abs(top[0, 0] - np.sqrt(48 * np.log(2.0))) < 1e-12


def test_float32_draw_error_is_what_the_gpu_test_scales_by():
    assert 5e-7 < tc.F32_DRAW_ERR < 5e-6, tc.F32_DRAW_ERR
    s64 = tc.noise_sample64(3, 1, 50, 6, tc.NOISE_STD)
    s32 = tc.noise_sample32(3, 1, 50, 6, tc.NOISE_STD)
    assert s32.dtype == np.float32 and s64.shape == s32.shape == (5, 50, 3)
    scale = tc.NOISE_STD / np.sqrt(5)
    assert np.abs(s32 - s64).max() <= 2 * tc.F32_DRAW_ERR * scale
    seq = tc.noise_sequence64(s64)
    assert not seq[0].any() and np.allclose(seq[2], 2 * s64[0] + s64[1], rtol=1e-14, atol=0)
    assert list(tc.running_sum_weights(6)) == [0, 1, 3, 6, 10, 15]


@pytest.mark.parametrize("name", tc.ALL_CASES)
def test_case_is_in_its_regime(name):
    c = tc.CASES[name]
    recs = c.recordings()
    assert all(r.shape == (c.T, c.n, tc.REC_DIM) and r.dtype == np.float32 for r in recs)
    assert c.B <= tc.GM_TRAIN_BATCH_MAX and all(t + c.k < c.T for _, t in c.samples)
    for rec in recs:
        rigid = rec[0, :, tc.MAT] == 1
        assert 0 < rigid.sum() < c.n and ((rec[:, :, tc.MAT] == 0) | (rec[:, :, tc.MAT] == 1)).all()
    wins = c.windows()
    assert all(o.shape == (c.k, c.n, c.D) and nx.shape == (c.n, 3) for o, nx in wins)
    if not c.zero:
        assert all(np.abs(np.diff(r[:, :, tc.CART], axis=0)).max(axis=-1).min() > 0 for r in recs)   # every row moves, every frame
    if c.control and not c.zero:
        for o, _ in wins:
            rigid = o[0, :, tc.MAT] == 1
            assert o[:, rigid][:, :, tc.CTRL].any() and not o[:, ~rigid][:, :, tc.CTRL].any()
    if name == "three97":
        assert c.B * c.n == 291 > 256 and c.n % 64
        assert {r for r, _ in c.samples} == {0, 1}
        (r0, t0), (r1, t1) = c.samples[0], c.samples[1]
        assert r0 == r1 and 0 < t1 - t0 < c.k                                                 # overlapping windows of one recording
    if name == "k2":
        assert c.k == 2 and c.F == 13
    if name == "noctl":
        assert c.D == 5 and not c.control
    if name == "zeros":
        assert not recs[0][:, :, tc.CART].any() and c.n == 4096
    if name == "cap5":
        # under the restated noise the cap binds: nodes with more than 5 neighbours inside the radius
        ns = [tc.noise_sample32(1, b, c.n, c.k, tc.NOISE_STD) for b in range(c.B)]
        last = tc.noisy_windows(c, ns)[:, -1][:, :, tc.CART]
        for p in last:
            d2 = ((p[:, None, :].astype(np.float64) - p[None, :, :].astype(np.float64)) ** 2).sum(-1)
            assert ((d2 <= tc.R * tc.R).sum(1) > c.max_nb).sum() > c.n // 2


def test_oracle_noisy_path_is_the_references(golden):
    """Fixture G9 holds the reference's random_walk_noise / _process_noisy outputs for its own Normal draw: the oracle's noisy
    path reproduces them at the bars of tests/test_gpu_dataset.py::test_noise_path_golden."""
    g = golden("g9_dataset.npz")
    obs, sample = g["noise.obs"], g["noise.sample"]
    seq = orc.random_walk_noise(obs[:, :, 2:5], float(g["noise.std"]), sample)
    np.testing.assert_allclose(seq, g["noise.sequence"], rtol=1e-6, atol=1e-9)
    nodes, ea, s, r, acc = orc.process_noisy(obs, g["noise.tgt"], sample, STATS, BOUNDS, 0.015, CART, MAT, CTRL)
    np.testing.assert_array_equal(s, g["noise.senders"])
    np.testing.assert_array_equal(r, g["noise.receivers"])
    np.testing.assert_allclose(nodes, g["noise.nodes"], rtol=2e-6, atol=3e-5)
    np.testing.assert_allclose(ea, g["noise.edge_attr"], rtol=2e-6, atol=4e-6)
    np.testing.assert_allclose(acc, g["noise.acc"], rtol=1e-5, atol=6e-4)
    # and the windows helper of the cases is that path's obs + noise
    c = tc.CASES["k2"]
    ns = [tc.noise_sample32(2, b, c.n, c.k, tc.NOISE_STD) for b in range(c.B)]
    w = tc.noisy_windows(c, ns)
    clean = c.windows()
    assert np.array_equal(w[1][0], clean[1][0][0]) and np.array_equal(w[1][1][:, tc.CART], clean[1][0][1][:, tc.CART] + ns[1][0])
