"""bench.py --dump-outputs: what the timed path computed in its last step, written so that two builds of the library can be
compared output for output on the same seeded inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT


def test_dump_of_the_default_workload_size_is_whole(tmp_path):
    import bench
    rng = np.random.default_rng(0)
    state = rng.random((6, 100000, 8), dtype=np.float32)   # the default workload's window: 19.2 MB
    losses = rng.random(64)
    bench.dump_outputs(str(tmp_path), {"state": state, "losses": losses})
    assert sorted(os.listdir(tmp_path)) == ["losses.npy", "state.npy"]
    s, l = np.load(tmp_path / "state.npy"), np.load(tmp_path / "losses.npy")
    assert s.dtype == np.float32 and l.dtype == np.float64
    np.testing.assert_array_equal(s, state)
    np.testing.assert_array_equal(l, losses)


def test_dump_over_the_cap_is_a_fixed_sample_of_rows(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    state = rng.random((6, 400000, 8), dtype=np.float32)   # 76.8 MB: over the 64 MB cap
    gathered = rng.random((2, 3), dtype=np.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"state": state, "gathered_results": gathered})
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["gathered_results.npy", "state.npy", "state_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_LIMIT_BYTES == 64 << 20
    rows = np.load(tmp_path / "a" / "state_rows.npy")
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all() and len(rows) > 0.8 * state.shape[1]
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "state.npy"), state[:, rows.astype(np.int64)])
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "gathered_results.npy"), gathered)   # small arrays stay whole
    for f in files:   # the same rows in every run
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))


@pytest.mark.gpu
def test_bench_dumps_the_state_its_timed_steps_computed(tmp_path):
    """`bench.py --workload c2 --steps 3 --warmup 1 --dump-outputs DIR` as a fresh child process: the JSON line reports the three
    timed steps, and DIR/state.npy is the state window that the same seeded inputs reach in this process after one warm-up and
    three timed rollout steps."""
    import bench
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    out = tmp_path / "dump"
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GM_BENCH_REHEARSE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--steps", "3", "--warmup", "1",
                        "--no-extra", "--no-cpu-baseline", "--dump-outputs", str(out)], env=env, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace")
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert sorted(os.listdir(out)) == ["state.npy"]
    state = np.load(out / "state.npy")

    _, eng, obs, traj, *_ = bench.build_engine(bench.WORKLOADS["c2"], dev, 0, 1, "auto", 4)
    with torch.no_grad():
        eng.run(obs, traj[:1].contiguous(), 1)
        after_warmup = obs.cpu().numpy()
        eng.run(obs, traj[1:].contiguous(), 3)
    eng.status()
    assert state.dtype == np.float32 and state.shape == tuple(obs.shape) and np.isfinite(state).all()
    # Particles move ~1e-6 per step and the kernels sum in a fixed order: a bound of 1e-7 tells one step more or less apart.
    assert np.abs(state - after_warmup).max() > 1e-7
    np.testing.assert_allclose(state, obs.cpu().numpy(), rtol=0, atol=1e-7)


@pytest.mark.gpu
def test_plain_bench_run_is_lean_and_full_adds_the_rest(tmp_path):
    """A plain run prints the headline alone; `--full` adds the roofline and breakdown of the instrumented pass after the timed
    steps.  Both at the C2 size as fresh child processes, without the CPU baseline (which only `--full` would run anyway)."""
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GM_BENCH_REHEARSE"):
        env.pop(k, None)
    recs = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--no-cpu-baseline"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c2", "--steps", "3", "--warmup", "1"] + extra,
                           env=env, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stdout.decode(errors="replace") + r.stderr.decode(errors="replace")
        lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
        assert len(lines) == 1
        recs[mode] = json.loads(lines[0])
    for rec in recs.values():
        assert rec["unit"] == "rollout steps/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
        assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["value"] > 0 and rec["ms_per_step"] > 0
        assert rec["metric"] == "rollout steps/sec (N particles, 10 MP steps, hidden=128)"
    assert not {"roofline", "breakdown", "extra", "cpu_baseline"} & set(recs["plain"])
    full = recs["full"]
    assert full["roofline"]["kernel"].startswith("sys_edge_kernel") and full["roofline"]["avg_launch_ms"] > 0
    assert full["breakdown"]["profiled_steps"] == 3 and full["breakdown"]["edge_kernel_ms_per_step"] > 0
    assert "extra" not in full and "cpu_baseline" not in full   # sub-records: target workload only; baseline: skipped
