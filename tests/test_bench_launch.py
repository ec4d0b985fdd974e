"""bench.py's launcher contract: `python bench.py --gpus N` must really run N ranks.

CPU part: with PFMI_BENCH_LAUNCH_ONLY=1 the ranks only join a `gloo` world and count themselves, which exercises the
self-launch path (no WORLD_SIZE in the environment -> bench.py re-executes itself under torch.distributed.run on
127.0.0.1) and the WORLD_SIZE / --gpus consistency check.  The GPU part (tests/test_gpu_*.py::test_bench_*) runs the
real step through RCCL.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                          timeout=timeout)


def _json_line(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, out
    return json.loads(lines[-1])


def test_gpus_2_self_launches_two_ranks():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0"], {"PFMI_BENCH_LAUNCH_ONLY": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    line = _json_line(r.stdout)
    assert line["n_gpus"] == 2 and line["world_size"] == 2 and line["ranks_in_collective"] == 2


def test_full_reaches_every_rank():
    r = _run(["--gpus", "2", "--steps", "1", "--warmup", "0", "--full"], {"PFMI_BENCH_LAUNCH_ONLY": "1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert _json_line(r.stdout)["ranks_in_collective"] == 2


def test_world_size_must_match_gpus():
    r = _run(["--gpus", "2"], {"PFMI_BENCH_LAUNCH_ONLY": "1", "WORLD_SIZE": "1", "RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    r = _run(["--gpus", "1"], {"PFMI_BENCH_LAUNCH_ONLY": "1", "WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode != 0 and "--gpus 1" in r.stderr


def test_steps_must_be_positive():
    r = _run(["--steps", "0"], {"PFMI_BENCH_LAUNCH_ONLY": "1"})
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr


def test_dump_outputs_is_float64_deterministic_and_at_most_64_mb(tmp_path):
    """--dump-outputs writes every array as float64; over 64 MB the draws are cut to the same seeded sample of their columns every run."""
    import numpy as np
    import bench
    draws = np.arange(3000 * 4000, dtype=np.float64).reshape(3000, 4000)      # 96 MB
    arrays = {"draws": draws, "elbo": np.array([np.nan, 1.5, -2.0]), "best_iter": np.array([2, 7], dtype=np.int64), "pareto_k": 0.7}
    for run in ("a", "b"):
        bench._dump_outputs(str(tmp_path / run), arrays)
    got = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    again = {f[:-4]: np.load(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")}
    assert sorted(got) == ["best_iter", "draws", "draws_sample_index", "elbo", "pareto_k"] == sorted(again)
    assert all(a.dtype == np.float64 and np.array_equal(a, again[k], equal_nan=True) for k, a in got.items())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    sel = got["draws_sample_index"].astype(np.int64)
    assert len(sel) > 2000 and np.all(np.diff(sel) > 0) and np.array_equal(got["draws"], draws[:, sel])
    np.testing.assert_array_equal(got["elbo"], arrays["elbo"])
    assert got["best_iter"].tolist() == [2.0, 7.0] and got["pareto_k"].tolist() == [0.7]
    tab = bench._elbo_outputs(np.array([np.nan, -3.0, -2.5, np.nan, np.nan, -1.0]), np.array([np.nan, 0.1, 0.2, np.nan, np.nan, 0.3]))
    assert tab["elbo_fit_index"].tolist() == [1, 2, 5] and tab["elbo"].tolist() == [-3.0, -2.5, -1.0] and tab["elbo_se"].tolist() == [0.1, 0.2, 0.3]
    small = {"draws": draws[:, :10], "idx": np.arange(10)}
    bench._dump_outputs(str(tmp_path / "c"), small)
    assert sorted(os.listdir(tmp_path / "c")) == ["draws.npy", "idx.npy"]
    np.testing.assert_array_equal(np.load(tmp_path / "c" / "draws.npy"), draws[:, :10])
