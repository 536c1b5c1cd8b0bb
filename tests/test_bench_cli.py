"""bench.py's plain line, --full and --dump-outputs: the row sample on the CPU; -m gpu: the command line itself."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")
FULL_ONLY = ("roofline", "kernels_roofline", "kernels_ms_per_step", "serial_schedule", "native_equivalent", "deferred_diagnostic",
             "other_configs", "cpu_baseline")


def test_sample_rows_is_the_same_seeded_sample_every_time():
    small = np.ones((10, 6), dtype=np.float32)
    assert bench.sample_rows(small, 60).dtype == np.float64 and np.array_equal(bench.sample_rows(small, 60), small)
    a = np.arange(600000.0).reshape(-1, 6)
    s1, s2 = bench.sample_rows(a, 60000), bench.sample_rows(a, 60000)
    assert s1.shape == (10000, 6) and s1.dtype == np.float64
    assert np.array_equal(s1, s2)
    rows = (s1[:, 0] / 6).astype(np.int64)
    assert np.all(np.diff(rows) > 0) and np.array_equal(s1, a[rows])       # whole rows, in row order


def _fake_run(rank, n_points, s_patch):
    tile = types.SimpleNamespace(var_np1=np.random.default_rng(1).standard_normal((n_points, 6)))
    return types.SimpleNamespace(patch_spectral=lambda: np.random.default_rng(2).standard_normal((s_patch, 6)),
                                 tiles=[tile], tile_ids=[rank])


@pytest.mark.parametrize("world", [1, 4])
def test_dumped_outputs_stay_within_64_MB(tmp_path, world):
    """The headline grid's var_np1 is 8.4M points x 6 variables (400 MB): every rank's files together stay within 64 MB."""
    for rank in range(world):
        shapes = bench.dump_outputs(_fake_run(rank, 8421120, 3000000), str(tmp_path), world, rank)
        assert ("spectral_a" in shapes) == (rank == 0)
    names = ["var_np1.npy"] if world == 1 else ["var_np1_tile%d.npy" % r for r in range(world)]
    assert sorted(os.listdir(tmp_path)) == ["spectral_a.npy"] + names
    total = 0
    for f in os.listdir(tmp_path):
        a = np.load(tmp_path / f)
        assert a.dtype == np.float64 and a.shape[1] == 6
        total += a.nbytes
    assert total <= 64 << 20


def _bench(args, tmp_path, tag):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args + ["--dump-outputs", str(tmp_path / tag)],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {f: np.load(tmp_path / tag / f) for f in sorted(os.listdir(tmp_path / tag))}


@pytest.mark.gpu
def test_plain_and_full_runs_time_the_same_steps_and_dump_the_same_outputs(tmp_path):
    """Two plain runs and a --full run with the same arguments: the contract line with --steps timed steps, the --full figures
    in the --full line only, and bit-identical outputs of the last timed step from all three."""
    args = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--workload", "rlz_small"]
    a, da = _bench(args, tmp_path, "a")
    b, db = _bench(args, tmp_path, "b")
    f, df = _bench(args + ["--full", "--no-cpu-baseline"], tmp_path, "f")
    for d in (a, b, f):
        assert all(k in d for k in CONTRACT)
        assert d["steps"] == 4 and d["warmup"] == 2 and d["value"] > 0 and d["config"]["nan"] is False
        assert abs(d["ms_per_step"] - 1e3 / d["value"]) < 1e-9 * d["ms_per_step"]
    assert not any(k in a for k in FULL_ONLY) and "roofline" in f and "kernels_roofline" in f
    assert sorted(da) == ["spectral_a.npy", "var_np1.npy"]
    for name, x in da.items():
        assert x.dtype == np.float64 and np.isfinite(x).all()
        assert np.array_equal(x, db[name]) and np.array_equal(x, df[name])
