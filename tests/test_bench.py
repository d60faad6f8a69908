"""bench.py's contract with whoever runs it: --dump-outputs writes float32 / float64 .npy files within the byte budget
(a fixed row sample of a larger array), and a plain run prints the headline line only, with --steps timed steps,
leaving everything that takes runs of its own to --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("phase_ms_per_step", "kernel_us", "roofline", "roofline_next_kernels", "solve_end_to_end")


def test_dump_outputs_types_and_values(tmp_path):
    f64 = np.linspace(0.0, 1.0, 30).reshape(10, 3)
    f32 = np.arange(7, dtype=np.float32) / 3
    i32 = np.array([0, -5, 2 ** 31 - 1], dtype=np.int32)
    u8 = np.array([0, 1, 255], dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "d"), {"a": f64, "b": f32, "c": i32, "d": u8, "loss": [2.5]})
    got = {n: np.load(tmp_path / "d" / (n + ".npy")) for n in ("a", "b", "c", "d", "loss")}
    assert got["a"].dtype == np.float64 and np.array_equal(got["a"], f64)
    assert got["b"].dtype == np.float32 and np.array_equal(got["b"], f32)
    assert got["c"].dtype == np.float64 and np.array_equal(got["c"], i32.astype(np.float64))
    assert got["d"].dtype == np.float64 and np.array_equal(got["d"], [0.0, 1.0, 255.0])
    assert got["loss"].shape == (1,) and got["loss"][0] == 2.5


def test_dump_outputs_samples_within_budget(tmp_path, monkeypatch):
    assert bench.DUMP_BUDGET_BYTES == 64 * 2 ** 20
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096)
    big = np.arange(3000, dtype=np.float64).reshape(1000, 3)   # 24000 bytes: over its 2048-byte share
    small = np.arange(12, dtype=np.float32)
    for d in ("x", "y"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert np.array_equal(x, y)                                # the same rows in every run
    assert x.shape == (2048 // 24, 3)
    rows = (x[:, 0] / 3).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(x, big[rows])  # whole rows, in order, no repeats
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), small)
    assert sum(np.load(tmp_path / "x" / f).nbytes for f in os.listdir(tmp_path / "x")) <= 4096


def _bench(*extra):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--config", "1", "--deterministic", *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120, cwd=REPO)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    """One plain run with --dump-outputs, shared: (result line, dump directory)."""
    a = str(tmp_path_factory.mktemp("bench") / "a")
    return _bench("--dump-outputs", a), a


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only(plain_run):
    d, a = plain_run
    for k in HEADLINE:
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and len(d["pcg_iters"]) == 3  # --steps is the number of timed steps
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 1.0) < 1e-2
    assert d["unit"] == "LM it/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    for k in FULL_ONLY:
        assert k not in d, k
    assert d["cpu_baseline"] is None
    assert sorted(os.listdir(a)) == ["cams.npy", "loss.npy", "points.npy"]
    assert np.load(os.path.join(a, "cams.npy")).shape[0] == 20
    assert np.load(os.path.join(a, "points.npy")).shape == (2000, 3)
    assert np.load(os.path.join(a, "loss.npy")).shape == (1,)


@pytest.mark.gpu
def test_dumps_repeat_from_run_to_run(plain_run, tmp_path):
    _, a = plain_run
    b = str(tmp_path / "b")
    _bench("--dump-outputs", b)
    for f in os.listdir(a):
        x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f))
        assert x.dtype == np.float64 and np.all(np.isfinite(x))
        assert np.array_equal(x, y), f  # deterministic mode: the same inputs give the same bits


@pytest.mark.gpu
def test_full_run_adds_the_rest():
    d = _bench("--full", "--no-cpu")
    for k in HEADLINE + FULL_ONLY + ("final_rmse_px",):
        assert k in d, k
    assert d["steps"] == 3 and len(d["pcg_iters"]) == 3
