"""bench.py --dump-outputs (no GPU): what is written for a frame within the size limit and for one beyond it, and the
arguments it is refused with."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_a_frame_within_the_limit_is_written_whole(tmp_path):
    img = np.random.default_rng(3).random((7, 5, 3), dtype=np.float32)
    shapes = bench.dump_outputs(tmp_path / "d", np, img)
    assert shapes == {"radiance": [7, 5, 3]}
    got = np.load(tmp_path / "d" / "radiance.npy")
    assert got.dtype == np.float32 and np.array_equal(got, img)


def test_a_larger_frame_is_sampled_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 40 * 20)  # 40 pixels of 3 float32 + one float64 index each
    img = np.random.default_rng(4).random((16, 16, 3), dtype=np.float32)
    a = bench.dump_outputs(tmp_path / "a", np, img)
    b = bench.dump_outputs(tmp_path / "b", np, img)
    assert a == b == {"radiance_sample": [40, 3], "radiance_sample_index": [40]}
    total = 0
    for name in a:
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype in (np.float32, np.float64) and np.array_equal(x, y)
        total += x.nbytes
    assert total <= bench.DUMP_LIMIT_BYTES
    idx = np.load(tmp_path / "a" / "radiance_sample_index.npy").astype(np.int64)
    assert len(set(idx.tolist())) == 40 and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "radiance_sample.npy"), img.reshape(-1, 3)[idx])


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--dump-outputs", "d", "--emulate-all", "2"]])
def test_bench_refuses_arguments_it_cannot_honour(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "error:" in r.stderr
