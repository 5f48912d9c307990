"""bench.py --dump-outputs (no GPU): what is written for a frame within the size limit and for one beyond it, and the
arguments it is refused with; on the GPU, that a plain run and a --full one time and dump the same frames."""
import json
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


@pytest.mark.parametrize("argv", [["--one-shot", "3"], ["--check"], ["--same-camera-steps", "-1"], ["--cpu-col-stride", "4", "--isolated-steps", "2"]])
def test_a_plain_run_refuses_the_options_of_the_full_legs(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "only a --full run" in r.stderr, r.stderr[-1000:]
    for opt in argv:
        if opt.startswith("--"):
            assert opt in r.stderr


SMALL = ["--steps", "3", "--warmup", "1", "--width", "256", "--height", "192", "--spp", "6", "--triangles", "3003"]


def _run(argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_a_plain_run_times_and_dumps_what_a_full_run_does(tmp_path):
    """A plain run leaves out every leg but the timed one; what it times and dumps is the --full run's frame, bit for bit."""
    plain = _run([*SMALL, "--dump-outputs", str(tmp_path / "plain")])
    full = _run([*SMALL, "--full", "--cpu-col-stride", "16", "--cpu-threads", "4", "--dump-outputs", str(tmp_path / "full")])
    assert plain["full"] is False and full["full"] is True
    for j in (plain, full):
        assert j["steps"] == 3 and j["warmup"] == 1 and j["value"] > 0.0 and j["ms_per_step"] > 0.0
        assert j["dumped_outputs"]["arrays"] == {"radiance": [192, 256, 3]}
    assert plain["roofline"] is None and plain["config"]["image_sha256_16"] is None and plain["ms_per_step_same_camera"] is None
    assert not {"same_camera_leg", "single_frame", "one_shot", "cpu_baseline"} & set(plain)
    assert full["roofline"]["kernel_ms"] > 0.0 and full["roofline"]["isolated_leg"]["steps"] == 8
    assert full["same_camera_leg"]["steps"] == 3 and full["single_frame"]["frames"] == 5 and full["one_shot"]["calls"] == 5
    assert full["cpu_baseline"]["value"] > 0.0 and len(full["config"]["image_sha256_16"]) == 16
    a, b = np.load(tmp_path / "plain" / "radiance.npy"), np.load(tmp_path / "full" / "radiance.npy")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
