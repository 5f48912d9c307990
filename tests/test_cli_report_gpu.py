"""The command line's `--report -` line, pinned as text: key order, separators, number formats and every value that is not a
measured time, for a set of small runs that emits every conditional block of the report at least once.
tests/golden/cli_reports.json has the expected lines; `python tests/test_cli_report_gpu.py --record` writes that file from the
binary that is built, on a GPU (the test never does).

Measured keys are masked before the comparison: those that end in _s or _ms (mray_samples_per_s is one) and the nested "ms".
Every run is one short process in an empty directory with a copy of a mesh-free scene, so every file name in a report is relative."""
import json
import re
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
GOLDEN = Path(__file__).resolve().parent / "golden" / "cli_reports.json"
SIZE = ["--width", "32", "--height", "24", "-s", "4"]
PLAIN = ["-c", "checker.yaml", *SIZE]
MEASURED = re.compile(r'"(\w+_s|\w+_ms|ms)": [-+.0-9e]+')

# (the first run writes the radiance that the two comparisons read)
RUNS = {
    "plain": [*PLAIN, "--radiance", "ref.pfm"],
    "adaptive": [*PLAIN, "--adaptive", "0.05", "--min-samples", "2", "--adaptive-step", "1", "--sample-map", "m.png"],
    "denoise": [*PLAIN, "--denoise", "--denoise-radius", "2", "--noisy", "n.png"],
    "denoise-guided, features": [*PLAIN, "--denoise-guided", "--guided-levels", "2", "--features", "f", "--feature-samples", "2"],
    "frames, shutter": [*PLAIN, "--frames", "2", "--camera-step", "0.1,0,0", "--shutter", "0.5", "--temporal-depth", "-0", "--history-map", "h.png"],
    "shutter-travel, compare": [*PLAIN, "--shutter-travel", "0.2,0,-0.1", "--compare", "ref.pfm", "--compare-epsilon", "0.02", "--error-map", "e.pfm"],
    "the scene file's shutter travel": ["-c", "shutter.yaml", *SIZE],
    "upscale": [*PLAIN, "--upscale", "2", "--upscale-depth", "0.2"],
    "despike": [*PLAIN, "--despike", "--despike-threshold", "1.5", "--spike-map", "k.png"],
    "glare, tonemap": [*PLAIN, "--glare", "0.3", "--glare-levels", "3", "--tonemap", "reinhard", "--white", "2", "--exposure", "auto"],
    "compare with itself": [*PLAIN, "--compare", "ref.pfm", "--ssim-map", "s.png"],  # (a PSNR that is not finite: a string)
    "environment": [*PLAIN, "--environment", "env.pfm", "--environment-resolution", "16", "--seed", "7", "--report=-"],
}


def masked(line):
    return MEASURED.sub(lambda m: f'"{m.group(1)}": "*"', line)


def workdir(d):
    shutil.copy(ROOT / "scenes" / "checker" / "checker_ground.yaml", d / "checker.yaml")
    shutil.copy(ROOT / "scenes" / "shutter" / "shutter_spheres.yaml", d / "shutter.yaml")
    sky = [c for row in range(4) for col in range(8) for c in (0.2 + 0.1 * row, 0.3 + 0.05 * col, 1.0 - 0.1 * row)]
    (d / "env.pfm").write_bytes(b"PF\n8 4\n-1.0\n" + struct.pack("<96f", *sky))
    return d


def report(d, name):
    """The masked report line of one run in the directory d."""
    r = subprocess.run([str(EXE), *RUNS[name], "-t", "o.png", "--report", "-"], cwd=d, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (name, r.returncode, r.stderr)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1 and r.stdout.endswith(lines[0] + "\n"), (name, r.stdout)
    json.loads(lines[0])
    return masked(lines[0])


@pytest.fixture(scope="module")
def reports(tmp_path_factory):
    d = workdir(tmp_path_factory.mktemp("cli_reports"))
    return d, {"plain": report(d, "plain")}


@pytest.mark.parametrize("name", list(RUNS))
def test_the_report_line_is_what_was_recorded(reports, name):
    d, done = reports
    got = done[name] if name in done else report(d, name)
    assert got == json.loads(GOLDEN.read_text())[name]


def test_the_runs_emit_every_block_of_the_report():
    keys = {k for line in json.loads(GOLDEN.read_text()).values() for k in json.loads(line)}
    for k in ("adaptive_threshold", "active_tiles_per_round", "environment_file", "denoise_ms", "guided_ms", "temporal_ms", "camera_step",
              "shutter_travel", "upsample_ms", "spikes_b", "glare_ms", "tonemap_ms", "compare_psnr_db", "features", "mray_samples_per_s"):
        assert k in keys, k


if __name__ == "__main__":
    import tempfile

    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_cli_report_gpu.py --record")
    with tempfile.TemporaryDirectory() as tmp:
        recorded = {name: report(workdir(Path(tmp)) if name == "plain" else Path(tmp), name) for name in RUNS}
    GOLDEN.write_text(json.dumps(recorded, indent=1) + "\n")
    print(f"recorded {len(recorded)} report lines in {GOLDEN}")
