"""The CLI's side of the feature buffers, without a GPU: the help text and the refusals of --features and --feature-samples,
each by name, with exit status 2 and before anything is loaded or written."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def run(*argv):
    return subprocess.run([str(EXE), *argv], capture_output=True, text=True)


def test_cli_features_help():
    assert EXE.exists(), "build the CLI with `make`"
    r = run("--help")
    assert r.returncode == 0
    for flag in ("--features <prefix>", "--feature-samples <n>"):
        assert flag in r.stdout, flag
    for name in (".albedo.pfm", ".normal.pfm", ".depth.pfm", ".coverage.pfm"):
        assert name in r.stdout, name
    assert "primary rays per pixel, 1 to 65536 [default: --samples, at most 8]" in r.stdout
    assert "Cannot be combined with --gpus > 1" in r.stdout


def test_cli_features_refusals(tmp_path):
    out = ["-t", str(tmp_path / "x.png")]
    prefix = str(tmp_path / "f")
    cases = {
        "an empty prefix": (["--features", ""], "--features"),
        "an empty prefix, = form": (["--features="], "--features"),
        "no prefix at all": (["--features"], "--features"),
        "0 samples": (["--features", prefix, "--feature-samples", "0"], "--feature-samples"),
        "65537 samples": (["--features", prefix, "--feature-samples", "65537"], "--feature-samples"),
        "negative samples": (["--features", prefix, "--feature-samples", "-3"], "--feature-samples"),
        "samples that are no number": (["--features", prefix, "--feature-samples", "x"], "--feature-samples"),
        "samples without --features": (["--feature-samples", "4"], "--feature-samples"),
        "two GPUs": (["--features", prefix, "--gpus", "2"], "--gpus > 1"),
    }
    for what, (argv, name) in cases.items():
        r = run(*argv, *(out if what != "no prefix at all" else []))
        assert r.returncode == 2, (what, r.returncode, r.stderr)
        assert r.stderr.startswith("error: ") and name in r.stderr, (what, r.stderr)
        assert not list(tmp_path.iterdir()), what  # neither the image nor a feature file
    r = run("--feature-samples", "4", *out)
    assert "needs '--features'" in r.stderr
    r = run("--features", prefix, "--gpus", "2", *out)
    assert "'--features' cannot be combined with '--gpus > 1'" in r.stderr
