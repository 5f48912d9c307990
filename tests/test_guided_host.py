"""The guided denoiser's command line without a GPU: the help text, and every refusal by name with exit status 2 before
anything is loaded or written. And that the new kernel file is hashed with the others and shares no code with kernels.hip."""
import re
import subprocess
from pathlib import Path

from rbrt_amd import srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def test_the_kernel_source_is_hashed_and_keeps_to_itself():
    assert "rbrt_amd/csrc/guided.hip" in srchash.KERNEL_SOURCES
    src = (ROOT / "rbrt_amd" / "csrc" / "guided.hip").read_text()
    assert "#pragma clang fp contract(off)" in src and "kernels.hip" not in re.sub(r"//[^\n]*", "", src)


def test_cli_guided_help():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise-guided  ", "--guided-levels <l>", "--guided-colour <k>", "--guided-normal <k>", "--guided-depth <k>",
                 "--guided-albedo <k>", "--guided-no-demodulation  "):
        assert flag in r.stdout, flag
    for text in ("1 to 6; each doubles its reach [default: 5]", "above 0 [default: 2]", "above 0 [default: 0.35]", "above 0 [default: 0.05]",
                 "above 0 [default: 0.1]", "--samples must be at least 2", "--feature-samples apply"):
        assert text in r.stdout, text
    # --denoise keeps its text
    assert "--denoise                    filter the image: a dual-buffer non-local-means filter" in r.stdout


def test_cli_guided_refusals(tmp_path):
    out = ["-t", str(tmp_path / "x.png")]

    def refused(argv, *names):
        r = subprocess.run([str(EXE), *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and all(n in r.stderr for n in names), (argv, r.returncode, r.stderr)
        assert not list(tmp_path.iterdir()), argv  # nothing written

    G = ["--denoise-guided", "-s", "8"]
    refused([*G, "--denoise"], "--denoise-guided", "'--denoise'")
    refused([*G, "--gpus", "2"], "--denoise-guided", "--gpus > 1")
    refused([*G, "--adaptive", "0.05", "--gpus", "2"], "--gpus > 1")
    refused([*G, "--checkpoint", str(tmp_path / "c.bin")], "--denoise-guided", "--checkpoint")
    refused([*G, "--pass-samples", "4"], "--denoise-guided", "--pass-samples")
    refused([*G, "--features", str(tmp_path / "f"), "--gpus", "2"], "--gpus > 1")
    # fewer than two samples: a half would be empty
    refused(["--denoise-guided", "-s", "1"], "--denoise-guided", "--samples")
    refused(["--denoise-guided", "-s", "0"], "--denoise-guided", "--samples")
    # the flags take no value
    refused(["--denoise-guided=1", "-s", "8"], "--denoise-guided", "takes no value")
    refused([*G, "--guided-no-demodulation=1"], "--guided-no-demodulation", "takes no value")
    # values out of range
    for argv in (["--guided-levels", "0"], ["--guided-levels", "7"], ["--guided-levels", "-1"], ["--guided-levels", "x"], ["--guided-levels=2.5"]):
        refused([*G, *argv], "--guided-levels")
    for name in ("--guided-colour", "--guided-normal", "--guided-depth", "--guided-albedo"):
        for v in ("0", "-0.5", "nan", "inf", "x", ""):
            refused([*G, f"{name}={v}"], name)
    refused([*G, "--feature-samples", "0"], "--feature-samples")
    refused([*G, "--feature-samples", "65537"], "--feature-samples")
    # the options without --denoise-guided
    for argv, name in ((["--guided-levels", "3"], "--guided-levels"), (["--guided-colour", "1"], "--guided-colour"),
                       (["--guided-normal", "1"], "--guided-normal"), (["--guided-depth", "1"], "--guided-depth"),
                       (["--guided-albedo", "1"], "--guided-albedo"), (["--guided-no-demodulation"], "--guided-no-demodulation")):
        refused(["-s", "8", *argv], name, "needs '--denoise-guided'")
        refused(["--denoise", "-s", "8", *argv], name, "needs '--denoise-guided'")
    for flag in ("--guided-levels", "--guided-colour", "--guided-normal", "--guided-depth", "--guided-albedo"):  # a value is required
        assert subprocess.run([str(EXE), "--denoise-guided", flag], capture_output=True, text=True).returncode == 2
    # what --denoise refuses by its own name stays as it was
    refused(["-s", "8", "--noisy", str(tmp_path / "n.png")], "'--noisy' needs '--denoise'")
    refused(["-s", "8", "--feature-samples", "4"], "'--feature-samples' needs '--features'")
