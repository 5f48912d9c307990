"""The glare stage on the host side, without a GPU: the command line's options and refusals, and the kernel source in the
source hash. What the CLI writes with them is compared with the restatement on the GPU (test_glare_gpu.py)."""
from __future__ import annotations

import subprocess
from pathlib import Path

import pytest

from rbrt_amd import srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
OPTIONS = ("--glare", "--glare-threshold", "--glare-levels", "--glare-spread")


def test_help_lists_the_options():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--glare <intensity>", "--glare-threshold <t>", "--glare-levels <l>", "--glare-spread <s>"):
        assert opt in r.stdout, opt
    head = (ROOT / "rbrt_amd" / "host" / "main.cpp").read_text().split("#include")[0]
    for opt in OPTIONS:
        assert opt in head, opt


@pytest.mark.parametrize("argv,names", [
    (["--glare", "bright"], ["--glare", "bright"]),
    (["--glare", "0"], ["--glare"]),
    (["--glare", "-0.1"], ["--glare"]),
    (["--glare", "1.5"], ["--glare"]),
    (["--glare", "nan"], ["--glare"]),
    (["--glare", "inf"], ["--glare"]),
    (["--glare"], ["--glare"]),
    (["--glare", "0.1", "--glare-threshold", "-1"], ["--glare-threshold"]),
    (["--glare", "0.1", "--glare-threshold", "nan"], ["--glare-threshold"]),
    (["--glare", "0.1", "--glare-threshold", "inf"], ["--glare-threshold"]),
    (["--glare", "0.1", "--glare-levels", "0"], ["--glare-levels", "1 to 8"]),
    (["--glare", "0.1", "--glare-levels", "9"], ["--glare-levels", "1 to 8"]),
    (["--glare", "0.1", "--glare-levels", "three"], ["--glare-levels"]),
    (["--glare", "0.1", "--glare-levels", "-1"], ["--glare-levels"]),
    (["--glare", "0.1", "--glare-spread", "-0.5"], ["--glare-spread"]),
    (["--glare", "0.1", "--glare-spread", "nan"], ["--glare-spread"]),
    (["--glare", "0.1", "--glare-spread", "inf"], ["--glare-spread"]),
    (["--glare-threshold", "2"], ["--glare-threshold", "needs '--glare'"]),
    (["--glare-levels", "3"], ["--glare-levels", "needs '--glare'"]),
    (["--glare-spread", "0.5"], ["--glare-spread", "needs '--glare'"]),
])
def test_parse_errors(tmp_path, argv, names):
    """Refused by name, with exit code 2, before a scene is read or a device touched: nothing is written."""
    out = tmp_path / "x.ppm"
    r = subprocess.run([str(EXE), *argv, "-t", str(out), "-c", str(tmp_path / "no_such_scene.yaml")], capture_output=True, text=True)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert r.stderr.startswith("error:")
    for name in names:
        assert name in r.stderr, (name, r.stderr)
    assert not out.exists()


def test_good_options_get_as_far_as_the_scene(tmp_path):
    """The accepted forms, the ends of the ranges included: the first complaint is about the scene file that is not there."""
    for argv in (["--glare", "1"], ["--glare", "1e-3", "--glare-threshold", "0", "--glare-levels", "8", "--glare-spread", "0"],
                 ["--glare", "0.25", "--glare-levels", "1", "--glare-spread", "2.5", "--glare-threshold", "1e6"]):
        r = subprocess.run([str(EXE), *argv, "-t", str(tmp_path / "x.ppm"), "-c", str(tmp_path / "no_such_scene.yaml")],
                           capture_output=True, text=True)
        assert r.returncode != 0 and "no_such_scene.yaml" in r.stderr and "--glare" not in r.stderr, (argv, r.stderr)


def test_the_kernel_source_is_in_the_source_hash():
    assert "rbrt_amd/csrc/glare.hip" in srchash.KERNEL_SOURCES
    assert (ROOT / "rbrt_amd" / "csrc" / "glare.hip").exists()
    mk = (ROOT / "Makefile").read_text()
    assert mk.count("$(CSRC)/glare.hip") >= 4  # both library rules: prerequisites and command line
