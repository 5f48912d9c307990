"""Spike removal without a GPU: every refusal of rbrt_hip_despike_halves comes back before a device is needed, the command
line's help has the new flags and refuses by name with exit status 2 before anything is loaded or written, and the new kernel
file is hashed and built with the others and shares no code with them."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

import rbrt_amd
from rbrt_amd import abi, srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def test_the_kernel_source_is_hashed_built_and_keeps_to_itself():
    assert "rbrt_amd/csrc/despike.hip" in srchash.KERNEL_SOURCES
    src = (ROOT / "rbrt_amd" / "csrc" / "despike.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in src
    assert not any(name in code for name in ("kernels.hip", "megakernel.inl", "features.inl", "guided.hip", "temporal.hip", "upsample.hip"))
    assert "asm" not in code and "__shfl" not in code  # plain C++; the counts go through ballots
    assert "__frcp" not in code and "__fdividef" not in code and "fast" not in code  # no reciprocal shortcuts
    assert code.count("__syncthreads()") == 1 and code.index("__syncthreads()") < code.index(">= W) return;")  # the early return is behind the barrier
    for r in (1, 2):
        for k in (1, 2, 3, 4):
            assert f"despike_kernel<R, {k}>" in code
        assert f"launch_rank<{r}>" in code
    make = (ROOT / "Makefile").read_text()
    assert all("despike.hip" in l for l in make.splitlines() if l.lstrip().startswith("$(HIPCC) $(HIPFLAGS)"))
    assert "despike.hip" in (ROOT / "tools" / "build_variant.sh").read_text() and '"despike.hip"' in (ROOT / "tools" / "kres.py").read_text()
    assert "DespikeParams" in (ROOT / "rbrt_amd" / "csrc" / "device_types.h").read_text()


def test_every_invalid_argument_is_refused_before_a_device_is_touched():
    """Host memory stands in for the inputs and the outputs: a refused call reads and writes none of them."""
    lib = abi.load_hip()
    fake = (C.c_uint8 * 8192)()
    p = C.addressof(fake)
    O = rbrt_amd.despike_opts
    nan, inf = float("nan"), float("inf")
    ok = dict(a=p, b=p + 1024, w=8, h=4, opts=O(), oa=p + 2048, ob=p + 3072, mask=p + 4096, res=p + 5120)

    def call(**kw):
        k = dict(ok, **kw)
        rc = lib.rbrt_hip_despike_halves(0, None, C.c_void_p(k["a"]), C.c_void_p(k["b"]), k["w"], k["h"],
                                         C.byref(k["opts"]) if k["opts"] is not None else None, C.c_void_p(k["oa"]), C.c_void_p(k["ob"]),
                                         C.c_void_p(k["mask"]), C.c_void_p(k["res"]))
        return rc, lib.rbrt_hip_last_error().decode()

    rows = {
        "null a": (dict(a=0), "null"), "null b": (dict(b=0), "null"), "null opts": (dict(opts=None), "null"),
        "width 0": (dict(w=0), "width"), "height 0": (dict(h=0), "height"),
        "radius 0": (dict(opts=O(radius=0)), "radius"), "radius 3": (dict(opts=O(radius=3)), "radius"), "radius 2^31": (dict(opts=O(radius=1 << 31)), "radius"),
        "rank 0": (dict(opts=O(rank=0)), "rank"), "rank 5": (dict(opts=O(rank=5)), "rank"), "rank 2^31": (dict(opts=O(rank=1 << 31)), "rank"),
        "flag 1": (dict(opts=O(flags=1)), "flag"), "high flag": (dict(opts=O(flags=1 << 31)), "flag"),
        "out a is a": (dict(oa=p), "output"), "out a is b": (dict(oa=p + 1024), "output"), "out b is a": (dict(ob=p), "output"),
        "out b is b": (dict(ob=p + 1024), "output"), "mask is a": (dict(mask=p), "output"), "mask is b": (dict(mask=p + 1024), "output"),
        "result is a": (dict(res=p), "output"), "result is b": (dict(res=p + 1024), "output"),
        "out a is a, the rest null": (dict(oa=p, ob=0, mask=0, res=0), "output"),
    }
    for k in range(3):
        rows[f"reserved[{k}]"] = (dict(opts=O(reserved=tuple(int(j == k) for j in range(3)))), "reserved")
    for what, v in (("0", 0.0), ("below 1", 0.999), ("negative", -4.0), ("nan", nan), ("inf", inf), ("-inf", -inf)):
        rows[f"threshold {what}"] = (dict(opts=O(threshold=v)), "threshold")
    for what, v in (("negative", -0.01), ("nan", nan), ("inf", inf), ("-inf", -inf)):
        rows[f"floor {what}"] = (dict(opts=O(floor=v)), "floor")
    for name, (kw, word) in rows.items():
        rc, msg = call(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg.startswith("despike_halves: ") and word in msg, (name, rc, msg)
    for opts in (O(), O(radius=1, rank=4)):
        rc, msg = call(w=1 << 16, h=1 << 15, opts=opts)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and "2^31" in msg, (rc, msg)
        rc, msg = call(w=1 << 31, h=1, opts=opts, oa=0, ob=0, mask=0, res=0)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and "2^31" in msg, (rc, msg)
    assert not any(fake)
    with pytest.raises(abi.RbrtError) as e:
        rbrt_amd.despike_halves(0, p, p + 1024, 8, 4, p + 2048, opts=O(rank=9))
    assert e.value.code == abi.RBRT_ERR_INVALID_ARG


def test_cli_despike_help():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--despike  ", "--despike-threshold <t>", "--despike-rank <k>", "--despike-radius <r>", "--spike-map <file>"):
        assert flag in r.stdout, flag
    for text in ("at least 1 [default: 4]", "1 to 4", "[default: 2]", "1 or 2 [default: 2]", "0 none, 85 the first half image, 170 the second, 255 both",
                 "--pass-samples or --sample-map; --samples must be at least 2; --noisy applies",
                 "--despike that is the image in front of spike removal (with --upscale as well: the"):
        assert text in r.stdout, text
    # the other stages keep their text
    assert "--denoise-guided             filter the image with the feature buffers as guides" in r.stdout
    assert "--upscale <f>                trace the image at 1 / f of its width and height, f 2 to 4, and reconstruct the full size:" in r.stdout


def test_cli_despike_refusals(tmp_path):
    out = ["-t", str(tmp_path / "x.png")]

    def refused(argv, *names):
        r = subprocess.run([str(EXE), *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and all(n in r.stderr for n in names), (argv, r.returncode, r.stderr)
        assert not list(tmp_path.iterdir()), argv  # nothing written

    D = ["--despike", "-s", "8"]
    # the companions --upscale refuses
    refused([*D, "--gpus", "2"], "'--despike'", "--gpus > 1")
    refused([*D, "--adaptive", "0.05"], "'--despike'", "'--adaptive'")
    refused([*D, "--checkpoint", str(tmp_path / "c.bin")], "'--despike'", "--checkpoint")
    refused([*D, "--pass-samples", "4"], "'--despike'", "--pass-samples")
    refused([*D, "--sample-map", str(tmp_path / "m.png")], "'--despike'", "--sample-map")
    refused([*D, "--adaptive", "0.05", "--sample-map", str(tmp_path / "m.png")], "'--despike'", "'--adaptive'")
    refused([*D, "--denoise-guided", "--denoise"], "--denoise-guided", "'--denoise'")
    # fewer than two samples: a half would be empty
    refused(["--despike", "-s", "1"], "'--despike'", "--samples")
    refused(["--despike", "-s", "0"], "'--despike'", "--samples")
    # bad values
    for v in ("0", "0.5", "0.999", "-4", "nan", "inf", "x", ""):
        refused([*D, f"--despike-threshold={v}"], "--despike-threshold")
    for v in ("0", "5", "-1", "x", "1.5", ""):
        refused([*D, f"--despike-rank={v}"], "--despike-rank")
    for v in ("0", "3", "-1", "x", "1.5", ""):
        refused([*D, f"--despike-radius={v}"], "--despike-radius")
    # the options without --despike
    for name, v in (("--despike-threshold", "3"), ("--despike-rank", "3"), ("--despike-radius", "1"), ("--spike-map", str(tmp_path / "m.png"))):
        refused(["-s", "8", name, v], name, "needs '--despike'")
        refused(["--denoise-guided", "-s", "8", name, v], name, "needs '--despike'")
        refused(["--upscale", "2", "-s", "8", name, v], name, "needs '--despike'")
    for flag in ("--despike-threshold", "--despike-rank", "--despike-radius", "--spike-map"):  # a value is required
        assert subprocess.run([str(EXE), "-s", "8", flag], capture_output=True, text=True).returncode == 2
    # what the other options refuse by their own names stays as it was
    refused(["-s", "8", "--noisy", str(tmp_path / "n.png")], "'--noisy' needs '--denoise'")
    refused(["-s", "8", "--sample-map", str(tmp_path / "m.png")], "'--sample-map' needs '--adaptive'")
    refused(["--upscale", "2", "-s", "8", "--sample-map", str(tmp_path / "m.png")], "'--upscale'", "--sample-map")
