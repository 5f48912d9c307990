"""Image comparison without a GPU: every refusal of rbrt_hip_compare_images comes back before a device is needed, the command
line's help has the new flags and refuses by name with exit status 2 before anything is loaded, rendered or written -- a
reference of another size included -- and the new kernel file is hashed and built with the others and sums without atomics."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import rbrt_amd
from rbrt_amd import abi, srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def test_the_kernel_source_is_hashed_built_and_sums_in_a_fixed_order():
    assert "rbrt_amd/csrc/compare.hip" in srchash.KERNEL_SOURCES
    src = (ROOT / "rbrt_amd" / "csrc" / "compare.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in src
    assert not any(name in code for name in ("kernels.hip", "megakernel.inl", "features.inl", "guided.hip", "temporal.hip", "upsample.hip", "despike.hip"))
    assert "atomic" not in code and "asm" not in code  # the sums across workgroups go through the slab, in a fixed order
    assert "__frcp" not in code and "__fdividef" not in code and "fast" not in code and not re.search(r"exp2?f?\s*\(", code)  # no shortcuts; the taps are literals
    assert "compare_tile_kernel" in code and "compare_reduce_kernel" in code and "dim3(1), dim3(kThreads)" in code  # one workgroup reduces
    make = (ROOT / "Makefile").read_text()
    lines = [l for l in make.splitlines() if l.lstrip().startswith("$(HIPCC) $(HIPFLAGS)")]
    assert lines and all("compare.hip" in l for l in lines)
    assert make.count("$(CSRC)/compare.hip") == make.count("$(CSRC)/despike.hip") == 2 * len(lines)  # ... and on the dependency lists
    assert "compare.hip" in (ROOT / "tools" / "build_variant.sh").read_text() and '"compare.hip"' in (ROOT / "tools" / "kres.py").read_text()
    types = (ROOT / "rbrt_amd" / "csrc" / "device_types.h").read_text()
    assert "struct CompareParams" in types and "struct CompareTilePartial" in types
    lib = ROOT / "rbrt_amd" / "lib" / "librbrt_hip.so"
    assert lib.exists(), "build the library with `make`"
    assert b"compare_tile_kernel" in lib.read_bytes()  # the kernels are in the library that was built


def test_every_invalid_argument_is_refused_before_a_device_is_touched():
    """Host memory stands in for the inputs, the workspace and the outputs: a refused call reads and writes none of them."""
    lib = abi.load_hip()
    fake = (C.c_uint8 * 8192)()
    base = C.addressof(fake)
    p = (base + 63) & ~63  # (the alignment rows below need a base that is aligned)
    O = rbrt_amd.compare_opts
    nan, inf = float("nan"), float("inf")
    ok = dict(x=p, r=p + 1024, w=8, h=4, opts=O(), ws=p + 2048, rel=p + 3072, ssim=p + 4096, res=p + 5120)

    def call(**kw):
        k = dict(ok, **kw)
        rc = lib.rbrt_hip_compare_images(0, None, C.c_void_p(k["x"]), C.c_void_p(k["r"]), k["w"], k["h"], C.byref(k["opts"]) if k["opts"] is not None else None,
                                         C.c_void_p(k["ws"]), C.c_void_p(k["rel"]), C.c_void_p(k["ssim"]), C.c_void_p(k["res"]))
        return rc, lib.rbrt_hip_last_error().decode()

    rows = {
        "null x": (dict(x=0), "null"), "null ref": (dict(r=0), "null"), "null opts": (dict(opts=None), "null"),
        "null workspace with a result": (dict(ws=0), "workspace"), "null workspace with a result alone": (dict(ws=0, rel=0, ssim=0), "workspace"),
        "workspace off by 4": (dict(ws=p + 2052), "aligned"), "result off by 4": (dict(res=p + 5124), "aligned"),
        "width 0": (dict(w=0), "width"), "height 0": (dict(h=0), "height"),
        "flag 1": (dict(opts=O(flags=1)), "flag"), "high flag": (dict(opts=O(flags=1 << 31)), "flag"),
        "reserved[0]": (dict(opts=O(reserved=(1, 0))), "reserved"), "reserved[1]": (dict(opts=O(reserved=(0, 7))), "reserved"),
        "rel is x": (dict(rel=p), "input"), "rel is ref": (dict(rel=p + 1024), "input"), "ssim is x": (dict(ssim=p), "input"), "ssim is ref": (dict(ssim=p + 1024), "input"),
        "result is x": (dict(res=p), "input"), "result is ref": (dict(res=p + 1024), "input"), "workspace is x": (dict(ws=p), "input"),
        "workspace is ref": (dict(ws=p + 1024), "input"), "rel is x, the rest null": (dict(rel=p, ssim=0, res=0, ws=0), "input"),
        "ssim is rel": (dict(ssim=p + 3072), "another output"), "result is rel": (dict(res=p + 3072), "another output"),
        "result is ssim": (dict(res=p + 4096), "another output"), "workspace is rel": (dict(ws=p + 3072), "another output"),
        "workspace is ssim": (dict(ws=p + 4096), "another output"), "workspace is the result": (dict(ws=p + 5120), "another output"),
        "x is ref, and an output is both": (dict(r=p, rel=p), "input"),
    }
    for what, v in (("0", 0.0), ("-0", -0.0), ("negative", -0.01), ("nan", nan), ("inf", inf), ("-inf", -inf)):
        rows[f"epsilon {what}"] = (dict(opts=O(epsilon=v)), "epsilon")
    for name, (kw, word) in rows.items():
        rc, msg = call(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg.startswith("compare_images: ") and word in msg, (name, rc, msg)
    for kw in (dict(w=1 << 16, h=1 << 15), dict(w=1 << 31, h=1, ws=0, rel=0, ssim=0, res=0), dict(w=1 << 16, h=1 << 15, opts=O(epsilon=3.0))):
        rc, msg = call(**kw)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and "2^31" in msg, (rc, msg)
    assert not any(fake)
    with pytest.raises(abi.RbrtError) as e:
        rbrt_amd.compare_images(0, p, p + 1024, 8, 4, p + 2048, d_result=p + 5120, opts=O(epsilon=-1.0))
    assert e.value.code == abi.RBRT_ERR_INVALID_ARG


def test_cli_compare_help():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--compare <ref.pfm>", "--compare-epsilon <e>", "--error-map <file>", "--ssim-map <file>"):
        assert flag in r.stdout, flag
    for text in ("above 0", "[default: 0.01]", "MSE, MAE, relative MSE, PSNR (peak 1) and mean SSIM; --report gains compare_*", "0 black to 1 and", "1 (identical) white",
                 "the same images give the same bits"):
        assert text in r.stdout, text
    # the other stages keep their text
    assert "--despike                    remove spikes (fireflies)" in r.stdout
    assert "--radiance <file.pfm>        also write the linear radiance there as a colour PFM" in r.stdout


def write_pfm(path, a):
    h, w, _ = a.shape
    Path(path).write_bytes(f"PF\n{w} {h}\n-1.0\n".encode() + np.ascontiguousarray(a[::-1], "<f4").tobytes())


def test_cli_compare_refusals(tmp_path):
    out = ["-t", str(tmp_path / "x.png")]
    given = set()

    def refused(argv, *names):
        r = subprocess.run([str(EXE), *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and all(n in r.stderr for n in names), (argv, r.returncode, r.stderr)
        assert "Starting rendering" not in r.stdout and set(tmp_path.iterdir()) == given, argv  # nothing rendered, nothing written

    # the dependent flags without --compare
    for name, v in (("--compare-epsilon", "0.1"), ("--error-map", str(tmp_path / "e.png")), ("--ssim-map", str(tmp_path / "s.pfm"))):
        refused(["-s", "2", name, v], name, "needs '--compare'")
        refused(["--denoise", "-s", "2", name, v], name, "needs '--compare'")
    for flag in ("--compare", "--compare-epsilon", "--error-map", "--ssim-map"):  # a value is required
        assert subprocess.run([str(EXE), "-s", "2", flag], capture_output=True, text=True).returncode == 2
    # a missing or unreadable reference
    refused(["--compare", str(tmp_path / "missing.pfm")], "'--compare'", "missing.pfm")
    refused(["--compare", ""], "'--compare'")
    grey, short, text = tmp_path / "grey.pfm", tmp_path / "short.pfm", tmp_path / "text.pfm"
    grey.write_bytes(b"Pf\n2 2\n-1.0\n" + bytes(16))
    short.write_bytes(b"PF\n2 2\n-1.0\n" + bytes(40))
    text.write_text("not an image")
    ref = tmp_path / "ref.pfm"
    a = np.full((6, 8, 3), 0.25, np.float32)
    a[1, 2] = (np.nan, -1.0, np.inf)  # (a reference may hold anything: such a pixel is skipped)
    write_pfm(ref, a)
    given |= {grey, short, text, ref}
    refused(["--compare", str(grey)], "'--compare'", "grey.pfm")
    refused(["--compare", str(short)], "'--compare'", "truncated")
    refused(["--compare", str(text)], "'--compare'", "text.pfm")
    # a reference of another size: caught before any render (no GPU is needed to get here)
    refused(["--compare", str(ref)], "'--compare'", "8 x 6", "800 x 600")
    refused(["--compare", str(ref), "-w", "8", "--height", "7"], "8 x 6", "8 x 7")
    refused(["--compare", str(ref), "-w", "6", "--height", "8"], "8 x 6", "6 x 8")
    refused(["--compare", str(ref), "-w", "16", "--height", "12", "--upscale", "2", "-s", "2"], "8 x 6", "16 x 12")  # (the image's size counts, not the traced one)
    # a bad epsilon
    for v in ("0", "-0.5", "nan", "inf", "-inf", "x", "", "1e-60"):
        refused(["--compare", str(ref), "-w", "8", "--height", "6", f"--compare-epsilon={v}"], "--compare-epsilon")
    # what the other options refuse by their own names stays as it was
    refused(["-s", "8", "--spike-map", str(tmp_path / "m.png")], "needs '--despike'")
    refused(["-s", "8", "--radiance", str(tmp_path / "r.png")], "'--radiance'")
