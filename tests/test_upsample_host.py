"""Guided upsampling without a GPU: every refusal of rbrt_hip_upsample_halves, rbrt_hip_upsample_camera and
rbrt_hip_upsample_workspace_bytes comes back before a device is needed, the camera helper equals the restatement's rule bit for
bit, the command line's help has the new flags and refuses by name with exit status 2 before anything is loaded or written,
and the new kernel file is hashed and built with the others and shares no code with them."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_upsample as NU
import rbrt_amd
import scenes
import temporal_cases as TC
from rbrt_amd import abi, srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def test_the_kernel_source_is_hashed_built_and_keeps_to_itself():
    assert "rbrt_amd/csrc/upsample.hip" in srchash.KERNEL_SOURCES
    src = (ROOT / "rbrt_amd" / "csrc" / "upsample.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in src
    assert not any(name in code for name in ("kernels.hip", "megakernel.inl", "features.inl", "guided.hip", "temporal.hip"))
    assert "atomic" not in code and "__shfl" not in code and "asm" not in code  # no atomics, no cross-lane sums, plain C++
    assert "__frcp" not in code and "__fdividef" not in code and "fast" not in code  # no reciprocal shortcuts
    make = (ROOT / "Makefile").read_text()
    assert all("upsample.hip" in l for l in make.splitlines() if l.lstrip().startswith("$(HIPCC) $(HIPFLAGS)"))
    assert "upsample.hip" in (ROOT / "tools" / "build_variant.sh").read_text() and '"upsample.hip"' in (ROOT / "tools" / "kres.py").read_text()
    assert "UpsampleParams" in (ROOT / "rbrt_amd" / "csrc" / "device_types.h").read_text()


def cam_with(cam, **kw):
    c = type(cam).from_buffer_copy(cam)
    for name, v in kw.items():
        setattr(c, name, v)
    return c


def test_every_invalid_argument_of_the_stage_is_refused_before_a_device_is_touched():
    """Host memory stands in for the inputs, the workspace and the outputs: a refused call reads and writes none of them."""
    lib = abi.load_hip()
    fake = (C.c_uint8 * 4096)()
    p = (C.addressof(fake) + 15) // 16 * 16  # 16-byte aligned
    O = rbrt_amd.upsample_opts
    nan, inf = float("nan"), float("inf")
    ok = dict(a=p, b=p, wa=p, albedo=p, normal=p, depth=p, coverage=p, w=8, h=4, opts=O(), ws=p + 1024, oa=p, ob=p, ow=p)

    def call(**kw):
        k = dict(ok, **kw)
        rc = lib.rbrt_hip_upsample_halves(0, None, C.c_void_p(k["a"]), C.c_void_p(k["b"]), C.c_void_p(k["wa"]), C.c_void_p(k["albedo"]),
                                          C.c_void_p(k["normal"]), C.c_void_p(k["depth"]), C.c_void_p(k["coverage"]), k["w"], k["h"],
                                          C.byref(k["opts"]) if k["opts"] is not None else None, C.c_void_p(k["ws"]), C.c_void_p(k["oa"]),
                                          C.c_void_p(k["ob"]), C.c_void_p(k["ow"]))
        return rc, lib.rbrt_hip_last_error().decode()

    rows = {
        "null a": (dict(a=0), "null"), "null b": (dict(b=0), "null"), "null albedo": (dict(albedo=0), "null"), "null normal": (dict(normal=0), "null"),
        "null depth": (dict(depth=0), "null"), "null coverage": (dict(coverage=0), "null"), "null opts": (dict(opts=None), "null"),
        "null workspace": (dict(ws=0), "null"),
        "width 0": (dict(w=0), "width"), "height 0": (dict(h=0), "height"),
        "factor 0": (dict(opts=O(factor=0)), "factor"), "factor 5": (dict(opts=O(factor=5)), "factor"), "factor 2^31": (dict(opts=O(factor=1 << 31)), "factor"),
        "flag 2": (dict(opts=O(flags=2)), "flag"), "flag 3": (dict(opts=O(flags=3)), "flag"), "high flag": (dict(opts=O(flags=1 << 31)), "flag"),
        "misaligned workspace 4": (dict(ws=p + 1024 + 4), "aligned"), "misaligned workspace 8": (dict(ws=p + 1024 + 8), "aligned"),
    }
    for k in range(3):
        rows[f"reserved[{k}]"] = (dict(opts=O(reserved=tuple(int(j == k) for j in range(3)))), "reserved")
    for name in ("normal", "depth", "albedo"):
        for what, v in (("0", 0.0), ("negative", -0.5), ("nan", nan), ("inf", inf), ("-inf", -inf)):
            rows[f"{name} {what}"] = (dict(opts=O(**{name: v})), "normal, depth and albedo")
    for name, (kw, word) in rows.items():
        rc, msg = call(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg.startswith("upsample_halves: ") and word in msg, (name, rc, msg)
    for opts in (O(), O(factor=1), O(factor=4, flags=1)):
        rc, msg = call(w=1 << 16, h=1 << 15, opts=opts)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and "2^31" in msg, (rc, msg)
    assert not any(fake)


def test_workspace_bytes():
    wb = rbrt_amd.upsample_workspace_bytes
    assert abi.UPSAMPLE_WORKSPACE_BYTES_PER_LOW_PIXEL == 64
    assert wb(1, 1, 1) == 64 and wb(1, 1, 4) == 64 and wb(37, 21, 1) == 37 * 21 * 64 and wb(37, 21, 2) == 19 * 11 * 64
    assert wb(37, 21, 3) == 13 * 7 * 64 and wb(37, 21, 4) == 10 * 6 * 64 and wb(1024, 768, 2) == 512 * 384 * 64
    for W, H, f in ((50, 47, 2), (5, 5, 4), (17, 7, 3)):
        w, h = NU.low_size(W, H, f)
        assert wb(W, H, f) == w * h * 64 == NU.pack(NU.reduce(np.zeros((h, w, 3), NU.f32), np.zeros((h, w, 3), NU.f32), None, np.zeros((H, W, 3), NU.f32),
                                                              np.zeros((H, W, 3), NU.f32), np.zeros((H, W), NU.f32), np.zeros((H, W), NU.f32), f)).nbytes
    assert wb(0, 5, 2) == 0 and wb(5, 0, 2) == 0 and wb(0, 0, 1) == 0
    assert wb(5, 5, 0) == 0 and wb(5, 5, 5) == 0 and wb(5, 5, 1 << 31) == 0
    assert wb(1 << 16, 1 << 15, 2) == 0 and wb(1 << 31, 1, 4) == 0   # 2^31 pixels: refused
    assert wb((1 << 31) - 1, 1, 1) == ((1 << 31) - 1) * 64            # ... and one fewer is not
    assert wb((1 << 31) - 1, 1, 4) == (1 << 29) * 64


def test_the_camera_helper_refuses_and_otherwise_equals_the_restatement(oracle):
    lib = abi.load_hip()
    cam = scenes.camera(oracle, 50, 47)
    out = abi.Camera()
    nan, inf = float("nan"), float("inf")

    def call(full, f, low):
        rc = lib.rbrt_hip_upsample_camera(C.byref(full) if full is not None else None, f, C.byref(low) if low is not None else None)
        return rc, lib.rbrt_hip_last_error().decode()

    rows = {"null full": ((None, 2, out), "null"), "null low": ((cam, 2, None), "null"), "factor 0": ((cam, 0, out), "factor"),
            "factor 5": ((cam, 5, out), "factor"), "factor 2^31": ((cam, 1 << 31, out), "factor"),
            "width 0": ((cam_with(cam, img_width_pix=0), 2, out), "width"), "height 0": ((cam_with(cam, img_height_pix=0), 2, out), "height")}
    for field in ("mm_per_pix_hor", "mm_per_pix_vert"):
        for what, v in (("nan", nan), ("inf", inf), ("-inf", -inf)):
            rows[f"{field} {what}"] = ((cam_with(cam, **{field: v}), 2, out), "mm_per_pix")
    for name, (args, word) in rows.items():
        rc, msg = call(*args)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg.startswith("upsample_camera: ") and word in msg, (name, rc, msg)
    assert bytes(out) == bytes(abi.Camera())   # a refused call writes nothing
    with pytest.raises(abi.RbrtError):
        rbrt_amd.upsample_camera(cam, 7)
    # bit for bit: sizes that are and are not multiples of the factor, an `up` that is neither normalised nor perpendicular
    for W, H in ((16, 8), (15, 9), (17, 7), (16, 12), (5, 5), (50, 47), (1, 1), (1024, 768), (1920, 1080)):
        for pair in ("static", "turn"):
            full = TC.camera(W, H, **TC.PAIRS[pair])
            for f in (1, 2, 3, 4):
                got, exp = rbrt_amd.upsample_camera(full, f), NU.low_camera(full, f)
                assert bytes(got) == bytes(exp), (W, H, pair, f)
                assert (got.img_width_pix, got.img_height_pix) == NU.low_size(W, H, f)
            assert bytes(rbrt_amd.upsample_camera(full, 1)) == bytes(full)
    full = TC.camera(50, 47)
    rc, _ = call(full, 3, full)   # `low` may be `full` itself
    assert rc == abi.RBRT_OK and bytes(full) == bytes(NU.low_camera(TC.camera(50, 47), 3))


def test_cli_upscale_help():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--upscale <f>", "--upscale-normal <k>", "--upscale-depth <k>", "--upscale-albedo <k>"):
        assert flag in r.stdout, flag
    for text in ("f 2 to 4", "above 0 [default: 0.5]", "above 0 [default: 0.1]", "above 0 [default: 0.2]", "--sample-map; --samples must be at least 2"):
        assert text in r.stdout, text
    # the other stages keep their text
    assert "--denoise-guided             filter the image with the feature buffers as guides" in r.stdout
    assert "--frames <n>                 render a stream of n frames, at least 1, and write the last one" in r.stdout


def test_cli_upscale_refusals(tmp_path):
    out = ["-t", str(tmp_path / "x.png")]

    def refused(argv, *names):
        r = subprocess.run([str(EXE), *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and all(n in r.stderr for n in names), (argv, r.returncode, r.stderr)
        assert not list(tmp_path.iterdir()), argv  # nothing written

    U = ["--upscale", "2", "-s", "8"]
    refused([*U, "--gpus", "2"], "'--upscale'", "--gpus > 1")
    refused([*U, "--adaptive", "0.05"], "'--upscale'", "'--adaptive'")
    refused([*U, "--checkpoint", str(tmp_path / "c.bin")], "'--upscale'", "--checkpoint")
    refused([*U, "--pass-samples", "4"], "'--upscale'", "--pass-samples")
    refused([*U, "--sample-map", str(tmp_path / "m.png")], "'--upscale'", "--sample-map")
    refused([*U, "--adaptive", "0.05", "--sample-map", str(tmp_path / "m.png")], "'--upscale'", "'--adaptive'")
    refused([*U, "--frames", "3", "--gpus", "2"], "--gpus > 1")
    refused([*U, "--denoise-guided", "--denoise"], "--denoise-guided", "'--denoise'")
    # fewer than two samples: a half would be empty
    refused(["--upscale", "2", "-s", "1"], "'--upscale'", "--samples")
    refused(["--upscale", "2", "-s", "0"], "'--upscale'", "--samples")
    # the factor
    for v in ("0", "1", "5", "-1", "x", "2.5", ""):
        refused(["-s", "8", f"--upscale={v}"], "--upscale")
    # a bad sigma
    for name in ("--upscale-normal", "--upscale-depth", "--upscale-albedo"):
        for v in ("0", "-0.5", "nan", "inf", "x", ""):
            refused([*U, f"{name}={v}"], name)
    refused([*U, "--feature-samples", "0"], "--feature-samples")
    # the options without --upscale
    for name in ("--upscale-normal", "--upscale-depth", "--upscale-albedo"):
        refused(["-s", "8", name, "0.3"], name, "needs '--upscale'")
        refused(["--denoise-guided", "-s", "8", name, "0.3"], name, "needs '--upscale'")
    for flag in ("--upscale", "--upscale-normal", "--upscale-depth", "--upscale-albedo"):  # a value is required
        assert subprocess.run([str(EXE), "-s", "8", flag], capture_output=True, text=True).returncode == 2
    # what the other options refuse by their own names stays as it was
    refused(["-s", "8", "--noisy", str(tmp_path / "n.png")], "'--noisy' needs '--denoise'")
    refused(["-s", "8", "--sample-map", str(tmp_path / "m.png")], "'--sample-map' needs '--adaptive'")
    refused(["-s", "8", "--feature-samples", "4"], "'--feature-samples' needs '--features'")
    refused(["--frames", "3", "-s", "8", "--noisy", str(tmp_path / "n.png")], "'--noisy' needs '--denoise'")
