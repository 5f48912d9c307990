"""Temporal accumulation without a GPU: every refusal of rbrt_hip_temporal_accumulate comes back with its message before a
device is needed, the command line's help has the new flags and refuses by name with exit status 2 before anything is loaded or
written, and the new kernel file is hashed with the others and shares no code with them."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import rbrt_amd
import temporal_cases as TC
from rbrt_amd import abi, srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def test_the_kernel_source_is_hashed_and_keeps_to_itself():
    assert "rbrt_amd/csrc/temporal.hip" in srchash.KERNEL_SOURCES
    src = (ROOT / "rbrt_amd" / "csrc" / "temporal.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    assert "#pragma clang fp contract(off)" in src
    assert not any(name in code for name in ("kernels.hip", "megakernel.inl", "features.inl", "guided.hip"))
    assert "atomic" not in code and "__shfl" not in code  # no atomics, no cross-lane sums
    make = (ROOT / "Makefile").read_text()
    assert make.count("$(HIPCC) $(HIPFLAGS)") == 2 and all("temporal.hip" in l for l in make.splitlines() if l.lstrip().startswith("$(HIPCC) $(HIPFLAGS)"))


def test_every_invalid_argument_is_refused_before_a_device_is_touched():
    """Host memory stands in for the inputs, the histories and the outputs: a refused call reads none of them."""
    lib = abi.load_hip()
    fake = (C.c_uint8 * 4096)()
    p = (C.addressof(fake) + 15) // 16 * 16  # 16-byte aligned
    O = rbrt_amd.temporal_opts
    nan, inf = float("nan"), float("inf")
    cam = TC.camera(8, 4)

    def cam_with(**kw):
        c = type(cam).from_buffer_copy(cam)
        for name, v in kw.items():
            if isinstance(v, tuple):
                for k in range(3):
                    getattr(c, name)[k] = v[k]
            else:
                setattr(c, name, v)
        return c

    ok = dict(a=p, b=p, normal=p, depth=p, coverage=p, cam=cam, prev=cam, opts=O(), hin=p + 1024, hout=p + 2048, oa=p, ob=p, ol=p)

    def call(**kw):
        k = dict(ok, **kw)
        ref = lambda x: C.byref(x) if x is not None else None
        rc = lib.rbrt_hip_temporal_accumulate(0, None, C.c_void_p(k["a"]), C.c_void_p(k["b"]), C.c_void_p(k["normal"]), C.c_void_p(k["depth"]),
                                              C.c_void_p(k["coverage"]), ref(k["cam"]), ref(k["prev"]), ref(k["opts"]), C.c_void_p(k["hin"]),
                                              C.c_void_p(k["hout"]), C.c_void_p(k["oa"]), C.c_void_p(k["ob"]), C.c_void_p(k["ol"]))
        return rc, lib.rbrt_hip_last_error().decode()

    rows = {
        "null a": (dict(a=0), "null"), "null b": (dict(b=0), "null"), "null normal": (dict(normal=0), "null"), "null depth": (dict(depth=0), "null"),
        "null coverage": (dict(coverage=0), "null"), "null cam": (dict(cam=None), "null"), "null opts": (dict(opts=None), "null"),
        "history without cam_prev": (dict(prev=None), "cam_prev"),
        "history in == out": (dict(hout=p + 1024), "differ"),
        "misaligned history in": (dict(hin=p + 1024 + 4), "aligned"), "misaligned history out": (dict(hout=p + 2048 + 8), "aligned"),
        "misaligned history out, first frame": (dict(hin=0, prev=None, hout=p + 2048 + 8), "aligned"),
        "width 0": (dict(cam=cam_with(img_width_pix=0), prev=cam_with(img_width_pix=0)), "width"),
        "height 0": (dict(cam=cam_with(img_height_pix=0), prev=cam_with(img_height_pix=0)), "height"),
        "cam_prev's width": (dict(prev=cam_with(img_width_pix=9)), "size"), "cam_prev's height": (dict(prev=cam_with(img_height_pix=5)), "size"),
        "flag": (dict(opts=O(flags=1)), "flag"), "high flag": (dict(opts=O(flags=1 << 31)), "flag"),
        "degenerate cam_prev: right parallel to up": (dict(prev=cam_with(right=(0.0, 1.0, -0.4))), "degenerate"),
        "degenerate cam_prev: right 0": (dict(prev=cam_with(right=(0.0, 0.0, 0.0))), "degenerate"),
        "degenerate cam_prev: image plane through the position": (dict(prev=cam_with(img_center_point=tuple(cam.position))), "degenerate"),
        "degenerate cam_prev: nan": (dict(prev=cam_with(up=(nan, 1.0, 0.0))), "degenerate"),
        "degenerate cam_prev: inf": (dict(prev=cam_with(position=(inf, 0.0, 0.0))), "degenerate"),
    }
    for k in range(4):
        rows[f"reserved[{k}]"] = (dict(opts=O(reserved=tuple(int(j == k) for j in range(4)))), "reserved")
    for what, v in (("0.5", 0.5), ("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
        rows[f"max_history {what}"] = (dict(opts=O(max_history=v)), "max_history")
    for name in ("depth", "normal"):
        for what, v in (("negative", -0.5), ("nan", nan), ("inf", inf)):
            rows[f"{name} {what}"] = (dict(opts=O(**{name: v})), "depth and normal")
    for field in ("mm_per_pix_hor", "mm_per_pix_vert"):
        for what, v in (("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
            rows[f"cam {field} {what}"] = (dict(cam=cam_with(**{field: v})), "cam's mm_per_pix")
            rows[f"cam_prev {field} {what}"] = (dict(prev=cam_with(**{field: v})), "cam_prev's mm_per_pix")
    for name, (kw, word) in rows.items():
        rc, msg = call(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg.startswith("temporal_accumulate: ") and word in msg, (name, rc, msg)
    big = cam_with(img_width_pix=1 << 16, img_height_pix=1 << 15)
    rc, msg = call(cam=big, prev=big)
    assert rc == abi.RBRT_ERR_UNSUPPORTED and "2^31" in msg, (rc, msg)
    rc, msg = call(cam=big, prev=None, hin=0)  # ... on the first frame too
    assert rc == abi.RBRT_ERR_UNSUPPORTED, (rc, msg)
    assert not any(fake)


def test_cli_temporal_help():
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--frames <n>", "--camera-step <dx,dy,dz>", "--temporal-max-history <m>", "--temporal-depth <k>", "--temporal-normal <k>",
                 "--history-map <file>"):
        assert flag in r.stdout, flag
    for text in ("[default: 0,0,0]", "at least 1 [default: 32]", "0 or more [default: 0.05]", "0 or more [default: 0.35]", "seed + k"):
        assert text in r.stdout, text
    # the other filters keep their text
    assert "--denoise                    filter the image: a dual-buffer non-local-means filter" in r.stdout
    assert "--denoise-guided             filter the image with the feature buffers as guides" in r.stdout


def test_cli_temporal_refusals(tmp_path):
    out = ["-t", str(tmp_path / "x.png")]

    def refused(argv, *names):
        r = subprocess.run([str(EXE), *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and all(n in r.stderr for n in names), (argv, r.returncode, r.stderr)
        assert not list(tmp_path.iterdir()), argv  # nothing written

    F = ["--frames", "3", "-s", "8"]
    refused([*F, "--gpus", "2"], "'--frames'", "--gpus > 1")
    refused([*F, "--adaptive", "0.05"], "'--frames'", "'--adaptive'")
    refused([*F, "--checkpoint", str(tmp_path / "c.bin")], "'--frames'", "--checkpoint")
    refused([*F, "--pass-samples", "4"], "'--frames'", "--pass-samples")
    refused([*F, "--denoise", "--gpus", "2"], "--gpus > 1")
    refused([*F, "--denoise-guided", "--denoise"], "--denoise-guided", "'--denoise'")
    # fewer than two samples: a half would be empty
    refused(["--frames", "3", "-s", "1"], "'--frames'", "--samples")
    refused(["--frames", "3", "-s", "0"], "'--frames'", "--samples")
    # values out of range
    for v in ("0", "-1", "x", "2.5", ""):
        refused(["-s", "8", f"--frames={v}"], "--frames")
    for v in ("1,2", "1,2,3,4", "a,b,c", "nan,0,0", "0,inf,0", "1;2;3", ""):
        refused([*F, f"--camera-step={v}"], "--camera-step")
    for v in ("0", "0.5", "-1", "nan", "inf", "x", ""):
        refused([*F, f"--temporal-max-history={v}"], "--temporal-max-history")
    for name in ("--temporal-depth", "--temporal-normal"):
        for v in ("-0.5", "nan", "inf", "x", ""):
            refused([*F, f"{name}={v}"], name)
    refused([*F, "--feature-samples", "0"], "--feature-samples")
    # the options without --frames
    for argv, name in ((["--camera-step", "0.1,0,0"], "--camera-step"), (["--temporal-max-history", "8"], "--temporal-max-history"),
                       (["--temporal-depth", "0.1"], "--temporal-depth"), (["--temporal-normal", "0.1"], "--temporal-normal"),
                       (["--history-map", str(tmp_path / "h.png")], "--history-map")):
        refused(["-s", "8", *argv], name, "needs '--frames'")
        refused(["--denoise", "-s", "8", *argv], name, "needs '--frames'")
    for flag in ("--frames", "--camera-step", "--temporal-max-history", "--temporal-depth", "--temporal-normal", "--history-map"):  # a value is required
        assert subprocess.run([str(EXE), "-s", "8", flag], capture_output=True, text=True).returncode == 2
    # what the other options refuse by their own names stays as it was
    refused(["-s", "8", "--noisy", str(tmp_path / "n.png")], "'--noisy' needs '--denoise'")
    refused(["-s", "8", "--feature-samples", "4"], "'--feature-samples' needs '--features'")
    refused([*F, "--noisy", str(tmp_path / "n.png")], "'--noisy' needs '--denoise'")
