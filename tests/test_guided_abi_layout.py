"""The guided denoiser's additions to the C ABI, without a GPU: rbrt_guided_opts_t has the layout a C compiler gives
include/rbrt_hip.h in its ctypes mirror (rbrt_amd/abi.py), the entry points are in the symbol table, the ABI version stays 2,
rbrt_hip_guided_workspace_bytes answers 0 for what the call refuses, and every RBRT_ERR_INVALID_ARG row of
rbrt_hip_denoise_guided comes back before a device is touched."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import np_guided
import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def test_guided_opts_layout_matches_the_c_header(tmp_path):
    cname, cls = "rbrt_guided_opts_t", abi.GuidedOpts
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("flag %u\\n", RBRT_GUIDED_NO_DEMODULATION); printf("max %u\\n", RBRT_GUIDED_MAX_LEVELS);')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "gd.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "gd"), str(tmp_path / "gd.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "gd")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 32
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert [f for f, _ in cls._fields_] == ["levels", "colour", "normal", "depth", "albedo", "flags", "reserved"]
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == [0, 4, 8, 12, 16, 20, 24]
    assert int(got["flag"]) == abi.GUIDED_NO_DEMODULATION == np_guided.NO_DEMODULATION == 1
    assert int(got["max"]) == abi.GUIDED_MAX_LEVELS == 6


def test_symbols_version_and_defaults():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_guided_opts_default", "rbrt_hip_guided_workspace_bytes", "rbrt_hip_denoise_guided", "rbrt_hip_scene_denoise_guided"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(abi.HIP_SYMBOLS["rbrt_hip_denoise_guided"][1]) == 15 and len(abi.HIP_SYMBOLS["rbrt_hip_scene_denoise_guided"][1]) == 10
    d = abi.GuidedOpts(9, 9.0, 9.0, 9.0, 9.0, 9, (9, 9))
    lib.rbrt_guided_opts_default(C.byref(d))
    assert (d.levels, d.flags, list(d.reserved)) == (5, 0, [0, 0])
    assert (d.colour, d.normal, d.depth, d.albedo) == (f32(2.0), f32(0.35), f32(0.05), f32(0.1))
    lib.rbrt_guided_opts_default(None)  # (a NULL is ignored, as by the other *_default calls)
    assert np_guided.DEFAULTS == dict(levels=5, colour=2.0, normal=0.35, depth=0.05, albedo=0.1, flags=0)
    g = rbrt_amd.guided_opts(levels=3, depth=0.5, flags=1)
    assert (g.levels, g.depth, g.flags, g.colour) == (3, f32(0.5), 1, f32(2.0))
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "int rbrt_hip_denoise_guided(" in header and "int rbrt_hip_scene_denoise_guided(" in header
    assert "#define RBRT_ABI_VERSION 2" in header
    assert re.search(r"#define RBRT_GUIDED_TILE (\d+)u", (ROOT / "include" / "rbrt_hip_debug.h").read_text())
    assert hasattr(rbrt_amd.HipScene, "denoise_guided") and callable(rbrt_amd.denoise_guided)


def test_workspace_bytes():
    ws = rbrt_amd.guided_workspace_bytes
    assert ws(1, 1) == 96 and ws(37, 21) == 37 * 21 * 96 and ws(1024, 768) == 1024 * 768 * 96
    assert ws(0, 5) == 0 and ws(5, 0) == 0 and ws(0, 0) == 0
    assert ws(1 << 16, 1 << 15) == 0 and ws(1 << 31, 1) == 0       # 2^31 pixels: refused
    assert ws((1 << 31) - 1, 1) == ((1 << 31) - 1) * 96             # ... and one fewer is not


def test_every_invalid_argument_is_refused_before_a_device_is_touched():
    """Host memory stands in for the handle, the inputs, the workspace and the outputs: a refused call reads none of them."""
    lib = abi.load_hip()
    fake = (C.c_uint8 * 4096)()
    base = C.addressof(fake)
    p = (base + 15) // 16 * 16  # 16-byte aligned
    G = rbrt_amd.guided_opts
    nan, inf = float("nan"), float("inf")
    ok = dict(a=p, b=p, wa=p, albedo=p, normal=p, depth=p, coverage=p, w=8, h=4, opts=G(), ws=p)

    def call(**kw):
        k = dict(ok, **kw)
        o = k["opts"]
        rc = lib.rbrt_hip_denoise_guided(0, None, C.c_void_p(k["a"]), C.c_void_p(k["b"]), C.c_void_p(k["wa"]), C.c_void_p(k["albedo"]),
                                         C.c_void_p(k["normal"]), C.c_void_p(k["depth"]), C.c_void_p(k["coverage"]), k["w"], k["h"],
                                         C.byref(o) if o is not None else None, C.c_void_p(k["ws"]), C.c_void_p(p + 1024), None)
        return rc, lib.rbrt_hip_last_error()

    def scene_call(scene=p, **kw):
        k = dict(ok, **kw)
        o = k["opts"]
        rc = lib.rbrt_hip_scene_denoise_guided(C.c_void_p(scene), C.byref(o) if o is not None else None, None, C.c_void_p(k["albedo"]),
                                               C.c_void_p(k["normal"]), C.c_void_p(k["depth"]), C.c_void_p(k["coverage"]),
                                               C.c_void_p(k["ws"]), C.c_void_p(p + 1024), None)
        return rc, lib.rbrt_hip_last_error()

    shared = {"null albedo": dict(albedo=0), "null normal": dict(normal=0), "null depth": dict(depth=0), "null coverage": dict(coverage=0),
              "null opts": dict(opts=None), "null workspace": dict(ws=0), "misaligned workspace": dict(ws=p + 4),
              "levels 0": dict(opts=G(levels=0)), "levels 7": dict(opts=G(levels=7)), "unknown flag": dict(opts=G(flags=2)),
              "unknown flag beside the known": dict(opts=G(flags=3)), "high flag": dict(opts=G(flags=1 << 31)),
              "reserved[0]": dict(opts=G(reserved=(1, 0))), "reserved[1]": dict(opts=G(reserved=(0, 1)))}
    for name in ("colour", "normal", "depth", "albedo"):
        for what, v in (("0", 0.0), ("negative", -1.0), ("nan", nan), ("inf", inf)):
            shared[f"{name} {what}"] = dict(opts=G(**{name: v}))
    rows = dict(shared, **{"null a": dict(a=0), "null b": dict(b=0), "width 0": dict(w=0), "height 0": dict(h=0)})
    for name, kw in rows.items():
        rc, msg = call(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (name, rc, msg)
    for name, kw in shared.items():
        rc, msg = scene_call(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (name, rc, msg)
    rc, msg = scene_call(scene=0)
    assert rc == abi.RBRT_ERR_INVALID_ARG and msg
    assert call(w=1 << 16, h=1 << 15)[0] == abi.RBRT_ERR_UNSUPPORTED
    assert call(wa=0, w=0)[0] == abi.RBRT_ERR_INVALID_ARG  # (d_wa alone is optional: the refusal is the width's)
    assert not any(fake)
