"""Guided upsampling's additions to the C ABI, without a GPU: rbrt_upsample_opts_t has the layout a C compiler gives
include/rbrt_hip.h in its ctypes mirror (rbrt_amd/abi.py), the entry points are in the symbol table, the ABI version stays 2,
the defaults are the header's, and the gather kernel's tile is the same in the debug header and in abi.py."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import np_upsample
import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def test_upsample_opts_layout_matches_the_c_header(tmp_path):
    cname, cls = "rbrt_upsample_opts_t", abi.UpsampleOpts
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "up.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "up"), str(tmp_path / "up.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "up")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 32
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert [f for f, _ in cls._fields_] == ["factor", "normal", "depth", "albedo", "flags", "reserved"]
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == [0, 4, 8, 12, 16, 20]


def test_symbols_version_and_defaults():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_upsample_opts_default", "rbrt_hip_upsample_camera", "rbrt_hip_upsample_workspace_bytes", "rbrt_hip_upsample_halves"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(abi.HIP_SYMBOLS["rbrt_hip_upsample_halves"][1]) == 16
    d = abi.UpsampleOpts(9, 9.0, 9.0, 9.0, 9, (9, 9, 9))
    lib.rbrt_upsample_opts_default(C.byref(d))
    assert (d.factor, d.normal, d.depth, d.albedo, d.flags, list(d.reserved)) == (2, f32(0.5), f32(0.1), f32(0.2), 0, [0, 0, 0])
    lib.rbrt_upsample_opts_default(None)  # (a NULL is ignored, as by the other *_default calls)
    assert np_upsample.DEFAULTS == dict(factor=2, normal=0.5, depth=0.1, albedo=0.2, flags=0)
    t = rbrt_amd.upsample_opts(factor=3, albedo=0.4, flags=1)
    assert (t.factor, t.normal, t.depth, t.albedo, t.flags) == (3, f32(0.5), f32(0.1), f32(0.4), 1)
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "int rbrt_hip_upsample_halves(" in header and "size_t rbrt_hip_upsample_workspace_bytes(" in header
    assert "int rbrt_hip_upsample_camera(" in header and "#define RBRT_ABI_VERSION 2" in header
    assert "#define RBRT_UPSAMPLE_NO_DEMODULATION 1u" in header and abi.UPSAMPLE_NO_DEMODULATION == np_upsample.NO_DEMODULATION == 1
    assert "#define RBRT_UPSAMPLE_MAX_FACTOR 4u" in header and abi.UPSAMPLE_MAX_FACTOR == np_upsample.MAX_FACTOR == 4
    debug = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
    tw, th = (int(re.search(rf"#define RBRT_UPSAMPLE_TILE_{k} (\d+)u", debug).group(1)) for k in "WH")
    assert (tw, th) == (abi.UPSAMPLE_TILE_W, abi.UPSAMPLE_TILE_H) and tw * th == 256
    for name in ("upsample_opts", "upsample_workspace_bytes", "upsample_camera", "upsample_halves"):
        assert callable(getattr(rbrt_amd, name))
