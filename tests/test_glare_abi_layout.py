"""The glare stage's additions to the C ABI, without a GPU: rbrt_glare_opts_t has the layout a C compiler gives
include/rbrt_hip.h in its ctypes mirror (rbrt_amd/abi.py), the defines of both headers are the numbers abi.py has, the entry
points are in the symbol table, the ABI version stays 2, the workspace size is 0 for what the call refuses, and every
RBRT_ERR_INVALID_ARG row of rbrt_hip_glare comes back before a device is touched."""
import ctypes as C
import subprocess
from pathlib import Path

import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
DEFINES = {"RBRT_GLARE_MAX_LEVELS": abi.GLARE_MAX_LEVELS, "RBRT_GLARE_TILE_W": abi.GLARE_TILE_W, "RBRT_GLARE_TILE_H": abi.GLARE_TILE_H}


def test_glare_layout_matches_the_c_headers(tmp_path):
    structs = {"rbrt_glare_opts_t": abi.GlareOpts}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'printf("{d} %lu\\n", (unsigned long)({d}));' for d in DEFINES]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip_debug.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "gl.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "gl"), str(tmp_path / "gl.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "gl")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    for d, value in DEFINES.items():
        assert int(got[d]) == value, d
    assert C.sizeof(abi.GlareOpts) == 32 and abi.GlareOpts.reserved.offset == 16
    assert [f for f, _ in abi.GlareOpts._fields_] == ["threshold", "intensity", "levels", "spread", "reserved"]


def test_symbols_version_and_defaults():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_hip_glare", "rbrt_hip_glare_workspace_bytes", "rbrt_glare_opts_default"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    d = abi.GlareOpts(9, 9, 9, 9, (9, 9, 9, 9))
    lib.rbrt_glare_opts_default(C.byref(d))
    assert (d.threshold, d.levels, d.spread, list(d.reserved)) == (1.0, 5, 1.0, [0, 0, 0, 0])
    assert d.intensity == C.c_float(0.1).value
    g = rbrt_amd.glare_opts(threshold=0.5, levels=3)
    assert (g.threshold, g.levels, g.spread, g.intensity) == (0.5, 3, 1.0, C.c_float(0.1).value)


def test_workspace_bytes():
    wb = rbrt_amd.glare_workspace_bytes
    # refused arguments
    assert wb(0, 7, 3) == 0 and wb(7, 0, 3) == 0 and wb(7, 7, 0) == 0 and wb(7, 7, abi.GLARE_MAX_LEVELS + 1) == 0
    assert wb(1 << 16, 1 << 15, 1) == 0 and wb((1 << 31) - 1, 2, 1) == 0 and wb(0xFFFFFFFF, 0xFFFFFFFF, 8) == 0
    # levels 1..L must fit, whatever the layout: at least 12 bytes a pixel, and no more than a 16-byte pixel and a page of padding a level
    for (w, h, levels) in ((1, 1, 1), (1, 1, 8), (1, 7, 8), (97, 131, 1), (97, 131, 5), (1024, 768, 8), ((1 << 31) - 1, 1, 8), (46340, 46340, 2)):
        pixels, ww, hh = 0, w, h
        for _ in range(levels):
            ww, hh = (ww + 1) // 2, (hh + 1) // 2
            pixels += ww * hh
        got = wb(w, h, levels)
        assert 12 * pixels <= got <= 16 * pixels + 4096 * levels, (w, h, levels, got)
    assert wb(97, 131, 5) > wb(97, 131, 4) > wb(97, 131, 1) > 0


def test_every_invalid_argument_is_refused_before_a_device_is_touched():
    """Host pointers stand in for device memory: a refused call never reads them. The device number is one no machine has,
    so a call that got past the argument checks would fail with another status."""
    lib = abi.load_hip()
    T = rbrt_amd.glare_opts
    nan, inf = float("nan"), float("inf")
    buf = (C.c_float * 64)()
    ws = (C.c_uint8 * 1024)()
    x = C.addressof(buf)
    w16 = (C.addressof(ws) + 15) & ~15
    rows = {
        "null radiance": (0, 4, 4, T(), w16),
        "null opts": (x, 4, 4, None, w16),
        "null workspace": (x, 4, 4, T(), 0),
        "width 0": (x, 0, 4, T(), w16),
        "height 0": (x, 4, 0, T(), w16),
        "levels 0": (x, 4, 4, T(levels=0), w16),
        "levels 9": (x, 4, 4, T(levels=abi.GLARE_MAX_LEVELS + 1), w16),
        "reserved[0]": (x, 4, 4, T(reserved=(1, 0, 0, 0)), w16),
        "reserved[1]": (x, 4, 4, T(reserved=(0, 1, 0, 0)), w16),
        "reserved[2]": (x, 4, 4, T(reserved=(0, 0, 1, 0)), w16),
        "reserved[3]": (x, 4, 4, T(reserved=(0, 0, 0, 1)), w16),
        "threshold nan": (x, 4, 4, T(threshold=nan), w16),
        "threshold inf": (x, 4, 4, T(threshold=inf), w16),
        "threshold negative": (x, 4, 4, T(threshold=-0.5), w16),
        "intensity nan": (x, 4, 4, T(intensity=nan), w16),
        "intensity inf": (x, 4, 4, T(intensity=inf), w16),
        "intensity 0": (x, 4, 4, T(intensity=0.0), w16),
        "intensity negative": (x, 4, 4, T(intensity=-0.1), w16),
        "intensity above 1": (x, 4, 4, T(intensity=1.0000001), w16),
        "spread nan": (x, 4, 4, T(spread=nan), w16),
        "spread inf": (x, 4, 4, T(spread=inf), w16),
        "spread negative": (x, 4, 4, T(spread=-1.0), w16),
        "workspace not aligned": (x, 4, 4, T(), w16 + 8),
    }
    for name, (d_in, w, h, o, d_ws) in rows.items():
        rc = lib.rbrt_hip_glare(1 << 20, None, C.c_void_p(d_in), w, h, C.byref(o) if o is not None else None, C.c_void_p(d_ws),
                                C.c_void_p(x), None)
        assert rc == abi.RBRT_ERR_INVALID_ARG, (name, rc, lib.rbrt_hip_last_error())
        assert b"glare" in lib.rbrt_hip_last_error(), name
    rc = lib.rbrt_hip_glare(1 << 20, None, C.c_void_p(x), 1 << 16, 1 << 15, C.byref(T()), C.c_void_p(w16), C.c_void_p(x), None)
    assert rc == abi.RBRT_ERR_UNSUPPORTED, (rc, lib.rbrt_hip_last_error())
