"""Image comparison's additions to the C ABI, without a GPU: rbrt_compare_opts_t, rbrt_compare_result_t and
rbrt_compare_summary_t have the layout a C compiler gives include/rbrt_hip.h in their ctypes mirrors (rbrt_amd/abi.py), the entry
points are in the symbol table, the ABI version stays 2, the defaults are the header's, the tile of the sums is the same in the
header, in abi.py and in the restatement, and rbrt_compare_summary makes the same divisions as Python, bit for bit."""
import ctypes as C
import math
import re
import struct
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np

import compare_cases as CC
import np_compare as NC
import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
STRUCTS = {"rbrt_compare_opts_t": abi.CompareOpts, "rbrt_compare_result_t": abi.CompareResult, "rbrt_compare_summary_t": abi.CompareSummary}


def test_struct_layouts_match_the_c_header(tmp_path):
    lines = []
    for cname, cls in STRUCTS.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "cmp.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "cmp"), str(tmp_path / "cmp.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "cmp")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in STRUCTS.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert (C.sizeof(abi.CompareOpts), C.sizeof(abi.CompareResult), C.sizeof(abi.CompareSummary)) == (16, 64, 40)
    assert [f for f, _ in abi.CompareOpts._fields_] == ["epsilon", "flags", "reserved"]
    assert [getattr(abi.CompareOpts, f).offset for f, _ in abi.CompareOpts._fields_] == [0, 4, 8]
    assert [f for f, _ in abi.CompareResult._fields_] == ["sum_se", "sum_ae", "sum_rel", "sum_ssim", "max_abs", "usable", "skipped", "reserved"]
    assert [getattr(abi.CompareResult, f).offset for f, _ in abi.CompareResult._fields_] == [0, 8, 16, 24, 32, 36, 40, 44]
    assert [f for f, _ in abi.CompareSummary._fields_] == ["mse", "mae", "relmse", "psnr_db", "ssim"]
    assert struct.calcsize(NC.RESULT_FORMAT) == 64  # the restatement packs the same 64 bytes


def test_symbols_version_defaults_and_the_tile():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    names = ("rbrt_compare_opts_default", "rbrt_hip_compare_workspace_bytes", "rbrt_hip_compare_images", "rbrt_compare_summary")
    for name in names:
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(abi.HIP_SYMBOLS["rbrt_hip_compare_images"][1]) == 11 and len(abi.HIP_SYMBOLS["rbrt_compare_summary"][1]) == 5
    d = abi.CompareOpts(9.0, 9, (9, 9))
    lib.rbrt_compare_opts_default(C.byref(d))
    assert (d.epsilon, d.flags, list(d.reserved)) == (f32(0.01), 0, [0, 0])
    lib.rbrt_compare_opts_default(None)  # (a NULL is ignored, as by the other *_default calls)
    assert NC.DEFAULTS == dict(epsilon=0.01)
    t = rbrt_amd.compare_opts(epsilon=0.5)
    assert (t.epsilon, t.flags, list(t.reserved)) == (f32(0.5), 0, [0, 0])
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    for text in ("int rbrt_hip_compare_images(", "void rbrt_compare_opts_default(", "size_t rbrt_hip_compare_workspace_bytes(", "void rbrt_compare_summary(",
                 "#define RBRT_ABI_VERSION 2"):
        assert text in header, text
    tw, th = (int(re.search(rf"#define RBRT_COMPARE_TILE_{k} (\d+)u", header).group(1)) for k in "WH")
    assert (tw, th) == (abi.COMPARE_TILE_W, abi.COMPARE_TILE_H) == (NC.TILE_W, NC.TILE_H) == (CC.TW, CC.TH) == (16, 16) and tw * th == NC.LANES
    # the header's literals are the restatement's
    for lit in ("0.00102838012f", "0.00759875821f", "0.0360007733f", "0.109360687f", "0.213005543f", "0.266011715f", "C1 = 0.0001f", "C2 = 0.0009f"):
        assert lit in header, lit
    assert [repr(float(t)) for t in NC.TAPS[:6]] == [repr(float(f32(x))) for x in (0.00102838012, 0.00759875821, 0.0360007733, 0.109360687, 0.213005543, 0.266011715)]
    for name in ("compare_opts", "compare_workspace_bytes", "compare_images", "compare_summary"):
        assert callable(getattr(rbrt_amd, name))
    # the workspace: a record of 48 bytes a tile, nothing where the call would refuse the size
    for (w, h), tiles in (((1, 1), 1), ((16, 16), 1), ((17, 16), 2), ((16, 17), 2), ((33, 47), 9), ((1024, 768), 64 * 48), ((1, 8200), 513)):
        assert rbrt_amd.compare_workspace_bytes(w, h) == 48 * tiles, (w, h)
    for w, h in ((0, 5), (5, 0), (1 << 16, 1 << 15), (1 << 31, 1)):
        assert rbrt_amd.compare_workspace_bytes(w, h) == 0, (w, h)
    assert rbrt_amd.compare_workspace_bytes((1 << 31) - 1, 1) == 48 * (1 << 27)


def same_double(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b) or (math.isnan(a) and math.isnan(b))


def test_the_summary_makes_the_same_divisions_as_python():
    rng = np.random.default_rng(5)
    rows = [(1.5, 2.25, 0.125, 700.0, 0.5, 1000, 24, 32, 32, 1.0), (0.0, 0.0, 0.0, 1551.0, 0.0, 1551, 0, 33, 47, 1.0),  # mse 0: psnr +inf
            (0.0, 0.0, 0.0, 12.0, 0.0, 0, 1551, 33, 47, 1.0),                                                      # nothing usable: all NaN
            (float("inf"), 3e21, float("inf"), 1400.0, 1e25, 1551, 0, 33, 47, 1.0), (1e-300, 1e-200, 1e-100, -3.0, 1e-30, 1, 0, 1, 1, 255.0)]
    for _ in range(40):
        w, h = int(rng.integers(1, 3000)), int(rng.integers(1, 3000))
        usable = int(rng.integers(1, w * h + 1))
        rows.append((float(rng.uniform(0, 1e4)), float(rng.uniform(0, 1e4)), float(rng.uniform(0, 1e4)), float(rng.uniform(-1, 1) * w * h), float(rng.uniform(0, 50)),
                     usable, w * h - usable, w, h, float(rng.choice([1.0, 255.0, 0.5, 12.5]))))
    for se, ae, rel, ssim, mx, usable, skipped, w, h, peak in rows:
        r = abi.CompareResult(se, ae, rel, ssim, mx, usable, skipped, (0,) * 5)
        got = rbrt_amd.compare_summary(r, w, h, peak)
        exp = NC.summary(SimpleNamespace(sum_se=se, sum_ae=ae, sum_rel=rel, sum_ssim=ssim, usable=usable), w, h, peak)
        for k in ("mse", "mae", "relmse", "psnr_db", "ssim"):
            assert same_double(getattr(got, k), exp[k]), (k, getattr(got, k), exp[k], usable, w, h)
        if usable == 0:
            assert all(math.isnan(getattr(got, k)) for k in ("mse", "mae", "relmse", "psnr_db", "ssim"))
        else:  # the divisions themselves, written out
            n = 3.0 * usable
            assert same_double(got.mse, se / n) and same_double(got.mae, ae / n) and same_double(got.relmse, rel / n) and same_double(got.ssim, ssim / (float(w) * float(h)))
            if se == 0.0:
                assert got.psnr_db == math.inf and got.mse == 0.0
            elif math.isfinite(se):
                assert same_double(got.psnr_db, 10.0 * math.log10((peak * peak) / (se / n)))
    out = abi.CompareSummary(1.0, 2.0, 3.0, 4.0, 5.0)
    abi.load_hip().rbrt_compare_summary(None, 4, 4, 1.0, C.byref(out))  # a NULL result: nothing usable
    assert all(math.isnan(getattr(out, k)) for k in ("mse", "mae", "relmse", "psnr_db", "ssim"))
    abi.load_hip().rbrt_compare_summary(C.byref(abi.CompareResult()), 4, 4, 1.0, None)  # a NULL out is ignored
