"""The temporal accumulation's additions to the C ABI, without a GPU: rbrt_temporal_opts_t has the layout a C compiler gives
include/rbrt_hip.h in its ctypes mirror (rbrt_amd/abi.py), the entry points are in the symbol table, the ABI version stays 2,
the defaults are the header's, and rbrt_hip_temporal_history_bytes answers 48 bytes a pixel, or 0 for what the call refuses."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import np_temporal
import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def test_temporal_opts_layout_matches_the_c_header(tmp_path):
    cname, cls = "rbrt_temporal_opts_t", abi.TemporalOpts
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "tp.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "tp"), str(tmp_path / "tp.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "tp")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 32
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert [f for f, _ in cls._fields_] == ["max_history", "depth", "normal", "flags", "reserved"]
    assert [getattr(cls, f).offset for f, _ in cls._fields_] == [0, 4, 8, 12, 16]


def test_symbols_version_and_defaults():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_temporal_opts_default", "rbrt_hip_temporal_history_bytes", "rbrt_hip_temporal_accumulate"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(abi.HIP_SYMBOLS["rbrt_hip_temporal_accumulate"][1]) == 15
    d = abi.TemporalOpts(9.0, 9.0, 9.0, 9, (9, 9, 9, 9))
    lib.rbrt_temporal_opts_default(C.byref(d))
    assert (d.max_history, d.depth, d.normal, d.flags, list(d.reserved)) == (f32(32.0), f32(0.05), f32(0.35), 0, [0, 0, 0, 0])
    lib.rbrt_temporal_opts_default(None)  # (a NULL is ignored, as by the other *_default calls)
    assert np_temporal.DEFAULTS == dict(max_history=32.0, depth=0.05, normal=0.35)
    t = rbrt_amd.temporal_opts(max_history=8, normal=0.5)
    assert (t.max_history, t.depth, t.normal, t.flags) == (f32(8.0), f32(0.05), f32(0.5), 0)
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "int rbrt_hip_temporal_accumulate(" in header and "size_t rbrt_hip_temporal_history_bytes(" in header
    assert "#define RBRT_ABI_VERSION 2" in header
    block = re.search(r"#define RBRT_TEMPORAL_BLOCK (\d+)u", (ROOT / "include" / "rbrt_hip_debug.h").read_text())
    assert block and int(block.group(1)) == abi.TEMPORAL_BLOCK
    assert callable(rbrt_amd.temporal_accumulate)


def test_history_bytes():
    hb = rbrt_amd.temporal_history_bytes
    assert abi.TEMPORAL_HISTORY_BYTES_PER_PIXEL == 48
    assert hb(1, 1) == 48 and hb(37, 21) == 37 * 21 * 48 and hb(1024, 768) == 1024 * 768 * 48
    assert hb(0, 5) == 0 and hb(5, 0) == 0 and hb(0, 0) == 0
    assert hb(1 << 16, 1 << 15) == 0 and hb(1 << 31, 1) == 0       # 2^31 pixels: refused
    assert hb((1 << 31) - 1, 1) == ((1 << 31) - 1) * 48             # ... and one fewer is not
    h = np_temporal.History(*(np.zeros(s, f32) for s in ((21, 37, 3), (21, 37, 3), (21, 37), (21, 37, 3), (21, 37), (21, 37))))
    assert np_temporal.pack(h).nbytes == hb(37, 21)
