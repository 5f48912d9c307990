"""Spike removal's additions to the C ABI, without a GPU: rbrt_despike_opts_t and rbrt_despike_result_t have the layout a C
compiler gives include/rbrt_hip.h in their ctypes mirrors (rbrt_amd/abi.py), the entry points are in the symbol table, the ABI
version stays 2, the defaults are the header's, and the kernel's tile is the same in the debug header and in abi.py."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np

import despike_cases as DC
import np_despike
import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32


def test_struct_layouts_match_the_c_header(tmp_path):
    structs = {"rbrt_despike_opts_t": abi.DespikeOpts, "rbrt_despike_result_t": abi.DespikeResult}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "ds.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "ds"), str(tmp_path / "ds.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "ds")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, (cname, f)
    assert C.sizeof(abi.DespikeOpts) == 32 and C.sizeof(abi.DespikeResult) == 16
    assert [f for f, _ in abi.DespikeOpts._fields_] == ["radius", "rank", "threshold", "floor", "flags", "reserved"]
    assert [getattr(abi.DespikeOpts, f).offset for f, _ in abi.DespikeOpts._fields_] == [0, 4, 8, 12, 16, 20]
    assert [f for f, _ in abi.DespikeResult._fields_] == ["spikes_a", "spikes_b", "reserved"]
    assert [getattr(abi.DespikeResult, f).offset for f, _ in abi.DespikeResult._fields_] == [0, 4, 8]


def test_symbols_version_and_defaults():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_despike_opts_default", "rbrt_hip_despike_halves"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(abi.HIP_SYMBOLS["rbrt_hip_despike_halves"][1]) == 11
    d = abi.DespikeOpts(9, 9, 9.0, 9.0, 9, (9, 9, 9))
    lib.rbrt_despike_opts_default(C.byref(d))
    assert (d.radius, d.rank, d.threshold, d.floor, d.flags, list(d.reserved)) == (2, 2, f32(4.0), f32(0.01), 0, [0, 0, 0])
    lib.rbrt_despike_opts_default(None)  # (a NULL is ignored, as by the other *_default calls)
    assert np_despike.DEFAULTS == dict(radius=2, rank=2, threshold=4.0, floor=0.01)
    t = rbrt_amd.despike_opts(radius=1, threshold=2.5)
    assert (t.radius, t.rank, t.threshold, t.floor, t.flags) == (1, 2, f32(2.5), f32(0.01), 0)
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "int rbrt_hip_despike_halves(" in header and "void rbrt_despike_opts_default(" in header and "#define RBRT_ABI_VERSION 2" in header
    assert "#define RBRT_DESPIKE_MAX_RADIUS 2u" in header and abi.DESPIKE_MAX_RADIUS == np_despike.MAX_RADIUS == 2
    assert "#define RBRT_DESPIKE_MAX_RANK 4u" in header and abi.DESPIKE_MAX_RANK == np_despike.MAX_RANK == 4
    debug = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
    tw, th = (int(re.search(rf"#define RBRT_DESPIKE_TILE_{k} (\d+)u", debug).group(1)) for k in "WH")
    assert (tw, th) == (abi.DESPIKE_TILE_W, abi.DESPIKE_TILE_H) == (DC.TW, DC.TH) and tw * th == 256
    for name in ("despike_opts", "despike_halves"):
        assert callable(getattr(rbrt_amd, name))
