"""The display transform's additions to the C ABI, without a GPU: rbrt_tonemap_opts_t and rbrt_tonemap_result_t have the layout
a C compiler gives include/rbrt_hip.h in their ctypes mirrors (rbrt_amd/abi.py), the defines of both headers are the numbers
abi.py has, the entry points are in the symbol table, and the ABI version stays 2."""
import ctypes as C
import subprocess
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
DEFINES = {"RBRT_TONE_LINEAR": abi.TONE_LINEAR, "RBRT_TONE_REINHARD": abi.TONE_REINHARD, "RBRT_TONE_ACES": abi.TONE_ACES,
           "RBRT_TONEMAP_BINS": abi.TONEMAP_BINS, "RBRT_TONEMAP_RESULT_OFFSET": abi.TONEMAP_RESULT_OFFSET,
           "RBRT_TONEMAP_WORKSPACE_BYTES": abi.TONEMAP_WORKSPACE_BYTES, "RBRT_TONEMAP_BLOCK_PIXELS": abi.TONEMAP_BLOCK_PIXELS,
           "RBRT_TONEMAP_MAX_BLOCKS": abi.TONEMAP_MAX_BLOCKS}


def test_tonemap_layout_matches_the_c_headers(tmp_path):
    structs = {"rbrt_tonemap_opts_t": abi.TonemapOpts, "rbrt_tonemap_result_t": abi.TonemapResult}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += [f'printf("{d} %lu\\n", (unsigned long)({d}));' for d in DEFINES]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip_debug.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "tm.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "tm"), str(tmp_path / "tm.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "tm")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    for d, value in DEFINES.items():
        assert int(got[d]) == value, d
    assert C.sizeof(abi.TonemapOpts) == 32 and C.sizeof(abi.TonemapResult) == 32
    assert abi.TONEMAP_WORKSPACE_BYTES == abi.TONEMAP_BINS * 4 + C.sizeof(abi.TonemapResult)
    assert abi.TonemapResult.pixels.offset == 24 and abi.TonemapResult.counted.offset == 16
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_hip_tonemap", "rbrt_tonemap_opts_default"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    d = abi.TonemapOpts(9, 9, 9, 9, 9, 9, (9, 9))
    lib.rbrt_tonemap_opts_default(C.byref(d))
    assert (d.curve, d.exposure, d.key_permille, d.white, d.white_permille, list(d.reserved)) == (0, 1.0, 500, 0.0, 990, [0, 0])
    assert d.key == C.c_float(0.18).value
