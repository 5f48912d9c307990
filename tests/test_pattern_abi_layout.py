"""The solid-pattern additions to the C ABI, without a GPU: rbrt_pattern_t and rbrt_scene_patterns_t have the layout a C
compiler gives include/rbrt_hip.h in their ctypes mirrors (rbrt_amd/abi.py), the new entry points and the test hook are in
the symbol tables and in the library, and the ABI version stays 2."""
import ctypes as C
import subprocess
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent


def test_pattern_layout_matches_the_c_header(tmp_path):
    structs = {"rbrt_pattern_t": abi.Pattern, "rbrt_scene_patterns_t": abi.ScenePatterns}
    lines = ['printf("NONE %u\\n", RBRT_PATTERN_NONE);', 'printf("CHECKER %u\\n", RBRT_PATTERN_CHECKER);']
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\n#include "rbrt_hip_debug.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "pt.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "pt"), str(tmp_path / "pt.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "pt")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert C.sizeof(abi.Pattern) == 32 and C.sizeof(abi.ScenePatterns) == 16
    assert abi.Pattern.albedo2.offset == 4 and abi.Pattern.origin.offset == 16 and abi.Pattern.size.offset == 28
    assert int(got["NONE"]) == abi.PATTERN_NONE == 0 and int(got["CHECKER"]) == abi.PATTERN_CHECKER == 1


def test_the_symbols_are_declared_and_exported():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_hip_scene_create_patterned", "rbrt_hip_render_patterned"):
        assert name in abi.HIP_SYMBOLS and getattr(lib, name) is not None
    assert "rbrt_hip_debug_surface_albedo" in abi.DEBUG_SYMBOLS and lib.rbrt_hip_debug_surface_albedo is not None
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    for name in ("rbrt_hip_scene_create_patterned", "rbrt_hip_render_patterned", "rbrt_scene_patterns_t"):
        assert name in header
    assert "rbrt_hip_debug_surface_albedo" in (ROOT / "include" / "rbrt_hip_debug.h").read_text()
    rust = (ROOT / "integration" / "rust" / "hip_ffi.rs").read_text()
    assert "rbrt_hip_scene_create_patterned" in rust and "rbrt_hip_render_patterned" in rust and "RbrtScenePatterns" in rust


def test_a_checker_helper_fills_the_struct():
    p = abi.checker((0.8, 0.7, 0.6), 0.3, (1.0, 2.0, 3.0))
    assert p.kind == abi.PATTERN_CHECKER and list(p.origin) == [1.0, 2.0, 3.0] and abs(p.size - 0.3) < 1e-7
    sc = abi.SceneData(spheres=[((0, 0, -5), 1.0, abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5)))] * 3, patterns={1: p})
    assert sc.patterns.n_objects == 3 and sc.patterns.reserved == 0
    assert [sc.patterns.objects[i].kind for i in range(3)] == [0, 1, 0]
    assert abi.SceneData(spheres=[((0, 0, -5), 1.0, abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5)))]).patterns_ptr() is None
