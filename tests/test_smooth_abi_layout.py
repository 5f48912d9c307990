"""The smooth-shading additions to the C ABI, without a GPU: rbrt_mesh_normals_t and rbrt_scene_shading_t have the layout
a C compiler gives include/rbrt_hip.h in their ctypes mirrors (rbrt_amd/abi.py), the new entry points are in the symbol
tables, and the ABI version stays 2 (rbrt_mesh_t and rbrt_scene_t are checked by test_abi_layout.py)."""
import ctypes as C
import subprocess
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent


def test_shading_layout_matches_the_c_header(tmp_path):
    structs = {"rbrt_mesh_normals_t": abi.MeshNormals, "rbrt_scene_shading_t": abi.SceneShading}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "sh.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "sh"), str(tmp_path / "sh.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "sh")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert C.sizeof(abi.MeshNormals) == 72 and C.sizeof(abi.SceneShading) == 16
    assert abi.load_hip().rbrt_hip_abi_version() == 2
    for name in ("rbrt_hip_scene_create_shaded", "rbrt_hip_render_shaded"):
        assert name in abi.HIP_SYMBOLS
    assert "rbrt_hip_debug_shading_normals" in abi.DEBUG_SYMBOLS
