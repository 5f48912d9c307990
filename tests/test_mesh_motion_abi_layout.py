"""Moving meshes at the C boundary, without a GPU: rbrt_mesh_motion_t has the layout a C compiler gives the header, the
prototype in the header is the one abi.py binds, the symbol is exported, the ABI version stays 2, and the argument checks
that need no scene come back as codes."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent


def test_struct_layout_matches_the_c_header(tmp_path):
    cname, cls = "rbrt_mesh_motion_t", abi.MeshMotion
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "layout.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], check=True)
    out = subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 16
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert [f for f, _ in cls._fields_] == ["n_meshes", "reserved", "travel"]


def test_the_prototype_is_the_one_abi_py_binds():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "rbrt_hip.h").read_text(), flags=re.S)
    m = re.search(r"int\s+rbrt_hip_scene_set_mesh_motion\s*\(([^)]*)\)\s*;", header)
    assert m, "rbrt_hip_scene_set_mesh_motion is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["rbrt_hip_scene_t* scene", "const rbrt_mesh_motion_t* motion"]
    res, args = abi.HIP_SYMBOLS["rbrt_hip_scene_set_mesh_motion"]
    assert res is C.c_int and args == [C.c_void_p, C.POINTER(abi.MeshMotion)]
    # the struct as the issue states it: two words and a pointer to float
    body = re.search(r"typedef struct rbrt_mesh_motion \{(.*?)\} rbrt_mesh_motion_t;", header, flags=re.S).group(1)
    assert [" ".join(x.split()) for x in body.strip().split(";") if x.strip()] == ["uint32_t n_meshes", "uint32_t reserved", "const float* travel"]


def test_the_symbol_is_exported_and_the_abi_version_stays_2():
    lib = abi.load_hip()
    assert hasattr(lib, "rbrt_hip_scene_set_mesh_motion")
    assert lib.rbrt_hip_abi_version() == 2


def test_a_null_scene_is_refused_before_the_device_is_touched():
    lib = abi.load_hip()
    mo = abi.MeshMotion()
    assert lib.rbrt_hip_scene_set_mesh_motion(None, C.byref(mo)) == abi.RBRT_ERR_INVALID_ARG
    assert b"set_mesh_motion" in lib.rbrt_hip_last_error()
    assert lib.rbrt_hip_scene_set_mesh_motion(None, None) == abi.RBRT_ERR_INVALID_ARG


def test_the_header_no_longer_lists_meshes_as_not_built():
    text = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "Not built: moving meshes" not in text and "meshes and BasicTriangles do not move" not in text
    section = text[text.index("---- Moving meshes"):]
    section = section[:section.index("typedef struct rbrt_mesh_motion")]
    for phrase in ("moving BasicTriangles", "rotation", "a pattern that travels with its mesh", "a time argument for rbrt_hip_trace_rays"):
        assert phrase in section, phrase
