"""Emissive materials and the constant background: what the host side decides without a GPU (the C ABI's constants and
argument checks, the YAML factory, the CLI's --background)."""
from __future__ import annotations

import ctypes as C
import math
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"


def test_header_and_abi_py_agree_on_the_new_constants():
    h = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert re.search(r"\bRBRT_MAT_EMISSIVE\s*=\s*3\b", h)
    assert re.search(r"#define\s+RBRT_FLAG_CONSTANT_BACKGROUND\s+2u\b", h)
    assert re.search(r"#define\s+RBRT_ABI_VERSION\s+2\b", h)
    assert abi.MAT_EMISSIVE == 3 and abi.FLAG_CONSTANT_BACKGROUND == 2
    o = abi.default_opts(flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.25, 1.5))
    assert o.flags == 2 and list(o.bg) == [0.0, 0.25, 1.5]
    m = abi.material(abi.MAT_EMISSIVE, (2.0, 1.0, 0.5))
    assert m.kind == 3 and list(m.albedo) == [2.0, 1.0, 0.5]


def _create(scene: abi.SceneData):
    """rbrt_hip_scene_create's status (a handle it made is destroyed again)."""
    lib = abi.load_hip()
    h = C.c_void_p()
    rc = lib.rbrt_hip_scene_create(scene.ptr(), 0, C.byref(h))
    if rc == abi.RBRT_OK:
        lib.rbrt_hip_scene_destroy(h)
    return rc, lib.rbrt_hip_last_error().decode(errors="replace")


def _lamp_scenes(L):
    em = abi.material(abi.MAT_EMISSIVE, L)
    lam = abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5))
    tri = (((-1, 0, -3), (1, 0, -3), (0, 1, -3)), em)
    return {
        "sphere": abi.SceneData(spheres=[((0, 0, -5), 1.0, lam), ((0, 3, -5), 1.0, em)]),
        "triangle": abi.SceneData(spheres=[((0, 0, -5), 1.0, lam)], triangles=[tri]),
    }


def test_an_emitter_is_accepted():
    for what, sc in _lamp_scenes((1.0, 1.0, 1.0)).items():
        rc, _ = _create(sc)
        # no device here: NO_DEVICE; on a GPU box: OK. Never INVALID_ARG (which is what a library without the kind answers)
        assert rc in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE), (what, rc)
    rc, _ = _create(abi.SceneData(spheres=[((0, 0, -5), 1.0, abi.material(abi.MAT_EMISSIVE, (0.0, 7.5, 1e30)))]))
    assert rc in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE)


@pytest.mark.parametrize("L", [(math.nan, 1.0, 1.0), (1.0, math.inf, 1.0), (1.0, 1.0, -math.inf), (-0.5, 1.0, 1.0),
                               (1.0, 1.0, -1e-30)])
def test_a_bad_radiance_is_refused_before_the_device(L):
    for what, sc in _lamp_scenes(L).items():
        rc, msg = _create(sc)
        assert rc == abi.RBRT_ERR_INVALID_ARG and "emissive" in msg and what in msg, (what, rc, msg)
        # the one-shot call checks the scene the same way, before it touches a device
        from oracle import pyoracle
        cam = pyoracle.camera_new((0, 0, 0), (0, 0, -1), (0, 1, 0), 8, 8, 28.0)
        rgb = np.zeros((8, 8, 3), np.uint8)
        opts = abi.default_opts(spp=1, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0, 0, 0))
        rc = abi.load_hip().rbrt_hip_render(C.byref(cam), sc.ptr(), C.byref(opts), None, rgb.ctypes.data_as(abi.u8p))
        assert rc == abi.RBRT_ERR_INVALID_ARG, (what, rc)


def test_unknown_kinds_are_still_refused():
    for kind in (4, 7, -1):
        rc, msg = _create(abi.SceneData(spheres=[((0, 0, -5), 1.0, abi.material(kind, (1, 1, 1)))]))
        assert rc == abi.RBRT_ERR_INVALID_ARG and "unknown material kind" in msg, kind


YAML = """
camera_blueprint:
  camera_up: {x: 0.0, y: 1, z: 0}
  camera_look_at: {x: 0, y: 0, z: -1}
  camera_position: {x: 0, y: 0, z: 0}
  camera_focal_length_mm: 35
mesh_blueprints: []
sphere_blueprints:
- radius: 1
  center: {x: 0, y: 0, z: -5}
  material_type: "Emissive"
  albedo: {x: 4.0, y: 2.5, z: 0.25}
  material_param: 9.0
- radius: 2
  center: {x: 0, y: 3, z: -9}
  material_type: "emissive metal"
  albedo: {x: 0.5, y: 0.5, z: 0.5}
  material_param: 0.1
"""


def test_yaml_emissive_material(tmp_path):
    (tmp_path / "s.yaml").write_text(YAML)
    hs = abi.HostScene(tmp_path / "s.yaml", 10, 10)
    assert hs.struct.n_spheres == 2
    m = hs.struct.spheres[0].mat
    assert m.kind == abi.MAT_EMISSIVE and list(m.albedo) == [np.float32(4.0), np.float32(2.5), np.float32(0.25)]
    assert hs.struct.spheres[1].mat.kind == abi.MAT_METAL  # metal is matched first, as in the reference's factory


def test_yaml_emissive_needs_an_albedo(tmp_path):
    (tmp_path / "s.yaml").write_text(YAML.replace("  albedo: {x: 4.0, y: 2.5, z: 0.25}\n", ""))
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(tmp_path / "s.yaml", 10, 10)
    assert "you forgot to specify an albedo vector (the emitted radiance) for emissive" in str(e.value)


def test_shipped_emissive_scene_parses():
    hs = abi.HostScene(ROOT / "scenes" / "emissive_spheres.yaml", 24, 32)
    kinds = [hs.struct.spheres[i].mat.kind for i in range(hs.struct.n_spheres)]
    assert hs.struct.n_meshes == 0 and kinds.count(abi.MAT_EMISSIVE) >= 1


def test_cli_background_flag(tmp_path):
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--background <r,g,b>" in r.stdout
    for bad in ("1,2", "1,2,3,4", "a,b,c", "1,,2", "0,0,-1", "nan,0,0", "0,inf,0", ""):
        for argv in (["--background", bad], [f"--background={bad}"]):
            r = subprocess.run([str(EXE), *argv, "-t", str(tmp_path / "x.png")], capture_output=True, text=True)
            assert r.returncode == 2 and "--background" in r.stderr, (argv, r.returncode, r.stderr)
    r = subprocess.run([str(EXE), "--background"], capture_output=True, text=True)
    assert r.returncode == 2
