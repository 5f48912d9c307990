"""Solid patterns at the boundary and in the C++ host, without a GPU: every pattern argument the library refuses before it
touches a device, the YAML keys and their refusals, the patterns a loaded scene hands on, and the CLI on the shipped
scene."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
SHIPPED = ROOT / "scenes" / "checker" / "checker_ground.yaml"
f32 = np.float32
L, M, D, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE


def _cam():
    cam = abi.Camera()
    cam.position, cam.right, cam.up, cam.img_center_point = abi._f3((0, 0, 0)), abi._f3((1, 0, 0)), abi._f3((0, 1, 0)), abi._f3((0, 0, -1))
    cam.mm_per_pix_hor = cam.mm_per_pix_vert = 0.5
    cam.img_width_pix, cam.img_height_pix = 8, 8
    return cam


def _scene(kinds=(L, M, D, EM), n_extra=0):
    spheres = [((float(i), 0.0, -5.0), 0.4, abi.material(k, (0.5, 0.5, 0.5), 1.5 if k == D else 0.1)) for i, k in enumerate(kinds)]
    spheres += [((0.0, float(i), -9.0), 0.1, abi.material(L, (0.5, 0.5, 0.5))) for i in range(n_extra)]
    tri = [(((-1, 0, -4), (1, 0, -4), (0, 1, -4)), abi.material(L, (0.3, 0.3, 0.3)))]
    return abi.SceneData(spheres=spheres, triangles=tri)


def _patterns(sc, pats, n_objects=None, reserved=0):
    n = len(sc.spheres) + len(sc.triangles) + len(sc.meshes)
    arr = (abi.Pattern * n)()
    for k, p in pats.items():
        arr[k] = p
    return abi.ScenePatterns(n if n_objects is None else n_objects, reserved, arr), arr


def _both_calls(sc, pt):
    """The return codes of rbrt_hip_scene_create_patterned and rbrt_hip_render_patterned, and the last message."""
    lib = abi.load_hip()
    h = C.c_void_p()
    rc1 = lib.rbrt_hip_scene_create_patterned(sc.ptr(), None, C.byref(pt), 0, C.byref(h))
    msg = lib.rbrt_hip_last_error()
    if rc1 == abi.RBRT_OK:
        lib.rbrt_hip_scene_destroy(h)
    cam, rad, opts = _cam(), np.zeros((8, 8, 3), f32), abi.default_opts(spp=1)
    rc2 = lib.rbrt_hip_render_patterned(C.byref(cam), sc.ptr(), None, C.byref(pt), C.byref(opts), rad.ctypes.data_as(abi.f32p), None)
    return rc1, rc2, msg


GOOD = dict(albedo2=(0.8, 0.7, 0.6), size=0.3, origin=(0.1, 0.2, 0.3))


def _bad(**kw):
    d = dict(GOOD)
    d.update(kw)
    return abi.checker(d["albedo2"], d["size"], d["origin"])


CASES = {
    "n_objects": lambda sc: _patterns(sc, {0: _bad()}, n_objects=4),
    "reserved": lambda sc: _patterns(sc, {0: _bad()}, reserved=1),
    "unknown_kind": lambda sc: _patterns(sc, {0: abi.Pattern(2, abi._f3(GOOD["albedo2"]), abi._f3(GOOD["origin"]), 0.3)}),
    "on_metal": lambda sc: _patterns(sc, {1: _bad()}),
    "on_dielectric": lambda sc: _patterns(sc, {2: _bad()}),
    "on_emissive": lambda sc: _patterns(sc, {3: _bad()}),
    "size_zero": lambda sc: _patterns(sc, {0: _bad(size=0.0)}),
    "size_negative": lambda sc: _patterns(sc, {4: _bad(size=-1.0)}),
    "size_nan": lambda sc: _patterns(sc, {0: _bad(size=float("nan"))}),
    "size_inf": lambda sc: _patterns(sc, {0: _bad(size=float("inf"))}),
    "size_whose_inverse_overflows": lambda sc: _patterns(sc, {0: _bad(size=1e-39)}),
    "origin_nan": lambda sc: _patterns(sc, {0: _bad(origin=(0.0, float("nan"), 0.0))}),
    "origin_inf": lambda sc: _patterns(sc, {4: _bad(origin=(float("-inf"), 0.0, 0.0))}),
    "albedo2_nan": lambda sc: _patterns(sc, {0: _bad(albedo2=(0.5, 0.5, float("nan")))}),
    "albedo2_inf": lambda sc: _patterns(sc, {0: _bad(albedo2=(float("inf"), 0.5, 0.5))}),
    "albedo2_negative": lambda sc: _patterns(sc, {0: _bad(albedo2=(0.5, -0.001, 0.5))}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_invalid_pattern_arguments_are_refused_before_the_device(case):
    sc = _scene()
    pt, _keep = CASES[case](sc)
    rc1, rc2, msg = _both_calls(sc, pt)
    assert rc1 == abi.RBRT_ERR_INVALID_ARG and rc2 == abi.RBRT_ERR_INVALID_ARG, (rc1, rc2, msg)
    assert b"patterns" in msg


def test_the_record_byte_limits_objects_plus_patterns():
    """Entry numbers are bytes: 256 objects and patterned objects together fit, 257 do not; 255 objects stays the scene's limit."""
    sc = _scene(kinds=(L,), n_extra=198)  # 199 spheres + 1 triangle = 200 objects
    assert len(sc.spheres) + len(sc.triangles) == 200
    pt, _keep = _patterns(sc, {k: _bad() for k in range(57)})
    rc1, rc2, msg = _both_calls(sc, pt)
    assert rc1 == abi.RBRT_ERR_UNSUPPORTED and rc2 == abi.RBRT_ERR_UNSUPPORTED and b"256" in msg
    pt, _keep = _patterns(sc, {k: _bad() for k in range(56)})
    rc1, rc2, msg = _both_calls(sc, pt)
    assert rc1 in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE) and rc2 in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE), msg


def test_valid_patterns_are_no_argument_error():
    """A checker on a lambertian sphere and on a lambertian triangle, no objects array, kinds all NONE, NULL: accepted."""
    lib = abi.load_hip()
    sc = _scene()
    n = 5
    for pt in (_patterns(sc, {0: _bad(), 4: _bad(size=1e9)})[0], abi.ScenePatterns(n, 0, None), _patterns(sc, {})[0], None):
        h = C.c_void_p()
        rc = lib.rbrt_hip_scene_create_patterned(sc.ptr(), None, None if pt is None else C.byref(pt), 0, C.byref(h))
        assert rc in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE), lib.rbrt_hip_last_error()
        if rc == abi.RBRT_OK:
            lib.rbrt_hip_scene_destroy(h)


# ---- YAML --------------------------------------------------------------------------------------------------------------
YAML = """---
camera_blueprint:
  camera_up: {{x: 0.0, y: 1.0, z: -0.4}}
  camera_look_at: {{x: 0.0, y: -0.1, z: -1.0}}
  camera_position: {{x: 0.0, y: 5.0, z: 4.0}}
  camera_focal_length_mm: 28.0
mesh_blueprints:
{mesh}sphere_blueprints:
  - radius: 1.5
    center: {{x: -5.0, y: 1.5, z: -9.0}}
    material_type: "metal"
    material_param: 0.1
    albedo: {{x: 0.1, y: 0.1, z: 0.9}}
  - radius: 1000.0
    center: {{x: 0.0, y: -1000.0, z: -5.0}}
    material_type: "{mat}"
    material_param: 1.5
    albedo: {{x: 0.02, y: 0.2, z: 0.1}}
{keys}"""

MESH = """  - obj_filepath: {obj}
    scale: 1.0
    translation: {{x: 0.5, y: 1.0, z: -9.0}}
    rotation_rad: {{x: 0.0, y: 0.0, z: 0.0}}
    material_type: "lambertian"
    albedo: {{x: 0.8, y: 0.8, z: 0.8}}
    checker_albedo: {{x: 0.1, y: 0.2, z: 0.3}}
    checker_size: 0.25
"""


def _yaml(tmp_path, keys, mat="lambertian", mesh=False):
    m = " []\n"
    if mesh:
        obj = tmp_path / "t.obj"
        obj.write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
        m = "\n" + MESH.format(obj=obj)
    p = tmp_path / "s.yaml"
    text = YAML.format(mat=mat, keys=keys, mesh="@@")
    p.write_text(text.replace("mesh_blueprints:\n@@", "mesh_blueprints:" + m))
    return p


FULL = "    checker_albedo: {x: 0.8, y: 0.7, z: 0.6}\n    checker_size: 0.3\n    checker_origin: {x: 0.1, y: -0.15, z: 0.2}\n"


def test_yaml_keys_become_patterns_by_object_id(tmp_path):
    hs = abi.HostScene(_yaml(tmp_path, FULL, mesh=True), 24, 32)
    pt = hs.patterns
    assert pt is not None and pt.n_objects == 3 and pt.reserved == 0  # two spheres, then the mesh
    assert pt.objects[0].kind == abi.PATTERN_NONE
    g, m = pt.objects[1], pt.objects[2]
    assert g.kind == abi.PATTERN_CHECKER and np.array_equal(np.array(list(g.albedo2), f32), np.array([0.8, 0.7, 0.6], f32))
    assert np.array_equal(np.array(list(g.origin), f32), np.array([0.1, -0.15, 0.2], f32)) and g.size == f32(0.3)
    assert m.kind == abi.PATTERN_CHECKER and list(m.origin) == [0.0, 0.0, 0.0] and m.size == 0.25  # checker_origin defaults to 0
    assert hs.patterns_ptr() is not None
    assert abi.HostScene(_yaml(tmp_path, ""), 24, 32).patterns is None


@pytest.mark.parametrize("keys, needle", [
    ("    checker_albedo: {x: 0.8, y: 0.7, z: 0.6}\n", "checker_size"),
    ("    checker_size: 0.3\n", "checker_albedo"),
    ("    checker_origin: {x: 0.0, y: 0.0, z: 0.0}\n", "checker_origin"),
    ("    checker_albedo: {x: 0.8, y: 0.7, z: 0.6}\n    checker_size: 0.0\n", "checker_size"),
    ("    checker_albedo: {x: 0.8, y: 0.7, z: 0.6}\n    checker_size: .inf\n", "checker_size"),
    ("    checker_albedo: {x: 0.8, y: -0.7, z: 0.6}\n    checker_size: 0.3\n", "checker_albedo"),
    ("    checker_albedo: {x: 0.8, y: 0.7}\n    checker_size: 0.3\n", "checker_albedo"),
    ("    checker_albedo: {x: 0.8, y: 0.7, z: 0.6}\n    checker_size: 0.3\n    checker_origin: {x: .nan, y: 0.0, z: 0.0}\n", "checker_origin"),
])
def test_yaml_refusals_name_the_key(tmp_path, keys, needle):
    with pytest.raises(RuntimeError, match=needle):
        abi.HostScene(_yaml(tmp_path, keys), 24, 32)


@pytest.mark.parametrize("mat", ["metal", "dielectric", "emissive"])
def test_yaml_refuses_a_checker_on_another_material(tmp_path, mat):
    with pytest.raises(RuntimeError, match="checker_albedo.*lambertian"):
        abi.HostScene(_yaml(tmp_path, FULL, mat=mat), 24, 32)


# ---- the shipped scene and the CLI --------------------------------------------------------------------------------------
def test_the_shipped_scene_loads_with_its_ground_half_a_cell_down():
    hs = abi.HostScene(SHIPPED, 24, 32)
    assert hs.struct.n_spheres == 4 and hs.struct.n_meshes == 0
    pt = hs.patterns
    assert pt.n_objects == 4 and [pt.objects[i].kind for i in range(4)] == [1, 0, 0, 0]
    g = pt.objects[0]
    assert g.origin[1] == -0.5 * g.size and g.size > 0  # the ground's surface (y near 0) is mid-cell, not on a boundary
    assert hs.struct.spheres[0].mat.kind == L and "bunny" not in SHIPPED.read_text().split("---")[1]
    assert "checker_ground.yaml" in (ROOT / "README.md").read_text()


def test_the_cli_parses_the_shipped_scene(tmp_path):
    """The scene gets through the CLI's loader: whatever ends the run (no device here, or nothing at all), it is not the YAML."""
    r = subprocess.run([str(EXE), "-c", str(SHIPPED), "-t", str(tmp_path / "o.png"), "--height", "8", "-w", "8", "-s", "1"],
                       capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "Unable to parse" not in out and "checker" not in out, out
    bad = tmp_path / "bad.yaml"
    bad.write_text(SHIPPED.read_text().replace("    checker_size: 2.0\n", ""))
    r = subprocess.run([str(EXE), "-c", str(bad), "-t", str(tmp_path / "o.png"), "--height", "8", "-w", "8", "-s", "1"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "checker_albedo needs checker_size" in r.stdout + r.stderr
