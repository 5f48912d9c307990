"""Moving meshes in the C++ host, without a GPU: the per-mesh YAML key and its load errors, the shipped scene and its model,
the checkpoint fingerprint, and the command line's --no-motion. (What needs a render -- the report's list, the images with and
without --no-motion, the frames -- is in test_mesh_motion_gpu.py.)"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rbrt_amd import abi, standin

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "motion" / "moving_mesh.yaml"
OBJ = ROOT / "scenes" / "motion" / "moving_mesh.obj"
f32 = np.float32

SCENE_YAML = """---
camera_blueprint:
  camera_up: {{x: 0.0, y: 1.0, z: 0.0}}
  camera_look_at: {{x: 0.0, y: -0.1, z: -1.0}}
  camera_position: {{x: 0.0, y: 2.0, z: 4.0}}
  camera_focal_length_mm: 35.0
mesh_blueprints:
  - obj_filepath: {obj}
    scale: 10.0
{first}    translation: {{x: {tx}, y: 0.0, z: -6.0}}
    rotation_rad: {{x: 0.0, y: 0.0, z: 0.0}}
    material_type: "lambertian"
    albedo: {{x: 0.5, y: 0.5, z: 0.5}}
  - obj_filepath: {obj}
    scale: 8.0
{second}    translation: {{x: 2.0, y: 0.0, z: -5.0}}
    rotation_rad: {{x: 0.0, y: 0.0, z: 0.0}}
    material_type: "metal"
    albedo: {{x: 0.8, y: 0.8, z: 0.8}}
    material_param: 0.1
sphere_blueprints:
  - radius: 1000.0
    center: {{x: 0.0, y: -1000.0, z: -5.0}}
    material_type: "lambertian"
    albedo: {{x: 0.5, y: 0.5, z: 0.5}}
  - radius: 0.5
{sphere}    center: {{x: -2.0, y: 0.5, z: -6.0}}
    material_type: "lambertian"
    albedo: {{x: 0.5, y: 0.5, z: 0.5}}
"""


def _yaml(tmp_path, name, first=None, second=None, sphere=None, tx="0.0"):
    key = lambda v: "" if v is None else f"    shutter_travel: {v}\n"  # noqa: E731
    p = tmp_path / f"{name}.yaml"
    p.write_text(SCENE_YAML.format(obj=OBJ, first=key(first), second=key(second), sphere=key(sphere), tx=tx))
    return p


@pytest.mark.parametrize("text,want", [("[0.25, -0.5, 1.0e-3]", (0.25, -0.5, 1.0e-3)), ("[0, 0, 0]", (0.0, 0.0, 0.0)),
                                       ("{x: 1.5, y: 2.5, z: -3.5}", (1.5, 2.5, -3.5))])
def test_the_yaml_key(tmp_path, text, want):
    hs = abi.HostScene(_yaml(tmp_path, "key", second=text), 24, 32)
    assert hs.mesh_motion is not None and hs.mesh_motion.shape == (2, 3) and hs.mesh_motion.dtype == f32
    assert np.array_equal(hs.mesh_motion[1], np.array(want, f32))  # (a zero travel is a mesh motion, too: it draws)
    assert not hs.mesh_motion[0].any()                             # (the mesh without the key stays)
    assert hs.motion is None                                       # (HostScene.motion keeps its meaning: the spheres' keys only)
    plain = abi.HostScene(_yaml(tmp_path, "plain"), 24, 32)
    assert plain.mesh_motion is None and plain.motion is None
    # (the mesh as loaded is the mesh at the opening: the key moves nothing in the scene itself)
    for m in range(2):
        a, b = hs.struct.meshes[m], plain.struct.meshes[m]
        assert a.n_total == b.n_total and list(a.bbox_lo) == list(b.bbox_lo) and list(a.bbox_hi) == list(b.bbox_hi)
        assert np.array_equal(np.ctypeslib.as_array(a.v0x, (a.n_total,)), np.ctypeslib.as_array(b.v0x, (b.n_total,)))
    both = abi.HostScene(_yaml(tmp_path, "both", first="[1, 0, 0]", second=text, sphere="[0, 0, 2]"), 24, 32)
    assert np.array_equal(both.mesh_motion[0], np.array((1.0, 0.0, 0.0), f32)) and np.array_equal(both.mesh_motion[1], np.array(want, f32))
    assert both.motion is not None and np.array_equal(both.motion[1], np.array((0.0, 0.0, 2.0), f32))  # (each set of keys on its own)
    only_sphere = abi.HostScene(_yaml(tmp_path, "sphere", sphere="[0, 0, 2]"), 24, 32)
    assert only_sphere.mesh_motion is None and only_sphere.motion is not None


@pytest.mark.parametrize("text", ["[0.1, .nan, 0.0]", "[.inf, 0, 0]", "[0, 0, -.inf]", "[1, 2]", "[1, 2, 3, 4]", "0.5", "[a, b, c]"])
def test_a_bad_travel_is_a_load_error_that_names_the_mesh(tmp_path, text):
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(_yaml(tmp_path, "bad", second=text), 24, 32)
    assert "shutter_travel" in str(e.value) and "camera_shutter_travel" not in str(e.value) and "mesh 1" in str(e.value)


def test_a_travel_that_leaves_float32_is_a_load_error(tmp_path):
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(_yaml(tmp_path, "far", first="[3.0e38, 0, 0]", tx="3.0e38"), 24, 32)
    assert "box + shutter_travel of mesh 0 is not finite" in str(e.value)
    ok = abi.HostScene(_yaml(tmp_path, "near", first="[-3.0e38, 0, 0]", tx="3.0e38"), 24, 32)
    assert ok.mesh_motion[0, 0] == f32(-3.0e38)


def test_the_shipped_scene_and_its_model():
    hs = abi.HostScene(CFG, 24, 32)
    assert hs.shutter_travel is None and hs.motion is None  # (a static camera, and the spheres stay)
    assert hs.struct.n_meshes == 1 and np.array_equal(hs.mesh_motion, np.array([(1.5, 0.0, 0.0)], f32))
    spheres = abi.HostScene(ROOT / "scenes" / "motion" / "moving_spheres.yaml", 24, 32)
    assert spheres.struct.n_spheres == hs.struct.n_spheres
    for i in range(hs.struct.n_spheres):  # the row of spheres
        assert bytes(hs.struct.spheres[i]) == bytes(spheres.struct.spheres[i])
    # the model is the stand-in generator's, a few hundred triangles and a few KB
    assert 1000 < OBJ.stat().st_size < 16 * 1024
    v, f = standin.make_mesh(300)
    lines = OBJ.read_text().splitlines()
    assert sum(ln.startswith("f ") for ln in lines) == 300 == hs.struct.meshes[0].n_real
    got_v = np.array([[float(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("v ")], f32)
    got_f = np.array([[int(x) for x in ln.split()[1:]] for ln in lines if ln.startswith("f ")], np.int32) - 1
    assert np.array_equal(got_v, v) and np.array_equal(got_f, f)
    # it crosses the view: the camera looks down -z and the travel is along +x, through the image's middle column
    lo, hi = np.array(list(hs.struct.meshes[0].bbox_lo)), np.array(list(hs.struct.meshes[0].bbox_hi))
    assert lo[0] < 0.0 and hi[2] < float(hs.camera.position[2]) and hs.mesh_motion[0, 0] > 0.0
    for doc in ("README.md",):
        text = (ROOT / doc).read_text()
        assert "scenes/motion/moving_mesh.yaml" in text and "rbrt_amd.standin scenes/motion/moving_mesh.obj" in text


def test_checkpoint_fingerprint():
    h = 0x1234ABCD5678
    assert abi.mesh_motion_fingerprint(None, h) == h  # a scene none of whose meshes has the key keeps its fingerprint's bytes
    tv = np.array([(0.0, 0.0, 0.0), (0.002, 0.0, 0.0)], f32)
    a = abi.mesh_motion_fingerprint(tv, h)
    assert a != h and a == abi.mesh_motion_fingerprint(tv.copy(), h)
    assert abi.mesh_motion_fingerprint(tv[::-1], h) != a          # (which mesh moves)
    assert abi.mesh_motion_fingerprint(tv, h + 1) != a
    nxt = tv.copy()
    nxt[1, 0] = np.nextafter(f32(0.002), f32(1.0))
    assert abi.mesh_motion_fingerprint(nxt, h) != a
    zero = abi.mesh_motion_fingerprint(np.zeros((2, 3), f32), h)
    assert zero != h and zero != a  # (an all-zero mesh motion draws: its sums are not the motionless render's)
    assert abi.mesh_motion_fingerprint(np.zeros((3, 3), f32), h) != zero
    # the same numbers as a sphere motion, a mesh motion and a shutter never share a checkpoint
    assert len({a, abi.motion_fingerprint(tv, h), abi.shutter_fingerprint((0.002, 0.0, 0.0), h)}) == 3
    assert abi.motion_fingerprint(tv, h) == abi.motion_fingerprint(tv, h)  # (the spheres' part is what it was: test_motion_host.py)


def test_no_motion_covers_the_meshes_keys_in_the_documents():
    """(The --help text is a recorded yardstick and stays as it is: the flag's reach is described in the README, DESIGN.md
    section 27 and the shipped scene's header.)"""
    for doc in ("README.md", "DESIGN.md", "scenes/motion/moving_mesh.yaml"):
        assert "--no-motion" in (ROOT / doc).read_text(), doc
    r = subprocess.run([str(EXE), "-c", str(CFG), "-t", "unused.png", "--no-motion=1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--no-motion" in r.stderr, (r.returncode, r.stderr[-500:])
