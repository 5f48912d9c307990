"""Moving spheres in the C++ host, without a GPU: the per-sphere YAML key and its refusals, the shipped scene, the checkpoint
fingerprint, and the command line's --no-motion. (What needs a render -- the report's list, the images with and without
--no-motion -- is in test_motion_gpu.py.)"""
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "motion" / "moving_spheres.yaml"
f32 = np.float32

SCENE_YAML = """---
camera_blueprint:
  camera_up: {{x: 0.0, y: 1.0, z: 0.0}}
  camera_look_at: {{x: 0.0, y: -0.1, z: -1.0}}
  camera_position: {{x: 0.0, y: 2.0, z: 4.0}}
  camera_focal_length_mm: 35.0
mesh_blueprints: []
sphere_blueprints:
  - radius: 1000.0
    center: {{x: 0.0, y: -1000.0, z: -5.0}}
    material_type: "lambertian"
    albedo: {{x: 0.5, y: 0.5, z: 0.5}}
  - radius: 1.0
{first}    center: {{x: {cx}, y: 1.0, z: -8.0}}
    material_type: "lambertian"
    albedo: {{x: 0.5, y: 0.5, z: 0.5}}
  - radius: 0.5
{second}    center: {{x: 2.0, y: 0.5, z: -6.0}}
    material_type: "metal"
    albedo: {{x: 0.8, y: 0.8, z: 0.8}}
    material_param: 0.1
"""


def _yaml(tmp_path, name, first=None, second=None, cx="0.0"):
    key = lambda v: "" if v is None else f"    shutter_travel: {v}\n"  # noqa: E731
    p = tmp_path / f"{name}.yaml"
    p.write_text(SCENE_YAML.format(first=key(first), second=key(second), cx=cx))
    return p


@pytest.mark.parametrize("text,want", [("[0.25, -0.5, 1.0e-3]", (0.25, -0.5, 1.0e-3)), ("[0, 0, 0]", (0.0, 0.0, 0.0)),
                                       ("{x: 1.5, y: 2.5, z: -3.5}", (1.5, 2.5, -3.5))])
def test_the_yaml_key(tmp_path, text, want):
    hs = abi.HostScene(_yaml(tmp_path, "key", second=text), 24, 32)
    assert hs.motion is not None and hs.motion.shape == (3, 3) and hs.motion.dtype == f32
    assert np.array_equal(hs.motion[2], np.array(want, f32))  # (a zero travel is a motion, too: it draws)
    assert not hs.motion[:2].any()                            # (the spheres without the key stay)
    plain = abi.HostScene(_yaml(tmp_path, "plain"), 24, 32)
    assert plain.motion is None
    # (`center` is the sphere at the opening: the key moves nothing in the scene itself)
    for i in range(3):
        assert bytes(hs.struct.spheres[i]) == bytes(plain.struct.spheres[i])
    both = abi.HostScene(_yaml(tmp_path, "both", first="[1, 0, 0]", second=text), 24, 32)
    assert np.array_equal(both.motion[1], np.array((1.0, 0.0, 0.0), f32)) and np.array_equal(both.motion[2], np.array(want, f32))


def test_the_shipped_scene():
    hs = abi.HostScene(CFG, 24, 32)
    assert hs.shutter_travel is None  # (a static camera)
    moving = {int(i): tuple(float(v) for v in hs.motion[i]) for i in np.nonzero(hs.motion.any(axis=1))[0]}
    assert moving == {2: (float(f32(1.2)), 0.0, 0.0), 4: (0.0, 0.0, 3.0), 5: (-1.5, float(f32(0.4)), 0.0)}
    across = [i for i, t in moving.items() if t[0] != 0.0 and t[2] == 0.0]
    towards = [i for i, t in moving.items() if t[2] > 0.0 and t[0] == 0.0]  # (the camera looks down -z)
    assert len(across) == 2 and len(towards) == 1
    shutter = abi.HostScene(ROOT / "scenes" / "shutter" / "shutter_spheres.yaml", 24, 32)
    assert shutter.motion is None and shutter.struct.n_spheres == hs.struct.n_spheres
    for i in range(hs.struct.n_spheres):  # the shutter scene's row of spheres
        assert bytes(hs.struct.spheres[i]) == bytes(shutter.struct.spheres[i])


@pytest.mark.parametrize("text", ["[0.1, .nan, 0.0]", "[.inf, 0, 0]", "[0, 0, -.inf]", "[1, 2]", "[1, 2, 3, 4]", "0.5", "[a, b, c]"])
def test_a_bad_travel_is_a_load_error(tmp_path, text):
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(_yaml(tmp_path, "bad", second=text), 24, 32)
    assert "shutter_travel" in str(e.value) and "camera_shutter_travel" not in str(e.value)


def test_a_travel_that_leaves_float32_is_a_load_error(tmp_path):
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(_yaml(tmp_path, "far", first="[3.0e38, 0, 0]", cx="3.0e38"), 24, 32)
    assert "center + shutter_travel of sphere 1 is not finite" in str(e.value)
    ok = abi.HostScene(_yaml(tmp_path, "near", first="[-3.0e38, 0, 0]", cx="3.0e38"), 24, 32)
    assert ok.motion[1, 0] == f32(-3.0e38)


def test_checkpoint_fingerprint():
    h = 0x1234ABCD5678
    assert abi.motion_fingerprint(None, h) == h  # a render without a motion keeps its fingerprint
    tv = np.array([(0.0, 0.0, 0.0), (0.002, 0.0, 0.0)], f32)
    a = abi.motion_fingerprint(tv, h)
    assert a != h and a == abi.motion_fingerprint(tv.copy(), h)
    assert abi.motion_fingerprint(tv[::-1], h) != a          # (which sphere moves)
    assert abi.motion_fingerprint(tv, h + 1) != a
    nxt = tv.copy()
    nxt[1, 0] = np.nextafter(f32(0.002), f32(1.0))
    assert abi.motion_fingerprint(nxt, h) != a
    zero = abi.motion_fingerprint(np.zeros((2, 3), f32), h)
    assert zero != h and zero != a  # (an all-zero motion draws: its sums are not the motionless render's)
    assert abi.motion_fingerprint(np.zeros((3, 3), f32), h) != zero
    # a zero motion and a zero-travel shutter give the same image, and still never share a checkpoint
    assert zero != abi.shutter_fingerprint((0.0, 0.0, 0.0), h)


def test_no_motion_is_a_flag_that_takes_no_value():
    """(The --help text is a recorded yardstick, tests/golden/cli_refusals.json, and stays as it is: the flag is described in the
    README, INTEGRATION.md, DESIGN.md section 25 and the shipped scene's header.)"""
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md", "scenes/motion/moving_spheres.yaml"):
        assert "--no-motion" in (ROOT / doc).read_text(), doc
    r = subprocess.run([str(EXE), "-c", str(CFG), "-t", "unused.png", "--no-motion=1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--no-motion" in r.stderr, (r.returncode, r.stderr[-500:])
