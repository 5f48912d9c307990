"""The thin lens (RBRT_FLAG_THIN_LENS) at the boundary and in the C++ host, without a GPU: the rbrt_camera_lens_t layout,
the flags the library honours, lens arguments it rejects before touching a device, the host's derivation of the lens
from the YAML keys (bit for bit against np_lens.lens_from_yaml) and the load errors of a bad lens."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_lens
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32

CAMERA_YAML = """---
camera_blueprint:
  camera_up:
    x: 0.0
    y: 1.0
    z: -0.4
  camera_look_at:
    x: 0.3
    y: -0.1
    z: -1.0
  camera_position:
    x: 0.5
    y: 5.0
    z: 4.0
  camera_focal_length_mm: 35.0
{extra}mesh_blueprints: []
sphere_blueprints:
  - radius: 1.0
    center:
      x: 0.0
      y: 1.0
      z: -8.0
    material_type: "lambertian"
    albedo:
      x: 0.5
      y: 0.5
      z: 0.5
"""


def _yaml(tmp_path, name, **keys):
    extra = "".join(f"  {k}: {v}\n" for k, v in keys.items())
    p = tmp_path / f"{name}.yaml"
    p.write_text(CAMERA_YAML.format(extra=extra))
    return p


def test_camera_lens_layout_matches_the_c_header(tmp_path):
    names = [f for f, _ in abi.CameraLens._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(rbrt_camera_lens_t));'
           + "".join(f'printf("{f} %zu\\n", offsetof(rbrt_camera_lens_t, {f}));' for f in names)
           + 'printf("flag %u\\n", RBRT_FLAG_THIN_LENS); return 0;}')
    (tmp_path / "lens.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "lens"), str(tmp_path / "lens.c")], check=True)
    out = subprocess.run([str(tmp_path / "lens")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    assert int(got["size"]) == C.sizeof(abi.CameraLens)
    for f in names:
        assert int(got[f]) == getattr(abi.CameraLens, f).offset, f
    assert got["cam"] == "0"  # &lens.cam is the pointer every render entry point receives
    assert int(got["flag"]) == abi.FLAG_THIN_LENS == 4


def test_supported_flags():
    import rbrt_amd
    assert rbrt_amd.supported_flags() == 7
    assert abi.load_hip().rbrt_hip_supported_flags() == (abi.FLAG_COLLECT_STATS | abi.FLAG_CONSTANT_BACKGROUND | abi.FLAG_THIN_LENS)


@pytest.mark.parametrize("field,value", [("lens_u", (float("nan"), 0.0, 0.0)), ("lens_v", (0.0, float("inf"), 0.0)),
                                         ("focus_scale", 0.0), ("focus_scale", -2.0), ("focus_scale", float("nan")),
                                         ("focus_scale", float("inf")), ("reserved", 1)])
def test_invalid_lens_arguments_are_rejected_before_the_device(field, value):
    lib = abi.load_hip()
    cam = abi.Camera()
    cam.position, cam.right, cam.up, cam.img_center_point = abi._f3((0, 0, 0)), abi._f3((1, 0, 0)), abi._f3((0, 1, 0)), abi._f3((0, 0, -1))
    cam.mm_per_pix_hor = cam.mm_per_pix_vert = 0.5
    cam.img_width_pix, cam.img_height_pix = 8, 8
    sc = abi.SceneData(spheres=[((0.0, 0.0, -5.0), 1.0, abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5)))])
    lens = abi.camera_lens(cam, (0.001, 0.0, 0.0), (0.0, 0.001, 0.0), 10.0)
    setattr(lens, field, abi._f3(value) if isinstance(value, tuple) else value)
    opts = abi.default_opts(spp=1, flags=abi.FLAG_THIN_LENS)
    rad = np.zeros((8, 8, 3), f32)
    rc = lib.rbrt_hip_render(C.byref(lens.cam), sc.ptr(), C.byref(opts), rad.ctypes.data_as(abi.f32p), None)
    assert rc == abi.RBRT_ERR_INVALID_ARG, rc
    assert b"lens" in lib.rbrt_hip_last_error()
    # without the flag nothing past the camera is read: the same words are no error (a render, or no device here)
    opts.flags = 0
    rc = lib.rbrt_hip_render(C.byref(lens.cam), sc.ptr(), C.byref(opts), rad.ctypes.data_as(abi.f32p), None)
    assert rc in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE), lib.rbrt_hip_last_error()


def test_the_debug_hook_rejects_a_null_lens():
    out = np.zeros(1, np.uint32)
    assert abi.load_hip().rbrt_hip_debug_primary_cull_lens(None, None, out.ctypes.data_as(C.POINTER(C.c_uint32)), 1) == abi.RBRT_ERR_INVALID_ARG


def test_the_debug_hook_with_options_rejects_null_arguments():
    """rbrt_hip_debug_primary_cull_opts: the table of a render with given options; no scene, camera or options is an error."""
    out = np.zeros(1, np.uint32)
    words = out.ctypes.data_as(C.POINTER(C.c_uint32))
    opts = abi.default_opts(min_dist=1e-6)
    assert abi.load_hip().rbrt_hip_debug_primary_cull_opts(None, None, C.byref(opts), words, 1) == abi.RBRT_ERR_INVALID_ARG
    assert abi.load_hip().rbrt_hip_debug_primary_cull_opts(None, None, None, words, 1) == abi.RBRT_ERR_INVALID_ARG
    assert b"null argument" in abi.load_hip().rbrt_hip_last_error()


@pytest.mark.parametrize("aperture,focus", [(7.0, 15.0), (0.5, 2.25), (50.0, 3.0), (1e-3, 1000.0), (28.0 / 1.4, 6.5)])
def test_the_host_derives_the_lens_bit_for_bit(tmp_path, aperture, focus):
    hs = abi.HostScene(_yaml(tmp_path, "lens", camera_aperture_mm=aperture, camera_focus_distance=focus), 24, 32)
    assert hs.lens is not None
    u, v, fs = np_lens.lens_from_yaml(list(hs.camera.right), (0.3, -0.1, -1.0), 35.0, aperture, focus)
    assert np.array_equal(np.array(list(hs.lens.lens_u), f32).view(np.uint32), u.view(np.uint32))
    assert np.array_equal(np.array(list(hs.lens.lens_v), f32).view(np.uint32), v.view(np.uint32))
    assert f32(hs.lens.focus_scale).view(np.uint32) == fs.view(np.uint32)
    assert hs.lens.reserved == 0
    # the camera inside is the pinhole camera of the same YAML
    pin = abi.HostScene(_yaml(tmp_path, "pin"), 24, 32)
    assert bytes(hs.lens.cam) == bytes(pin.camera) == bytes(hs.camera)
    # the lens is orthogonal to the view direction and round: |u| = |v| = aperture / 2000, u . v = 0 (to float precision)
    r = aperture / 2000.0
    assert np.isclose(np.linalg.norm(u.astype(np.float64)), r, rtol=1e-5) and np.isclose(np.linalg.norm(v.astype(np.float64)), r, rtol=1e-5)
    assert abs(float(np.dot(u.astype(np.float64), v.astype(np.float64)))) < 1e-5 * r * r


def test_no_aperture_or_a_zero_aperture_is_the_pinhole(tmp_path):
    assert abi.HostScene(_yaml(tmp_path, "none"), 24, 32).lens is None
    assert abi.HostScene(_yaml(tmp_path, "zero", camera_aperture_mm=0.0), 24, 32).lens is None
    assert abi.HostScene(_yaml(tmp_path, "zero_f", camera_aperture_mm=0.0, camera_focus_distance=4.0), 24, 32).lens is None


@pytest.mark.parametrize("keys,words", [
    (dict(camera_aperture_mm=5.0), "camera_focus_distance"),
    (dict(camera_aperture_mm=-1.0, camera_focus_distance=3.0), "camera_aperture_mm"),
    (dict(camera_aperture_mm=".nan", camera_focus_distance=3.0), "camera_aperture_mm"),
    (dict(camera_aperture_mm=".inf", camera_focus_distance=3.0), "camera_aperture_mm"),
    (dict(camera_aperture_mm=5.0, camera_focus_distance=-3.0), "camera_focus_distance"),
    (dict(camera_aperture_mm=5.0, camera_focus_distance=0.0), "camera_focus_distance"),
    (dict(camera_aperture_mm=5.0, camera_focus_distance=".nan"), "camera_focus_distance"),
])
def test_a_bad_lens_is_a_load_error(tmp_path, keys, words):
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(_yaml(tmp_path, "bad", **keys), 24, 32)
    assert words in str(e.value)
