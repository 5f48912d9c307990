"""The camera shutter at the boundary and in the C++ host, without a GPU: the rbrt_shutter_t layout, the arguments the
library rejects before touching a device, the YAML key, the CLI's refusals and help text, and the checkpoint fingerprint.
(What needs a render -- the flags through --report, the images -- is in test_shutter_gpu.py.)"""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from rbrt_amd import abi
from test_thin_lens_host import CAMERA_YAML

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "shutter" / "shutter_spheres.yaml"
f32 = np.float32


def _yaml(tmp_path, name, **keys):
    p = tmp_path / f"{name}.yaml"
    p.write_text(CAMERA_YAML.format(extra="".join(f"  {k}: {v}\n" for k, v in keys.items())))
    return p


def test_shutter_layout_matches_the_c_header(tmp_path):
    names = [f for f, _ in abi.Shutter._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(rbrt_shutter_t));'
           + "".join(f'printf("{f} %zu\\n", offsetof(rbrt_shutter_t, {f}));' for f in names)
           + 'printf("abi %d\\n", RBRT_ABI_VERSION); return 0;}')
    (tmp_path / "shutter.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "shutter"), str(tmp_path / "shutter.c")], check=True)
    out = subprocess.run([str(tmp_path / "shutter")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    assert int(got["size"]) == C.sizeof(abi.Shutter) == 16
    for f in names:
        assert int(got[f]) == getattr(abi.Shutter, f).offset, f
    assert got["abi"] == "2"


def test_the_symbols_are_the_capability_and_no_flag_bit_was_added():
    import rbrt_amd
    assert "rbrt_hip_scene_set_shutter" in abi.HIP_SYMBOLS and "rbrt_hip_debug_primary_cull_shutter" in abi.DEBUG_SYMBOLS
    assert rbrt_amd.supported_flags() == 7
    assert abi.load_hip().rbrt_hip_abi_version() == 2


def test_invalid_arguments_are_rejected_before_the_device():
    lib = abi.load_hip()
    sh = abi.Shutter()
    assert lib.rbrt_hip_scene_set_shutter(None, C.byref(sh)) == abi.RBRT_ERR_INVALID_ARG
    assert b"null scene" in lib.rbrt_hip_last_error()
    assert lib.rbrt_hip_scene_set_shutter(None, None) == abi.RBRT_ERR_INVALID_ARG
    out = np.zeros(1, np.uint32)
    words = out.ctypes.data_as(C.POINTER(C.c_uint32))
    tv = (C.c_float * 3)(0.0, float("nan"), 0.0)
    assert lib.rbrt_hip_debug_primary_cull_shutter(None, None, None, tv, words, 1) == abi.RBRT_ERR_INVALID_ARG
    assert b"travel" in lib.rbrt_hip_last_error()
    assert lib.rbrt_hip_debug_primary_cull_shutter(None, None, None, None, words, 1) == abi.RBRT_ERR_INVALID_ARG
    ok = (C.c_float * 3)(0.1, 0.0, 0.0)
    assert lib.rbrt_hip_debug_primary_cull_shutter(None, None, None, ok, words, 1) == abi.RBRT_ERR_INVALID_ARG  # (no scene, no camera)


@pytest.mark.parametrize("text,want", [("[0.25, -0.5, 1.0e-3]", (0.25, -0.5, 1.0e-3)), ("[0, 0, 0]", (0.0, 0.0, 0.0)),
                                       ("{x: 1.5, y: 2.5, z: -3.5}", (1.5, 2.5, -3.5))])
def test_the_yaml_key(tmp_path, text, want):
    hs = abi.HostScene(_yaml(tmp_path, "key", camera_shutter_travel=text), 24, 32)
    assert hs.shutter_travel == tuple(float(f32(v)) for v in want)  # (a zero travel is a shutter, too: it draws)
    plain = abi.HostScene(_yaml(tmp_path, "plain"), 24, 32)
    assert plain.shutter_travel is None
    assert bytes(hs.camera) == bytes(plain.camera)  # (the camera is the camera at the opening: the key does not move it)


def test_the_shipped_scene():
    assert abi.HostScene(CFG, 24, 32).shutter_travel == (float(f32(0.6)), 0.0, 0.0)


@pytest.mark.parametrize("text", ["[0.1, .nan, 0.0]", "[.inf, 0, 0]", "[0, 0, -.inf]", "[1, 2]", "[1, 2, 3, 4]", "0.5", "[a, b, c]"])
def test_a_bad_travel_is_a_load_error(tmp_path, text):
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(_yaml(tmp_path, "bad", camera_shutter_travel=text), 24, 32)
    assert "camera_shutter_travel" in str(e.value)


def _run(*args):
    return subprocess.run([str(EXE), "-c", str(CFG), "-t", "unused.png", *args], capture_output=True, text=True)


@pytest.mark.parametrize("args,words", [
    (("--shutter", "0.5"), "'--shutter' needs '--camera-step'"),
    (("--frames", "2", "-s", "2", "--shutter", "0.5"), "'--shutter' needs '--camera-step'"),
    (("--frames", "2", "-s", "2", "--camera-step", "1,0,0", "--shutter", "0.5", "--shutter-travel", "1,0,0"), "cannot be combined with '--shutter-travel'"),
    (("--frames", "2", "-s", "2", "--camera-step", "1,0,0", "--shutter", "-0.5"), "invalid value '-0.5' for '--shutter'"),
    (("--frames", "2", "-s", "2", "--camera-step", "1,0,0", "--shutter", "nan"), "invalid value 'nan' for '--shutter'"),
    (("--frames", "2", "-s", "2", "--camera-step", "1,0,0", "--shutter", "inf"), "invalid value 'inf' for '--shutter'"),
    (("--frames", "2", "-s", "2", "--camera-step", "1e30,0,0", "--shutter", "1e30"), "is not finite"),
    (("--shutter-travel", "1,nan,0"), "invalid value '1,nan,0' for '--shutter-travel'"),
    (("--shutter-travel", "1,inf,0"), "invalid value '1,inf,0' for '--shutter-travel'"),
    (("--shutter-travel", "1,2"), "invalid value '1,2' for '--shutter-travel'"),
])
def test_the_cli_refuses_by_name_before_anything_is_loaded(args, words):
    r = _run(*args)
    assert r.returncode == 2 and words in r.stderr, (r.returncode, r.stderr[-500:])


def test_help():
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for text in ("--shutter-travel <dx,dy,dz>", "--shutter <s>", "camera_shutter_travel", "s times --camera-step", "opening cameras"):
        assert text in r.stdout, text


def test_shutter_product_is_float32():
    """--shutter S gives travel_c = S * camera_step_c in float32: what --shutter-travel takes when handed that product."""
    for s, step in ((0.5, (0.25, 0.0, -0.125)), (0.3, (0.1, 0.7, -1e-3)), (1.0 / 3.0, (3.0, 1e-6, 2.5))):
        travel = [f32(s) * f32(v) for v in step]
        assert all(t.dtype == f32 for t in travel)
        assert abi.shutter_fingerprint(travel, 5) == abi.shutter_fingerprint([float(t) for t in travel], 5)
        wide = [float(f32(s)) * float(f32(v)) for v in step]  # (the double product, rounded when it is stored)
        assert [float(f32(v)) for v in wide] == [float(t) for t in travel]  # (one rounding either way: 24 x 24 bits fit a double)


def test_checkpoint_fingerprint():
    h = 0x1234ABCD5678
    assert abi.shutter_fingerprint(None, h) == h  # a render without a shutter keeps its fingerprint
    a = abi.shutter_fingerprint((0.002, 0.0, 0.0), h)
    assert a != h and a == abi.shutter_fingerprint((0.002, 0.0, 0.0), h)
    assert abi.shutter_fingerprint((0.0, 0.002, 0.0), h) != a
    assert abi.shutter_fingerprint((0.002, 0.0, 0.0), h + 1) != a
    assert abi.shutter_fingerprint((float(np.nextafter(f32(0.002), f32(1.0))), 0.0, 0.0), h) != a
    assert abi.shutter_fingerprint((0.0, 0.0, 0.0), h) != h  # (a zero travel draws: its sums are not the shutterless render's)
