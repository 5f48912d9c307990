"""Environment lighting, what the host side decides without a GPU: the PFM reader, the conversion of a latitude/longitude
image into the octahedral node grid (against np_env's float64 restatement), the fold's boundary identities, the YAML
blueprint and the CLI's options, the checkpoint fingerprint, the C ABI's struct and the argument checks of
rbrt_hip_scene_set_environment that come before the device."""
from __future__ import annotations

import ctypes as C
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_env
from rbrt_amd import abi, standin

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def image(h, w, seed):
    return np.random.default_rng(seed).uniform(0.0, 8.0, (h, w, 3)).astype(f32)


# ---- PFM -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(1, 1), (2, 3), (16, 32)])
@pytest.mark.parametrize("little", [True, False])
def test_pfm_both_byte_orders_and_the_row_flip(tmp_path, h, w, little):
    img = image(h, w, 7 * h + w)
    np_env.write_pfm(tmp_path / "a.pfm", img, little=little)
    got = abi.read_pfm(tmp_path / "a.pfm")
    assert got.shape == (h, w, 3) and np.array_equal(bits(got), bits(img))
    # the file's first row of texels is the image's BOTTOM row
    raw = (tmp_path / "a.pfm").read_bytes()
    first = np.frombuffer(raw[-h * w * 12:][:w * 12], "<f4" if little else ">f4").reshape(w, 3)
    assert np.array_equal(first.astype(f32), img[-1])


def test_the_generated_sky_reads_back(tmp_path):
    sky = standin.make_sky(256, seed=3)
    standin.write_pfm(tmp_path / "sky.pfm", sky)
    assert np.array_equal(bits(abi.read_pfm(tmp_path / "sky.pfm")), bits(sky))
    assert sky.shape == (128, 256, 3) and np.isfinite(sky).all() and (sky >= 0).all()
    assert np.array_equal(sky, standin.make_sky(256, seed=3)) and not np.array_equal(sky, standin.make_sky(256, seed=4))
    up, down = sky[:32].mean(), sky[-32:].mean()
    assert sky.max() > 20.0 and down < 0.1 < up  # a sun, a dark ground


def _pfm_bytes(header: bytes, texels: np.ndarray) -> bytes:
    return header + np.ascontiguousarray(texels, "<f4").tobytes()


@pytest.mark.parametrize("what,data,word", [
    ("grey", _pfm_bytes(b"Pf\n2 2\n-1.0\n", np.zeros(4)), "grey"),
    ("not a pfm", b"P6\n2 2\n255\n" + bytes(12), "PF"),
    ("truncated", _pfm_bytes(b"PF\n2 2\n-1.0\n", np.zeros(11)), "truncated"),
    ("header only", b"PF\n2 2\n", "header"),
    ("trailing bytes", _pfm_bytes(b"PF\n2 2\n-1.0\n", np.zeros(13)), "after the pixels"),
    ("zero scale", _pfm_bytes(b"PF\n2 2\n0.0\n", np.zeros(12)), "scale"),
    ("scale not a number", _pfm_bytes(b"PF\n2 2\nabc\n", np.zeros(12)), "scale"),
    ("nan scale", _pfm_bytes(b"PF\n2 2\nnan\n", np.zeros(12)), "scale"),
    ("negative size", _pfm_bytes(b"PF\n-2 2\n-1.0\n", np.zeros(12)), "size"),
    ("zero size", _pfm_bytes(b"PF\n0 2\n-1.0\n", np.zeros(12)), "size"),
    ("size not a number", _pfm_bytes(b"PF\ntwo 2\n-1.0\n", np.zeros(12)), "size"),
    ("nan texel", _pfm_bytes(b"PF\n2 2\n-1.0\n", np.array([0, 0, 0, 0, math.nan, 0, 0, 0, 0, 0, 0, 0.0])), "texel"),
    ("inf texel", _pfm_bytes(b"PF\n2 2\n-1.0\n", np.array([0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, math.inf])), "texel"),
    ("negative texel", _pfm_bytes(b"PF\n2 2\n-1.0\n", np.array([0, -1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0])), "texel"),
])
def test_pfm_refusals(tmp_path, what, data, word):
    (tmp_path / "bad.pfm").write_bytes(data)
    with pytest.raises(RuntimeError) as e:
        abi.read_pfm(tmp_path / "bad.pfm")
    assert word in str(e.value), (what, str(e.value))


def test_pfm_missing_file(tmp_path):
    with pytest.raises(RuntimeError) as e:
        abi.read_pfm(tmp_path / "nothing.pfm")
    assert "cannot open" in str(e.value)


# ---- conversion ------------------------------------------------------------------------------------------------------------
def ulps(a, b):
    """Distance in float32 steps (both arrays non-negative and finite)."""
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.mark.parametrize("n", [1, 2, 5, 16])
@pytest.mark.parametrize("rotation", [0.0, 90.0, 33.3])
@pytest.mark.parametrize("intensity", [1.0, 0.5])
def test_conversion_against_the_float64_restatement(n, rotation, intensity):
    img = image(16, 32, 11)
    got = abi.environment_nodes(img, n, rotation, intensity)
    exp = np_env.nodes_from_latlong(img, n, rotation, intensity)
    assert got.shape == exp.shape == (n + 1, n + 1, 3)
    # both sides compute in double and round once: a libm difference in atan2 / acos can move a value over one rounding boundary
    assert ulps(got, exp).max() <= 1, ulps(got, exp).max()
    assert (got >= 0).all() and got.max() <= 8.0 * intensity


@pytest.mark.parametrize("n", [1, 2, 3, 5, 16, 33])
def test_boundary_nodes_of_one_direction_are_bit_equal(n):
    e = abi.environment_nodes(image(16, 32, 5), n, 33.3, 1.0)
    b = bits(e)
    for k in range(n + 1):
        assert np.array_equal(b[0, k], b[0, n - k]) and np.array_equal(b[n, k], b[n, n - k]), k
        assert np.array_equal(b[k, 0], b[n - k, 0]) and np.array_equal(b[k, n], b[n - k, n]), k
    if n > 1:  # (N = 1 has four corners and all of them are -y)
        assert np.unique(b.reshape(-1, 3), axis=0).shape[0] > n  # (not a constant map)


def test_a_constant_image_gives_a_constant_map():
    e = abi.environment_nodes(np.full((4, 8, 3), 2.5, f32), 7, 12.0, 1.0)
    assert np.array_equal(bits(e), bits(np.full((8, 8, 3), 2.5, f32)))


@pytest.mark.parametrize("row,col,expect", [
    (0, 16, (0.0, 1.0, 0.0)),     # the top row is +y
    (15, 16, (0.0, -1.0, 0.0)),   # the bottom row is -y
    (8, 16, (0.0, 0.0, -1.0)),    # the middle column looks along -z
    (8, 24, (1.0, 0.0, 0.0)),     # a quarter turn to the right of it: +x
    (8, 8, (-1.0, 0.0, 0.0)),
    (8, 0, (0.0, 0.0, 1.0)),      # the seam: +z
])
def test_one_white_texel_lands_where_the_convention_says(row, col, expect):
    img = np.zeros((16, 32, 3), f32)
    img[row, col] = 1.0
    n = 32
    e = abi.environment_nodes(img, n, 0.0, 1.0)
    j, i = np.unravel_index(np.argmax(e[..., 0]), e.shape[:2])
    d = np_env.node_directions(n)[j, i]
    assert e[j, i, 0] > 0.2 and np.dot(d, expect) > 0.97, (j, i, d)
    # a rotation of +90 degrees about +y: the texel in the middle column lights the direction the +x texel lit
    if (row, col) == (8, 16):
        r = abi.environment_nodes(img, n, 90.0, 1.0)
        j, i = np.unravel_index(np.argmax(r[..., 0]), r.shape[:2])
        assert np.dot(np_env.node_directions(n)[j, i], (1.0, 0.0, 0.0)) > 0.97


def test_the_lookup_reads_a_converted_map_back_at_its_nodes():
    """np_env.lookup (the device's rule) at a node's own direction returns the node, up to the direction's float32 rounding:
    the two halves of the convention -- host unfolding, device folding -- are inverse to each other."""
    n = 8
    e = np_env.smooth_map(n, 3)
    d = np_env.node_directions(n).astype(f32).reshape(-1, 3)
    got = np_env.lookup(e, d).reshape(e.shape)
    assert np.allclose(got, e, rtol=0, atol=1e-3)


# ---- YAML and CLI ------------------------------------------------------------------------------------------------------------
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
  material_type: "lambertian"
  albedo: {x: 0.5, y: 0.5, z: 0.5}
"""


def _scene(tmp_path, env_block, h=16, w=32, seed=2):
    img = image(h, w, seed)
    np_env.write_pfm(tmp_path / "map.pfm", img)
    (tmp_path / "s.yaml").write_text(YAML + env_block.replace("MAP", str(tmp_path / "map.pfm")))
    return img


def test_yaml_defaults_and_overrides(tmp_path):
    img = _scene(tmp_path, "")
    assert abi.HostScene(tmp_path / "s.yaml", 10, 10).environment() is None
    _scene(tmp_path, 'environment_blueprint:\n  file: "MAP"\n  resolution: 6\n')
    e = abi.HostScene(tmp_path / "s.yaml", 10, 10).environment()
    assert np.array_equal(bits(e), bits(abi.environment_nodes(img, 6, 0.0, 1.0)))
    _scene(tmp_path, 'environment_blueprint:\n  file: "MAP"\n  rotation_deg: 33.3\n  intensity: 0.5\n  resolution: 9\n')
    e = abi.HostScene(tmp_path / "s.yaml", 10, 10).environment()
    assert np.array_equal(bits(e), bits(abi.environment_nodes(img, 9, float(f32(33.3)), 0.5)))  # (the YAML's numbers are float32)
    _scene(tmp_path, 'environment_blueprint:\n  file: "MAP"\n')  # the default resolution
    assert abi.HostScene(tmp_path / "s.yaml", 10, 10).environment().shape == (1025, 1025, 3)


@pytest.mark.parametrize("block,word", [
    ('environment_blueprint:\n  rotation_deg: 1\n', "file"),
    ('environment_blueprint:\n  file: "MAP"\n  intensity: -1\n', "intensity"),
    ('environment_blueprint:\n  file: "MAP"\n  intensity: .nan\n', "intensity"),
    ('environment_blueprint:\n  file: "MAP"\n  intensity: .inf\n', "intensity"),
    ('environment_blueprint:\n  file: "MAP"\n  rotation_deg: .inf\n', "rotation_deg"),
    ('environment_blueprint:\n  file: "MAP"\n  resolution: 0\n', "resolution"),
    ('environment_blueprint:\n  file: "MAP"\n  resolution: 4097\n', "resolution"),
    ('environment_blueprint:\n  file: "MAP"\n  resolution: 2.5\n', "resolution"),
    ('environment_blueprint:\n  file: "MAP.missing"\n', "cannot open"),
])
def test_yaml_refusals(tmp_path, block, word):
    _scene(tmp_path, block)
    with pytest.raises(RuntimeError) as e:
        abi.HostScene(tmp_path / "s.yaml", 10, 10)
    assert word in str(e.value)


def test_the_shipped_scene_names_an_environment():
    text = (ROOT / "scenes" / "environment" / "environment_spheres.yaml").read_text()
    assert "environment_blueprint:" in text and ".pfm" in text
    assert "--environment <file|none>" in subprocess.run([str(EXE), "--help"], capture_output=True, text=True).stdout


def _cli(*argv):
    return subprocess.run([str(EXE), *argv], capture_output=True, text=True, timeout=60)


def test_cli_refusals_before_any_render(tmp_path):
    _scene(tmp_path, 'environment_blueprint:\n  file: "MAP"\n  resolution: 4\n')
    cfg, out = str(tmp_path / "s.yaml"), str(tmp_path / "x.png")
    for argv, word in (
        (["--environment", str(tmp_path / "map.pfm"), "--background", "0,0,0"], "--background"),
        (["--environment-intensity", "-1"], "--environment-intensity"),
        (["--environment-intensity", "nan"], "--environment-intensity"),
        (["--environment-intensity", "inf"], "--environment-intensity"),
        (["--environment-rotation", "inf"], "--environment-rotation"),
        (["--environment-rotation", "x"], "--environment-rotation"),
        (["--environment-resolution", "0"], "--environment-resolution"),
        (["--environment-resolution", "4097"], "--environment-resolution"),
        (["--environment", ""], "--environment"),
    ):
        r = _cli("-c", cfg, "-t", out, *argv)
        assert r.returncode == 2 and word in r.stderr, (argv, r.returncode, r.stderr)
    # the scene file's environment and --background: an error that names both, and the way out
    r = _cli("-c", cfg, "-t", out, "--background", "0,0,0")
    assert r.returncode == 101 and "--background" in r.stderr and "environment" in r.stderr, r.stderr
    # a missing file, from the command line and with the scene file's switched on again
    r = _cli("-c", cfg, "-t", out, "--environment", str(tmp_path / "nothing.pfm"))
    assert r.returncode == 101 and "cannot open" in r.stderr, r.stderr
    # the map's options without a map
    (tmp_path / "plain.yaml").write_text(YAML)
    r = _cli("-c", str(tmp_path / "plain.yaml"), "-t", out, "--environment-rotation", "10")
    assert r.returncode == 101 and "need an environment" in r.stderr, r.stderr
    r = _cli("-c", cfg, "-t", out, "--environment", "none", "--environment-rotation", "10")
    assert r.returncode == 101 and "need an environment" in r.stderr, r.stderr
    assert not Path(out).exists()


# ---- checkpoints -----------------------------------------------------------------------------------------------------------
def test_checkpoint_fingerprint():
    h = 0x0123456789ABCDEF
    assert abi.environment_fingerprint(None, h) == h  # a render without one keeps its fingerprint
    a, b = np_env.noise_map(3, 1), np_env.noise_map(3, 1)
    fa = abi.environment_fingerprint(a, h)
    assert fa != h and fa == abi.environment_fingerprint(b, h)
    b[2, 1, 0] = np.nextafter(b[2, 1, 0], f32(9.0))
    assert abi.environment_fingerprint(b, h) != fa
    assert abi.environment_fingerprint(np_env.noise_map(4, 1), h) != fa
    assert abi.environment_fingerprint(a, h + 1) != fa
    # N is covered, not just the bytes: a 1-map of the same 12 floats as part of another shape differs
    flat = np.zeros((2, 2, 3), f32)
    assert abi.environment_fingerprint(flat, h) != abi.environment_fingerprint(np.zeros((3, 3, 3), f32), h)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_environment_layout_matches_the_c_header(tmp_path):
    cname, cls = "rbrt_environment_t", abi.Environment
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));']
    lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "env.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "env"), str(tmp_path / "env.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "env")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 16
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2 and lib.rbrt_hip_supported_flags() == 7  # no new flag bit: the symbol is the capability
    assert "rbrt_hip_scene_set_environment" in abi.HIP_SYMBOLS and "rbrt_hip_debug_environment" in abi.DEBUG_SYMBOLS


def test_a_null_scene_is_refused():
    lib = abi.load_hip()
    nodes = np.zeros((2, 2, 3), f32)
    env = abi.Environment(1, 0, abi.fptr(nodes))
    assert lib.rbrt_hip_scene_set_environment(None, C.byref(env)) == abi.RBRT_ERR_INVALID_ARG
    assert lib.rbrt_hip_scene_set_environment(None, None) == abi.RBRT_ERR_INVALID_ARG
    assert lib.rbrt_hip_debug_environment(None, None, 0, None) == abi.RBRT_ERR_INVALID_ARG
