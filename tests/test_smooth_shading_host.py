"""Smooth shading at the boundary and in the C++ host, without a GPU: the .obj loader's `vn` lines and face forms, the
corner normals it derives (the file's, rotated; or area-weighted vertex normals, bit for bit against np_smooth), the
unchanged triangles and SoA arrays of every file, the YAML key, the CLI flag and the shading arguments the library rejects
before it touches a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_smooth
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
NF = abi.NORMAL_FIELDS
_libm = C.CDLL("libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = C.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [C.c_float]

YAML = """---
camera_blueprint:
  camera_up: {{x: 0.0, y: 1.0, z: -0.4}}
  camera_look_at: {{x: 0.0, y: -0.1, z: -1.0}}
  camera_position: {{x: 0.0, y: 5.0, z: 4.0}}
  camera_focal_length_mm: 28.0
mesh_blueprints:
  - obj_filepath: {obj}
    scale: {scale}
    translation: {{x: 0.5, y: -1.0, z: -9.0}}
    rotation_rad: {{x: {rx}, y: {ry}, z: {rz}}}
    material_type: "metal"
    material_param: 0.1
    albedo: {{x: 0.8, y: 0.8, z: 0.8}}
{shading}sphere_blueprints: []
"""


def _yaml(tmp_path, name, obj, shading=None, scale=1.5, rot=(0.3, -0.7, 1.1)):
    sh = "" if shading is None else f"    shading: {shading}\n"
    p = tmp_path / f"{name}.yaml"
    p.write_text(YAML.format(obj=obj, scale=scale, rx=rot[0], ry=rot[1], rz=rot[2], shading=sh))
    return p


def _obj(tmp_path, name, text):
    p = tmp_path / f"{name}.obj"
    p.write_text(text)
    return p


def rotate_point(v, rot):
    """Vec3::rotate_point (vec3.rs:139-155) in float32 with the host's sinf / cosf, in the C++ expression's order."""
    sx, sy, sz = (f32(_libm.sinf(float(a))) for a in rot)
    cx, cy, cz = (f32(_libm.cosf(float(a))) for a in rot)
    x, y, z = (f32(c) for c in v)
    return np.array([
        f32(f32(f32(f32(cx * cz) - f32(f32(cy * sx) * sz)) * x) - f32(f32(f32(cx * sz) + f32(f32(cy * cz) * sx)) * y)) + f32(f32(sx * sy) * z),
        f32(f32(f32(f32(cz * sx) + f32(f32(cx * cy) * sz)) * x) + f32(f32(f32(f32(cx * cy) * cz) - f32(sx * sz)) * y)) - f32(f32(cx * sy) * z),
        f32(f32(f32(sy * sz) * x) + f32(f32(cz * sy) * y)) + f32(cy * z)], f32)


def transform(p, scale, rot, trans):
    """mesh.rs:102-112 as the host does it: scale, rotate_point, translate."""
    return rotate_point([f32(f32(c) * f32(scale)) for c in p], rot) + np.asarray(trans, f32)


def corners(arrs):
    """(n_total, 3, 3) corner normals out of HostScene.mesh_arrays."""
    return np.stack([np.stack([arrs[f"n{k}{c}"] for c in "xyz"], -1) for k in range(3)], 1)


# An octahedron with one normal per vertex (unnormalised), faces in every token form the loader accepts.
V = [(0, 0, 1), (1, 0, 0), (0, 1, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)]
VN = [(0.1, 0.2, 2.0), (1.5, 0.1, 0.0), (0.0, 0.7, 0.1), (-3.0, 0.0, 0.2), (0.0, -1.0, 0.0), (0.2, 0.1, -1.0)]
FACES = [(1, 2, 3), (1, 3, 4), (1, 4, 5), (1, 5, 2), (6, 3, 2), (6, 4, 3), (6, 5, 4), (6, 2, 5)]


def octahedron(form, negative=False):
    lines = [f"v {x} {y} {z}" for x, y, z in V] + [f"vn {x} {y} {z}" for x, y, z in VN] + ["vt 0.5 0.5"]
    for f in FACES:
        toks = []
        for i in f:
            j = i - 7 if negative else i  # (-6 .. -1: relative to the end of what was read so far)
            toks.append({"v//vn": f"{j}//{j}", "v/vt/vn": f"{j}/1/{j}" if not negative else f"{j}/-1/{j}"}[form])
        lines.append("f " + " ".join(toks))
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("form", ["v//vn", "v/vt/vn"])
@pytest.mark.parametrize("negative", [False, True])
@pytest.mark.parametrize("scale", [1.5, -2.0])
def test_file_normals_of_every_face_form_are_rotated(tmp_path, form, negative, scale):
    rot = (0.3, -0.7, 1.1)
    obj = _obj(tmp_path, "oct", octahedron(form, negative))
    hs = abi.HostScene(_yaml(tmp_path, "s", obj, "smooth", scale=scale, rot=rot), 24, 32)
    got = corners(hs.mesh_arrays(0))
    assert got.shape == (8, 3, 3)  # (8 triangles: no padding)
    sign = f32(1.0 if scale > 0 else -1.0)
    for t, f in enumerate(FACES):
        for k, i in enumerate(f):
            exp = rotate_point(sign * np.array(VN[i - 1], f32), rot)
            assert np.array_equal(got[t, k].view(np.uint32), exp.view(np.uint32)), (t, k, got[t, k], exp)
    # the positions are those of the same file without normals
    plain = _obj(tmp_path, "plain", "\n".join([f"v {x} {y} {z}" for x, y, z in V] + ["f %d %d %d" % f for f in FACES]) + "\n")
    hp = abi.HostScene(_yaml(tmp_path, "p", plain, scale=scale, rot=rot), 24, 32)
    a, b = hs.mesh_arrays(0), hp.mesh_arrays(0)
    for k in abi.MeshData.FIELDS + ("is_padding",):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert not any(k in b for k in NF)  # (a flat mesh has no corner normals)


def grid_obj(n=5, seed=3, with_vn=None):
    """A bumpy n x n height field: shared vertices, faces in file order. with_vn: None (no vn), 'partial' (vn on some
    corners only) or 'all'."""
    rng = np.random.default_rng(seed)
    lines = []
    for j in range(n):
        for i in range(n):
            lines.append(f"v {i * 0.5:.6g} {rng.uniform(-0.3, 0.3):.6g} {j * 0.5:.6g}")
    if with_vn:
        lines.append("vn 0 1 0")
    faces = []
    for j in range(n - 1):
        for i in range(n - 1):
            a, b, c, d = j * n + i + 1, j * n + i + 2, (j + 1) * n + i + 2, (j + 1) * n + i + 1
            faces += [(a, c, b), (a, d, c)]
    for q, f in enumerate(faces):
        if with_vn == "all" or (with_vn == "partial" and q % 3 == 0):
            lines.append("f " + " ".join(f"{i}//1" for i in f))
        else:
            lines.append("f " + " ".join(str(i) for i in f))
    pos = np.array([[float(x) for x in l.split()[1:]] for l in lines if l.startswith("v ")], np.float64)
    return "\n".join(lines) + "\n", pos.astype(f32), np.array(faces) - 1


@pytest.mark.parametrize("with_vn", [None, "partial"])
def test_computed_normals_follow_the_stated_summation(tmp_path, with_vn):
    text, pos, faces = grid_obj(with_vn=with_vn)
    rot, scale, trans = (0.3, -0.7, 1.1), 1.5, (0.5, -1.0, -9.0)
    hs = abi.HostScene(_yaml(tmp_path, "g", _obj(tmp_path, "g", text), "smooth", scale=scale, rot=rot), 24, 32)
    got = corners(hs.mesh_arrays(0))
    tv = np.stack([np.stack([transform(pos[i], scale, rot, trans) for i in f]) for f in faces])
    exp = np_smooth.area_weighted(tv, faces)
    n = len(faces)
    assert got.shape[0] == n + n % 8
    assert np.array_equal(got[:n].view(np.uint32), exp.view(np.uint32))
    assert np.array_equal(got[n:].view(np.uint32), np.repeat(exp[:1], n % 8, 0).view(np.uint32))  # padding: entry 0's
    # the vertex normals are shared: a vertex has one normal in every triangle that uses it
    assert np.array_equal(got[0, 0], got[1, 0])
    # and are not the face normals
    a = hs.mesh_arrays(0)
    assert not np.array_equal(got[:n, 0, 0], a["nx"][:n])


def test_file_normals_need_every_corner_of_a_model(tmp_path):
    """Two models (o lines): the first names a vn on every corner (file normals), the second on some (computed)."""
    text, pos, faces = grid_obj(n=3, with_vn="all")
    text2, _, _ = grid_obj(n=3, with_vn="partial")
    second = [l for l in text2.splitlines() if l.startswith("f ")]
    obj = _obj(tmp_path, "two", text + "o second\n" + "\n".join(second) + "\n")
    rot = (0.0, 0.0, 0.5)
    hs = abi.HostScene(_yaml(tmp_path, "two", obj, "smooth", scale=1.0, rot=rot), 24, 32)
    got = corners(hs.mesh_arrays(0))
    n1 = len(faces)
    up = rotate_point(np.array([0.0, 1.0, 0.0], f32), rot)
    assert np.array_equal(got[:n1].reshape(-1, 3), np.tile(up, (3 * n1, 1)))
    tv = np.stack([np.stack([transform(pos[i], 1.0, rot, (0.5, -1.0, -9.0)) for i in f]) for f in faces])
    assert np.array_equal(got[n1:2 * n1].view(np.uint32), np_smooth.area_weighted(tv, faces).view(np.uint32))


def test_zero_sums_and_degenerate_triangles(tmp_path):
    """Two triangles on the same three positions, opposite windings: every sum is zero, each corner gets its own face
    normal. A lone degenerate triangle has no finite face normal either: (0, 0, 0), which the library meets with the
    stored face normal."""
    obj = _obj(tmp_path, "z", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 3 2\no d\nv 2 2 2\nf 4 4 4\n")
    hs = abi.HostScene(_yaml(tmp_path, "z", obj, "smooth", scale=1.0, rot=(0.0, 0.0, 0.0)), 24, 32)
    a = hs.mesh_arrays(0)
    got = corners(a)
    for t in range(2):
        face = np.array([a["nx"][t], a["ny"][t], a["nz"][t]], f32)
        assert np.all(np.isfinite(face))
        for k in range(3):
            assert np.array_equal(got[t, k], face)
    assert np.array_equal(got[2], np.zeros((3, 3), f32))


def test_flat_arrays_and_output_do_not_change(tmp_path):
    """A file with vn lines and v//vn, v/vt/vn faces loads to the same triangles, SoA arrays and stdout lines as the same
    file stripped of them, flat or smooth."""
    text, _, _ = grid_obj(n=6, with_vn="all")
    text = text.replace("vn 0 1 0\n", "vn 0 1 0\nvt 0.25 0.75\n")
    lines = text.splitlines()
    lines = [l if not l.startswith("f ") or i % 2 else l.replace("//1", "/1/1") for i, l in enumerate(lines)]
    rich = _obj(tmp_path, "rich", "\n".join(lines) + "\n")
    plain = _obj(tmp_path, "plain", "\n".join(l.replace("//1", "").replace("/1/1", "") for l in lines
                                              if not l.startswith(("vn", "vt"))) + "\n")
    arrays = []
    outs = []
    for obj, sh in ((plain, None), (rich, None), (rich, "flat"), (rich, "smooth"), (plain, "smooth")):
        y = _yaml(tmp_path, f"{obj.stem}_{sh}", obj, sh)
        a = abi.HostScene(y, 24, 32).mesh_arrays(0)
        arrays.append(a)
        r = subprocess.run([str(EXE), "-c", str(y), "-t", str(tmp_path / "o.png"), "--height", "8", "-w", "8", "-s", "1"],
                           capture_output=True, text=True, timeout=300)
        outs.append([l for l in r.stdout.splitlines() if "loaded" in l or "AVX" in l])
    for a in arrays[1:]:
        for k in abi.MeshData.FIELDS + ("is_padding",):
            assert a[k].tobytes() == arrays[0][k].tobytes(), k
    assert all(o == [l.replace(str(plain), str(rich)) for l in outs[0]] for o in outs[1:4]), outs
    assert outs[4] == outs[0] and outs[0]
    assert not any(k in arrays[1] for k in NF) and all(k in arrays[3] for k in NF)
    assert not np.array_equal(corners(arrays[3]), corners(arrays[4]))  # (file normals vs computed)


def test_bad_face_tokens_still_fail_and_bad_normals_fall_back(tmp_path):
    """A face whose position is bad is an error, as before; a vn index out of range or a bad vn line only costs the model
    its file normals."""
    bad = _obj(tmp_path, "bad", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1//1 2//1 4//1\n")
    with pytest.raises(RuntimeError, match="bad face index"):
        abi.HostScene(_yaml(tmp_path, "bad", bad, "smooth"), 24, 32)
    text = "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0.5\nvn 0 0 1\nvn x y z\nf 1//1 2//1 3//1\nf 2//7 4//1 3//1\nf 1//2 2//1 3//1\n"
    hs = abi.HostScene(_yaml(tmp_path, "fb", _obj(tmp_path, "fb", text), "smooth", scale=1.0, rot=(0.0, 0.0, 0.0)), 24, 32)
    got = corners(hs.mesh_arrays(0))
    pos = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0.5)], f32)
    faces = np.array([(0, 1, 2), (1, 3, 2), (0, 1, 2)])
    tv = np.stack([np.stack([transform(pos[i], 1.0, (0.0, 0.0, 0.0), (0.5, -1.0, -9.0)) for i in f]) for f in faces])
    assert np.array_equal(got[:3].view(np.uint32), np_smooth.area_weighted(tv, faces).view(np.uint32))  # (computed)
    assert not np.array_equal(got[0, 1], np.array([0.0, 0.0, 1.0], f32))


@pytest.mark.parametrize("value", ["phong", "Smooth", "1", "[]"])
def test_bad_shading_values_are_rejected(tmp_path, value):
    obj = _obj(tmp_path, "oct", octahedron("v//vn"))
    with pytest.raises(RuntimeError, match="shading"):
        abi.HostScene(_yaml(tmp_path, "bad", obj, value), 24, 32)


def test_no_key_is_flat_and_the_cli_flag_is_checked(tmp_path):
    obj = _obj(tmp_path, "oct", octahedron("v//vn"))
    assert abi.HostScene(_yaml(tmp_path, "none", obj), 24, 32).shading is None
    assert abi.HostScene(_yaml(tmp_path, "flat", obj, "flat"), 24, 32).shading is None
    assert abi.HostScene(_yaml(tmp_path, "smooth", obj, "smooth"), 24, 32).shading is not None
    r = subprocess.run([str(EXE), "-c", str(_yaml(tmp_path, "none", obj)), "--shading", "gouraud"], capture_output=True, text=True)
    assert r.returncode == 2 and "--shading" in r.stderr
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert "--shading" in r.stdout


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
def _mesh(n=11):
    rng = np.random.default_rng(5)
    tris = rng.uniform(-1, 1, (n, 3, 3)).astype(f32) + np.array([0, 0, -5], f32)
    n_total = n + n % 8
    full = np.concatenate([tris, np.repeat(tris[:1], n_total - n, 0)])
    e1, e2 = full[:, 1] - full[:, 0], full[:, 2] - full[:, 0]
    nr = np.cross(e1, e2)
    nr = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(f32)
    arrs = dict(v0x=full[:, 0, 0], v0y=full[:, 0, 1], v0z=full[:, 0, 2], e1x=e1[:, 0], e1y=e1[:, 1], e1z=e1[:, 2],
                e2x=e2[:, 0], e2y=e2[:, 1], e2z=e2[:, 2], nx=nr[:, 0], ny=nr[:, 1], nz=nr[:, 2])
    pad = np.array([0] * n + [1] * (n_total - n), np.uint8)
    md = abi.MeshData(arrs, pad, n, full.reshape(-1, 3).min(0), full.reshape(-1, 3).max(0), abi.material(abi.MAT_METAL, (0.5, 0.5, 0.5), 0.0))
    return md, nr


def _shading(md, nr, n_meshes=None, reserved=0, null=(), bad=None):
    arrs = {k: np.ascontiguousarray(nr[:, "xyz".index(k[2])]) for k in NF}
    if bad is not None:
        arrs[bad[0]] = arrs[bad[0]].copy()
        arrs[bad[0]][bad[1]] = bad[2]
    mn = abi.MeshNormals()
    for k in NF:
        if k not in null:
            setattr(mn, k, abi.fptr(arrs[k]))
    arr = (abi.MeshNormals * 1)(mn)
    sh = abi.SceneShading(1 if n_meshes is None else n_meshes, reserved, arr)
    return sh, (arrs, arr)


@pytest.mark.parametrize("case", ["n_meshes", "reserved", "one_null", "eight_null", "nan", "inf_in_padding"])
def test_invalid_shading_arguments_are_rejected_before_the_device(case):
    lib = abi.load_hip()
    md, nr = _mesh()
    sc = abi.SceneData(meshes=[md])
    kw = dict(n_meshes=dict(n_meshes=2), reserved=dict(reserved=1), one_null=dict(null=("n1y",)),
              eight_null=dict(null=NF[1:]), nan=dict(bad=("n2x", 3, float("nan"))),
              inf_in_padding=dict(bad=("n0z", md.n_total - 1, float("inf"))))[case]
    sh, _keep = _shading(md, nr, **kw)
    h = C.c_void_p()
    assert lib.rbrt_hip_scene_create_shaded(sc.ptr(), C.byref(sh), 0, C.byref(h)) == abi.RBRT_ERR_INVALID_ARG
    assert b"shading" in lib.rbrt_hip_last_error()
    cam = abi.Camera()
    cam.position, cam.right, cam.up, cam.img_center_point = abi._f3((0, 0, 0)), abi._f3((1, 0, 0)), abi._f3((0, 1, 0)), abi._f3((0, 0, -1))
    cam.mm_per_pix_hor = cam.mm_per_pix_vert = 0.5
    cam.img_width_pix, cam.img_height_pix = 8, 8
    rad = np.zeros((8, 8, 3), f32)
    opts = abi.default_opts(spp=1)
    rc = lib.rbrt_hip_render_shaded(C.byref(cam), sc.ptr(), C.byref(sh), C.byref(opts), rad.ctypes.data_as(abi.f32p), None)
    assert rc == abi.RBRT_ERR_INVALID_ARG


def test_valid_shading_is_no_argument_error():
    """All nine arrays, all NULL, or no shading at all: accepted (a render, or no device here)."""
    lib = abi.load_hip()
    md, nr = _mesh()
    sc = abi.SceneData(meshes=[md])
    h = C.c_void_p()
    for sh in (_shading(md, nr)[0], _shading(md, nr, null=NF)[0], None):
        rc = lib.rbrt_hip_scene_create_shaded(sc.ptr(), None if sh is None else C.byref(sh), 0, C.byref(h))
        assert rc in (abi.RBRT_OK, abi.RBRT_ERR_NO_DEVICE), lib.rbrt_hip_last_error()
        if rc == abi.RBRT_OK:
            lib.rbrt_hip_scene_destroy(h)


def test_mesh_data_normals_make_a_shaded_scene():
    md, nr = _mesh()
    flat = abi.SceneData(meshes=[md])
    assert flat.shading_ptr() is None
    smooth = abi.SceneData(meshes=[md, md.with_normals({k: nr[:, "xyz".index(k[2])] for k in NF})])
    assert smooth.shading is not None and smooth.shading.n_meshes == 2 and smooth.shading.reserved == 0
    assert not smooth.shading.meshes[0].n0x and smooth.shading.meshes[1].n0x
