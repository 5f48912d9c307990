"""Smooth shading of meshes (rbrt_hip.h rbrt_scene_shading_t) on the GPU.

The debug hook's normals and the images are compared bit for bit with the numpy restatement (np_smooth.py), through every
entry point, under both BVH builders, the refined tree and with the tile pass off. A scene without corner normals gives
exactly the image of the flat entry points, with the same LDS per wave. Independent of the restatement: a tessellated
sphere with its exact normals looks like the analytic sphere far more closely than the same mesh shaded flat. The C++
host: the YAML key, --shading, several ranks and checkpoints."""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import np_smooth
import scenes
from rbrt_amd import abi, standin

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
W, H = 32, 24
L_, M_, D_ = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC
MATS = {"lambertian": abi.material(L_, (0.7, 0.4, 0.2)), "metal": abi.material(M_, (0.8, 0.8, 0.75), 0.05),
        "dielectric": abi.material(D_, (0.0, 0.0, 0.0), 1.5)}
N_ZEROED = 40  # entries of the computed-normals mesh whose corner normals are all zero: the fallback to the face normal


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    """Bit for bit, a NaN anywhere in one only where the other has one too."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(bits(np.where(nan, 0, a)), bits(np.where(nan, 0, b)))


def hook_scene(oracle):
    """The example spheres, a flat stand-in, a stand-in with file-style normals (1203 entries: big enough for the device
    builder's first tree) and one with computed normals whose first N_ZEROED entries have all-zero corner normals."""
    flat = scenes.standin_mesh(oracle, 61, 30.0, (-1.5, 0.3, -7.0), (0.0, 0.5, 0.0), abi.material(M_, (0.7, 0.6, 0.5), 0.1))
    filed = np_smooth.standin_smooth(oracle, 1203, 40.0, (4.0, -1.5, -11.0), MATS["metal"], "file")
    comp = np_smooth.standin_smooth(oracle, 603, 30.0, (0.5, -1.0, -13.0), MATS["dielectric"], "computed")
    nrm = {k: v.copy() for k, v in comp.normals.items()}
    for k in nrm:
        nrm[k][:N_ZEROED] = 0.0
        nrm[k][comp.n_real:] = nrm[k][0]  # (padding copies entry 0)
    return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES), meshes=[flat, filed, comp.with_normals(nrm)])


def image_scene(oracle, kind):
    """The example spheres and two small smooth meshes of material `kind`: a tessellated sphere (exact normals) and the
    stand-in (computed normals); a flat stand-in behind them."""
    mat = MATS[kind]
    _, ball = np_smooth.sphere_mesh(oracle, (3.2, 1.2, -8.0), 1.2, 3, mat)
    blob = np_smooth.standin_smooth(oracle, 61, 30.0, (-1.0, -1.3, -6.5), mat, "computed")
    flat = scenes.standin_mesh(oracle, 61, 35.0, (0.0, -1.0, -14.0), (0.0, 0.0, 0.0), abi.material(L_, (0.3, 0.6, 0.3)))
    return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES), meshes=[ball, blob, flat])


def flat_copy(sc):
    return abi.SceneData(spheres=sc.spheres, meshes=[m.with_normals(None) for m in sc.meshes], triangles=sc.triangles,
                         element_order=sc.element_order)


# ---- the debug hook ------------------------------------------------------------------------------------------------------
def hook_rays(sc, rng):
    """Rays at random points of the meshes' entries (corners and edges included), from outside, some grazing; rays at the
    zeroed entries; rays from a camera position at random directions."""
    rays = []
    for mi, md in enumerate(sc.meshes):
        a = md.arrays
        n_real = md.n_real
        for j in range(1000 if mi else 400):
            i = int(rng.integers(0, N_ZEROED)) if (mi == 2 and j % 4 == 0) else int(rng.integers(0, n_real))
            v0 = np.array([a["v0x"][i], a["v0y"][i], a["v0z"][i]], np.float64)
            e1 = np.array([a["e1x"][i], a["e1y"][i], a["e1z"][i]], np.float64)
            e2 = np.array([a["e2x"][i], a["e2y"][i], a["e2z"][i]], np.float64)
            b = rng.dirichlet((1.0, 1.0, 1.0)) if j % 5 else np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0]][j % 4], float)
            p = v0 + b[1] * e1 + b[2] * e2
            nf = np.cross(e1, e2)
            nf /= np.linalg.norm(nf) + 1e-30
            t = rng.normal(size=3)
            t -= np.dot(t, nf) * nf
            t /= np.linalg.norm(t) + 1e-30
            side = 1.0 if rng.random() < 0.8 else -1.0
            dirn = (t + side * 0.02 * nf) if j % 7 == 0 else (side * nf + 0.8 * rng.normal(size=3))  # (grazing every 7th)
            dirn /= np.linalg.norm(dirn)
            o = p + rng.uniform(0.5, 6.0) * dirn
            rays.append(np.concatenate([o, -dirn]))
    cam = np.array([0.0, 5.0, 4.0])
    for _ in range(600):
        d = np.array([rng.uniform(-0.6, 0.6), rng.uniform(-0.7, 0.1), -1.0])
        rays.append(np.concatenate([cam, d / np.linalg.norm(d)]))
    return np.array(rays, f32)


def restated_normals(sc, rays):
    ns = np_smooth.np_scene(sc)
    out = np.full((len(rays), 3), np.nan, f32)
    zeroed = 0
    for k, r in enumerate(rays):
        o, d = r[:3].astype(f32), r[3:].astype(f32)
        hit = np_smooth.scene_hit(ns, o, d, f32(0.001), f32(2000.0))
        if hit is not None:
            out[k] = hit["normal"]
            zeroed += hit["obj"] - np_smooth.n_elements(ns) == 2 and hit["tri"] < N_ZEROED
    return out, zeroed


@pytest.mark.parametrize("builder", [None, "host", "device"])
def test_the_hook_gives_the_restated_normals(hip, oracle, monkeypatch, builder):
    if builder:
        monkeypatch.setenv("RBRT_BVH_BUILDER", builder)
    else:
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    sc = hook_scene(oracle)
    rays = hook_rays(sc, np.random.default_rng(4))
    exp, zeroed = restated_normals(sc, rays)
    with hip.HipScene(sc) as hs:
        got = hs.shading_normals(rays)
        if builder == "device":
            assert hs.info()["n_meshes_device_built"] >= 2
        if builder is None:
            assert hs.refine_wait(120.0)[0] in (0, 1)
            assert same_bits(hs.shading_normals(rays), exp)  # (the refined trees)
    bad = np.argwhere(~np.all((bits(got) == bits(exp)) | (np.isnan(got) & np.isnan(exp)), axis=1))[:, 0]
    assert same_bits(got, exp), (len(bad), bad[:5], got[bad[:3]], exp[bad[:3]])
    hits = ~np.isnan(exp[:, 0])
    print(f"{len(rays)} rays, {int(hits.sum())} hits, {zeroed} on zeroed entries")
    assert hits.sum() > 0.8 * len(rays) and zeroed >= 20
    # the smooth meshes' normals are not their face normals; the flat mesh's are
    with hip.HipScene(flat_copy(sc)) as hf:
        flat = hf.shading_normals(rays)
    assert not same_bits(flat, got)
    _, obj, _, _ = oracle.trace_rays(sc, rays, 0.001, 2000.0)
    on_flat = obj == len(sc.spheres)
    assert on_flat.sum() > 100 and same_bits(flat[on_flat], got[on_flat])


# ---- images ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(MATS))
def test_render_shaded_gives_the_restated_image(hip, oracle, kind):
    cam = scenes.camera(oracle, W, H)
    sc = image_scene(oracle, kind)
    opts = abi.default_opts(spp=3, seed=9)
    got, got8 = hip.render_scene(cam, 3, sc, seed=9)
    exp, exp8 = np_smooth.restated_image(cam, sc, opts)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    flat, _ = hip.render_scene(cam, 3, flat_copy(sc), seed=9)
    assert not np.array_equal(bits(flat), bits(got))


def test_every_entry_point_gives_the_same_image(hip, oracle):
    """render_shaded; create_shaded + render_device; render_pass cut at 0-1-4-5 and at 0-3-5; three ranks' tiles; a stream
    of frames at pipeline depth 4; the counting kernel."""
    import torch
    w, h, spp = 40, 32, 5
    cam = scenes.camera(oracle, w, h)
    sc = image_scene(oracle, "metal")
    exp, exp8 = hip.render_scene(cam, spp, sc, seed=11)
    opts = abi.default_opts(spp=spp, seed=11)

    def img():
        return torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")

    def same(t, what):
        torch.cuda.synchronize()
        assert np.array_equal(bits(t.cpu().numpy()), bits(exp)), what

    with hip.HipScene(sc) as hs:
        out, out8 = img(), torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        hs.render_device(cam, opts, out.data_ptr(), out8.data_ptr())
        same(out, "render_device")
        assert np.array_equal(out8.cpu().numpy(), exp8)
        for cuts in ((0, 1, 4, 5), (0, 3, 5)):
            acc, out = img(), img()
            for b, e in zip(cuts[:-1], cuts[1:]):
                hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == spp else None)
            same(out, f"render_pass {cuts}")
        world = 3
        slot = hip.packed_pixels(w, h, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            hs.render_device(cam, abi.default_opts(spp=spp, seed=11, tile_rank=r, tile_world=world), slots[r * slot * 3:].data_ptr())
        merged = img()
        hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        same(merged, "tile_world 3 + unpack")
        hs.set_pipeline(4)
        outs = [img() for _ in range(6)]
        for o in outs:
            hs.render_device(cam, opts, o.data_ptr())
        for n, o in enumerate(outs):
            same(o, f"stream frame {n}")
        out = img()
        hs.render_device(cam, abi.default_opts(spp=spp, seed=11, flags=abi.FLAG_COLLECT_STATS), out.data_ptr())
        same(out, "COLLECT_STATS")
        hs.check()


def _render_raw(lib, cam, sc, shading, opts):
    rad = np.zeros((cam.img_height_pix, cam.img_width_pix, 3), f32)
    abi.check(lib.rbrt_hip_render_shaded(C.byref(cam), sc.ptr(), shading, C.byref(opts), rad.ctypes.data_as(abi.f32p), None))
    return rad


def test_no_normals_change_nothing(hip, oracle):
    """NULL shading, a shading whose meshes are all NULL, and shading->meshes NULL: rbrt_hip_render's image; a handle made
    by create_shaded renders scene_create's image with the same LDS per wave -- and a smooth scene's handle too."""
    import torch
    lib = abi.load_hip()
    cam = scenes.camera(oracle, 48, 32)
    sc = flat_copy(image_scene(oracle, "dielectric"))
    opts = abi.default_opts(spp=4, seed=2)
    ref, _ = hip.render_scene(cam, 4, sc, seed=2)
    none = (abi.MeshNormals * len(sc.meshes))()
    for sh in (None, C.byref(abi.SceneShading(len(sc.meshes), 0, none)), C.byref(abi.SceneShading(len(sc.meshes), 0, None))):
        assert np.array_equal(bits(_render_raw(lib, cam, sc, sh, opts)), bits(ref))
    assert np.array_equal(bits(oracle.render(cam, sc, opts)[0]), bits(ref))  # (the reference's image)

    def device_image(make):
        h = C.c_void_p()
        abi.check(make(h))
        try:
            info = abi.SceneInfo()
            abi.check(lib.rbrt_hip_scene_info(h, C.byref(info)))
            out = torch.full((32, 48, 3), float("nan"), dtype=torch.float32, device="cuda")
            abi.check(lib.rbrt_hip_render_device(h, C.byref(cam), C.byref(opts), None, C.c_void_p(out.data_ptr()), None))
            abi.check(lib.rbrt_hip_scene_check(h))
            return out.cpu().numpy(), info.lds_bytes_per_wave
        finally:
            lib.rbrt_hip_scene_destroy(h)

    img0, lds0 = device_image(lambda h: lib.rbrt_hip_scene_create(sc.ptr(), 0, C.byref(h)))
    img1, lds1 = device_image(lambda h: lib.rbrt_hip_scene_create_shaded(sc.ptr(), C.byref(abi.SceneShading(len(sc.meshes), 0, none)), 0, C.byref(h)))
    assert np.array_equal(bits(img0), bits(ref)) and np.array_equal(bits(img1), bits(ref))
    smooth = image_scene(oracle, "dielectric")
    _, lds2 = device_image(lambda h: lib.rbrt_hip_scene_create_shaded(smooth.ptr(), smooth.shading_ptr(), 0, C.byref(h)))
    assert lds0 == lds1 == lds2, (lds0, lds1, lds2)


SETTINGS = {"host_builder": {"RBRT_BVH_BUILDER": "host"}, "device_builder": {"RBRT_BVH_BUILDER": "device"},
            "no_tile_pass": {"RBRT_HIP_LAB": "1", "RBRT_PRIMARY_CULL": "0"}}


@pytest.mark.parametrize("setting", list(SETTINGS) + ["refined"])
def test_the_same_image_under_every_tree_and_cull_setting(hip, oracle, tmp_path, setting):
    """The hook scene (a 1203-entry smooth mesh: the device builder's first tree, then the host's) at 64 x 48."""
    cam = scenes.camera(oracle, 64, 48)
    sc = hook_scene(oracle)
    ref, _ = hip.render_scene(cam, 2, sc, seed=5)
    script = tmp_path / "render.py"
    script.write_text(f"""import sys
sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r})
import numpy as np, torch
import rbrt_amd, scenes
from rbrt_amd import abi
from oracle import pyoracle
import test_smooth_shading as S
cam = scenes.camera(pyoracle, 64, 48)
sc = S.hook_scene(pyoracle)
one, _ = rbrt_amd.render_scene(cam, 2, sc, seed=5)
with rbrt_amd.HipScene(sc) as hs:
    if {setting == "refined"!r}:
        state, _ = hs.refine_wait(120.0)
        assert state == 1, state  # (the host builder's trees are in use)
    out = torch.full((48, 64, 3), float("nan"), dtype=torch.float32, device="cuda")
    hs.render_device(cam, abi.default_opts(spp=2, seed=5), out.data_ptr())
    torch.cuda.synchronize()
    hs.check()
np.save({str(tmp_path / 'one.npy')!r}, one)
np.save({str(tmp_path / 'dev.npy')!r}, out.cpu().numpy())
""")
    env = dict(os.environ, **SETTINGS.get(setting, {}))
    if setting == "refined":
        env.pop("RBRT_BVH_BUILDER", None)
        env.pop("RBRT_BVH_REFINE", None)
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    for name in ("one", "dev"):
        assert np.array_equal(bits(np.load(tmp_path / f"{name}.npy")), bits(ref)), name


# ---- physics ---------------------------------------------------------------------------------------------------------------
SMOOTH_ERROR_FRACTION = 0.25


def _covered(hip, sc, cam):
    """Pixels all four of whose corner rays hit object 0 (the pixel's samples all start on it)."""
    w, h = cam.img_width_pix, cam.img_height_pix
    v = lambda a: np.array(list(a), np.float64)  # noqa: E731
    pos, right, up, ctr = v(cam.position), v(cam.right), v(cam.up), v(cam.img_center_point)
    ok = np.ones((h, w), bool)
    for du in (0.0, 1.0):
        for dv in (0.0, 1.0):
            col = np.arange(w)[None, :] - w // 2 + du - 0.5
            row = np.arange(h)[:, None] - h // 2 + dv - 0.5
            tgt = ctr + (0.001 * col * cam.mm_per_pix_hor)[..., None] * right - (0.001 * row * cam.mm_per_pix_vert)[..., None] * up
            d = tgt - pos
            d /= np.linalg.norm(d, axis=-1, keepdims=True)
            rays = np.concatenate([np.broadcast_to(pos, d.shape), d], -1).reshape(-1, 6).astype(f32)
            with hip.HipScene(sc) as hs:
                _, obj, _, _ = hs.trace_rays(rays)
            ok &= (obj == 0).reshape(h, w)
    return ok


def test_smooth_shading_approaches_the_analytic_sphere(hip, oracle):
    """A mirror ball under the sky gradient: the analytic sphere against its tessellation (768 triangles) with the exact
    vertex normals and shaded flat. Over pixels that start on the object in all three scenes, the smooth image's mean
    error is below SMOOTH_ERROR_FRACTION of the flat image's."""
    c, r = (0.0, 1.5, -9.0), 1.5
    mat = abi.material(M_, (0.9, 0.9, 0.9), 0.0)
    cam = scenes.camera(oracle, 160, 120, look_at=(0.0, -0.35, -1.0))
    flat_m, smooth_m = np_smooth.sphere_mesh(oracle, c, r, 8, mat)
    scs = dict(analytic=abi.SceneData(spheres=[(c, r, mat)]), flat=abi.SceneData(meshes=[flat_m]),
               smooth=abi.SceneData(meshes=[smooth_m]))
    img = {k: hip.render_scene(cam, 8, s, seed=3)[0].astype(np.float64) for k, s in scs.items()}
    mask = _covered(hip, scs["analytic"], cam) & _covered(hip, scs["flat"], cam)
    assert mask.sum() > 300, mask.sum()
    err = {k: float(np.abs(img[k] - img["analytic"])[mask].mean()) for k in ("flat", "smooth")}
    print(f"{int(mask.sum())} pixels: mean error flat {err['flat']:.5f}, smooth {err['smooth']:.5f} "
          f"({err['smooth'] / err['flat']:.3f} of flat)")
    assert err["flat"] > 1e-3
    assert err["smooth"] < SMOOTH_ERROR_FRACTION * err["flat"]


# ---- the C++ host ----------------------------------------------------------------------------------------------------------
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CLI_YAML = """---
camera_blueprint:
  camera_up: {{x: 0.0, y: 1.0, z: -0.4}}
  camera_look_at: {{x: 0.0, y: -0.1, z: -1.0}}
  camera_position: {{x: 0.0, y: 5.0, z: 4.0}}
  camera_focal_length_mm: 28.0
mesh_blueprints:
  - obj_filepath: {obj}
    scale: 45.0
    translation: {{x: 2.0, y: -1.8, z: -10.5}}
    rotation_rad: {{x: 0.0, y: 0.6, z: 0.0}}
    material_type: "metal"
    material_param: 0.02
    albedo: {{x: 0.9, y: 0.8, z: 0.6}}
{shading}sphere_blueprints:
  - radius: 1000.0
    center: {{x: 0.0, y: -1000.0, z: -5.0}}
    material_type: "lambertian"
    albedo: {{x: 0.02, y: 0.2, z: 0.1}}
  - radius: 1.5
    center: {{x: -3.5, y: 1.5, z: -9.0}}
    material_type: "dielectric"
    material_param: 1.6
"""


def _cli_files(tmp_path):
    obj = tmp_path / "blob.obj"
    v, f = standin.make_mesh(1203)
    standin.write_obj(obj, v, f)
    files = {}
    for name, sh in (("flat", ""), ("smooth", "    shading: smooth\n")):
        files[name] = tmp_path / f"{name}.yaml"
        files[name].write_text(CLI_YAML.format(obj=obj, shading=sh))
    return files


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _cli(tmp_path, cfg, name, *args, env=None):
    out = tmp_path / f"{name}.png"
    r = subprocess.run([str(EXE), "-c", str(cfg), "-t", str(out), "--height", str(H), "-w", str(W), *args], capture_output=True,
                       text=True, timeout=300, env=env)
    return r, out


def test_cli_yaml_key_and_flag_give_the_python_image(hip, tmp_path):
    files = _cli_files(tmp_path)
    hs = abi.HostScene(files["smooth"], H, W)
    assert hs.shading is not None
    _, exp8 = hip.render_scene(hs.camera, 4, hs, seed=1)
    flat = abi.HostScene(files["flat"], H, W)
    _, flat8 = hip.render_scene(flat.camera, 4, flat, seed=1)
    assert not np.array_equal(exp8, flat8)
    for name, cfg, args in (("yaml", files["smooth"], ()), ("flag", files["flat"], ("--shading", "smooth"))):
        r, out = _cli(tmp_path, cfg, name, "-s", "4", *args)
        assert r.returncode == 0, r.stderr[-2000:]
        assert np.array_equal(_png(out), exp8), name
    r, out = _cli(tmp_path, files["smooth"], "off", "-s", "4", "--shading", "flat")
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), flat8)


def test_cli_three_ranks_give_the_one_rank_image(hip, tmp_path):
    files = _cli_files(tmp_path)
    r1, out1 = _cli(tmp_path, files["smooth"], "g1", "-s", "3", "--gpus", "1")
    r3, out3 = _cli(tmp_path, files["smooth"], "g3", "-s", "3", "--gpus", "3", "--oversubscribe")
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr[-1000:], r3.stderr[-1000:])
    assert np.array_equal(_png(out1), _png(out3))


def test_cli_checkpoint_does_not_resume_across_shading(hip, tmp_path):
    files = _cli_files(tmp_path)
    ck = tmp_path / "render.ckpt"
    args = ["-s", "9", "--seed", "3", "--pass-samples", "3", "--checkpoint", str(ck)]
    stop = dict(os.environ, RBRT_TEST_STOP_AFTER_PASS="1")
    r, full = _cli(tmp_path, files["smooth"], "full", "-s", "9", "--seed", "3")
    assert r.returncode == 0, r.stderr[-1000:]
    full8 = _png(full)
    r, _ = _cli(tmp_path, files["smooth"], "a", *args, env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, files["smooth"], "a", *args)
    assert r.returncode == 0 and "Resuming from checkpoint" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(_png(out), full8)
    r, _ = _cli(tmp_path, files["flat"], "b", *args, env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, files["flat"], "b", *args, "--shading", "smooth")  # (a flat run's sums are not resumed)
    assert r.returncode == 0 and "does not match this render" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(_png(out), full8)
