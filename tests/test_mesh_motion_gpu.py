"""Moving meshes (rbrt_hip_scene_set_mesh_motion) on the GPU.

Images: bit for bit against the numpy restatement (np_mesh_motion.restated_image), on a subset of pixels where the whole image
would take long on the CPU: meshes of 1, 5, about 300 and 2000 triangles (a root with one leaf, one more than a leaf holds, past
the device builder's threshold under both builders and on the refined tree, stacks that spill to global memory), each
material, flat and smooth, checkers on the mesh and under it, spheres in front and behind, a BasicTriangle, lens, shutter,
sphere motion, environment and all of them, four phases. Two, three and eight meshes in one ray's way. Parked and resumed
paths under test_motion_gpu's PARK_ROWS. Every entry point. The feature buffers and the motion buffer, the moving
accumulation, the tile pass, the short-path stage, the handle's state and the C ABI's refusals."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import np_animation as NA
import np_env
import np_features
import np_lens
import np_mesh_motion as MM
import np_motion as NM
import np_reference as R
import np_smooth as S
import np_temporal as NT
import scenes
import test_motion_gpu as TM
import test_primary_cull as PC
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

f32 = np.float32
L_, M_, D_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
bits, render = TM.bits, TM.render
DEPTH = 8
W, H = 48, 32
MESH_AT = (0.5, -0.6, -4.5)  # in front of the example spheres, where test_motion_gpu puts its small mesh
TRAVEL = (0.9, 0.15, -0.2)
SPHERE_TRAVELS = np.array([(0.0, 0.0, 0.0), (0.9, 0.0, 0.0), (-0.4, 0.3, 0.5), (0.0, 0.6, -0.7), (0.3, 0.0, 0.2), (-0.2, 0.1, 0.0)], f32)


def grid(w, h, step=1, off=0):
    return [(r, c) for r in range(off, h, step) for c in range(off, w, step)]


def mats():
    return {"lambertian": abi.material(L_, (0.7, 0.3, 0.2)), "metal": abi.material(M_, (0.8, 0.7, 0.6), 0.05),
            "glass": abi.material(D_, (0.0, 0.0, 0.0), 1.5), "emissive": abi.material(EM, (2.0, 1.5, 1.0))}


def standin(oracle, n, mat, *, smooth=False, scale=25.0, at=MESH_AT):
    if smooth:
        return S.standin_smooth(oracle, n, scale, at, mat, "computed")
    return scenes.standin_mesh(oracle, n, scale, at, (0.0, 0.4, 0.0), mat)


def stage(oracle, meshes, *, triangle=False, patterns=None):
    """The example spheres, one small sphere in front of the mesh's place and one behind it; `meshes` in their order."""
    sph = list(scenes.EXAMPLE_SPHERES) + [((0.2, 0.5, -2.0), 0.35, abi.material(M_, (0.9, 0.9, 0.9), 0.0)),
                                          ((0.8, 0.9, -7.0), 0.9, abi.material(L_, (0.2, 0.6, 0.8)))]
    kw = {}
    if triangle:
        kw = dict(triangles=[(((-4.0, 0.3, -6.0), (-1.5, 0.4, -6.5), (-2.7, 2.6, -7.0)), abi.material(M_, (0.9, 0.6, 0.3), 0.05))],
                  element_order=[0, 1, scenes.T | 0, 2, 3, 4, 5])
    if patterns:
        kw["patterns"] = patterns
    return abi.SceneData(spheres=sph, meshes=list(meshes), **kw)


def lens_of(cam):
    return np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 40.0, 9.0)


def compare(got, exp, pixels, what=""):
    bad = [(r, c) for r, c in pixels if not np.array_equal(bits(got[r, c]), bits(exp[r, c]))]
    assert not bad, (what, len(bad), bad[:5])


def run(hip, sc, cam, opts, mesh_travels, *, travels=None, phase=0.0, lens=None, shutter=None, nodes=None):
    with hip.HipScene(sc) as hs:
        if nodes is not None:
            hs.set_environment(nodes)
        hs.set_shutter(shutter)
        if travels is not None:
            hs.set_motion(travels)
        hs.set_mesh_motion(mesh_travels)
        hs.set_motion_phase(phase)
        got, got8 = render(hs, cam, opts, lens)
        hs.check()
        assert hs.last_trace_build() == "general"
    return got, got8


# ---- sizes, materials, shading ---------------------------------------------------------------------------------------------
SIZES = [
    ("1_triangle_metal", 1, "metal", False, 60.0),
    ("5_triangles_lambertian", 5, "lambertian", False, 60.0),
    ("5_triangles_glass_smooth", 5, "glass", True, 60.0),
    ("300_triangles_metal_smooth", 300, "metal", True, 25.0),
    ("300_triangles_emissive", 300, "emissive", False, 25.0),
    ("2000_triangles_lambertian", 2000, "lambertian", False, 25.0),
    ("2000_triangles_glass_smooth", 2000, "glass", True, 25.0),
]


@pytest.mark.parametrize("name,n,mat,smooth,scale", SIZES, ids=[s[0] for s in SIZES])
def test_images_by_mesh_size_material_and_shading(hip, oracle, name, n, mat, smooth, scale):
    """48 x 32 x 4, depth 8: ragged tiles, 6 x 4 of them; a sphere in front of the mesh and one behind."""
    sc = stage(oracle, [standin(oracle, n, mats()[mat], smooth=smooth, scale=scale)])
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=4, seed=7, max_depth=DEPTH)
    pix = grid(W, H)
    exp, _ = MM.restated_image(cam, sc, opts, [TRAVEL], pixels=pix)
    got, _ = run(hip, sc, cam, opts, [TRAVEL])
    compare(got, exp, pix, name)
    if n >= 300:
        still, _ = MM.restated_image(cam, sc, opts, [(0.0, 0.0, 0.0)], pixels=pix)
        assert any(not np.array_equal(bits(still[r, c]), bits(exp[r, c])) for r, c in pix)  # (the travel does something here)


@functools.lru_cache(maxsize=None)
def builder_reference():
    from oracle import pyoracle
    sc = stage(pyoracle, [standin(pyoracle, 301, mats()["metal"], smooth=True)])
    cam = scenes.camera(pyoracle, W, H)
    opts = abi.default_opts(spp=4, seed=9, max_depth=DEPTH)
    pix = grid(W, H)
    exp, _ = MM.restated_image(cam, sc, opts, [TRAVEL], phase=0.5, pixels=pix)
    exp.setflags(write=False)
    return sc, cam, opts, pix, exp


@pytest.mark.parametrize("builder", ["host", "device", "refined"])
def test_both_builders_and_the_refined_tree(hip, oracle, monkeypatch, builder):
    import torch
    sc, cam, opts, pix, exp = builder_reference()
    monkeypatch.delenv("RBRT_BVH_REFINE", raising=False)
    if builder == "refined":
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
        monkeypatch.setenv("RBRT_BVH_DEVICE_MIN", "0")
    else:
        monkeypatch.setenv("RBRT_BVH_BUILDER", builder)
    with hip.HipScene(sc) as hs:
        hs.set_mesh_motion([TRAVEL])
        hs.set_motion_phase(0.5)
        if builder == "refined":
            assert hs.create_times()["meshes_device_built"] == 1
            got, _ = render(hs, cam, opts)
            compare(got, exp, pix, "the device builder's tree")
            assert hs.refine_wait(120.0)[0] == 1
        got, _ = render(hs, cam, opts)
        torch.cuda.synchronize()
        hs.check()
    compare(got, exp, pix, builder)


# ---- everything around the mesh ------------------------------------------------------------------------------------------------
AROUND = ["checkers", "triangle", "lens", "shutter", "sphere_motion", "environment", "everything"]


@pytest.mark.parametrize("case", AROUND)
def test_images_with_everything_around_the_mesh(hip, oracle, case):
    every = case == "everything"
    n_sph = 6
    patterns = None
    if case == "checkers" or every:  # on the ground under the mesh and on the mesh itself (object id n_elem + 0)
        n_elem = n_sph + (1 if every else 0)
        patterns = {0: abi.checker((0.8, 0.9, 0.97), 1.5, (0.4, -1.5, 0.2)), n_elem: abi.checker((0.1, 0.3, 0.8), 0.3, (0.11, -0.07, 0.23))}
    sc = stage(oracle, [standin(oracle, 300, mats()["lambertian"], smooth=every)], triangle=case == "triangle" or every, patterns=patterns)
    cam = scenes.camera(oracle, W, H)
    lens = lens_of(cam) if case == "lens" or every else None
    shutter = TM.SKEW if case == "shutter" or every else None
    travels = SPHERE_TRAVELS if case == "sphere_motion" or every else None
    nodes = np_env.noise_map(8, 3) if case == "environment" or every else None
    phase = 0.5 if every else 0.0
    opts = abi.default_opts(spp=4, seed=11, max_depth=DEPTH)
    pix = grid(W, H)
    exp, _ = MM.restated_image(cam, sc, opts, [TRAVEL], travels=travels, phase=phase, lens=lens, shutter=shutter, nodes=nodes, pixels=pix)
    got, _ = run(hip, sc, cam, opts, [TRAVEL], travels=travels, phase=phase, lens=lens, shutter=shutter, nodes=nodes)
    compare(got, exp, pix, case)
    if case == "checkers":  # both colours of the mesh's checker are seen: the pattern stays and the mesh moves through it
        seen = set()
        sl = {}
        MM.restated_image(cam, sc, abi.default_opts(spp=2, seed=11, max_depth=1), [TRAVEL], pixels=pix, scatters=sl)
        assert any(v and v[0] == n_sph for v in sl.values()), seen


@pytest.mark.parametrize("phase", [-3.0, 0.0, 0.5, 40.0])
def test_phases(hip, oracle, phase):
    """The mesh is placed so that the phase has carried it to MESH_AT: its uploaded position is MESH_AT - phase * travel."""
    tv = np.array(TRAVEL, f32) * f32(0.5)
    at = tuple(float(x) for x in (np.array(MESH_AT) - phase * tv.astype(np.float64)))
    sc = stage(oracle, [standin(oracle, 300, mats()["metal"], at=at)])
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=4, seed=13, max_depth=DEPTH)
    pix = grid(W, H)
    sl = {}
    exp, _ = MM.restated_image(cam, sc, opts, [tv], travels=SPHERE_TRAVELS * f32(0.02), phase=phase, pixels=pix, scatters=sl)
    assert any(6 in v for v in sl.values())  # (the mesh is in view at this phase)
    got, _ = run(hip, sc, cam, opts, [tv], travels=SPHERE_TRAVELS * f32(0.02), phase=phase)
    compare(got, exp, pix, phase)


# ---- several meshes in one ray's way ---------------------------------------------------------------------------------------------
def plate(oracle, z, mat, x=0.5, y=0.6, half=1.1, n=3):
    """A plate of 2 n^2 triangles facing the camera's side, at depth z, slightly tilted so that no two plates are parallel."""
    xs = np.linspace(-half, half, n + 1)
    tris = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = (xs[i], xs[j]), (xs[i + 1], xs[j]), (xs[i + 1], xs[j + 1]), (xs[i], xs[j + 1])
            p = lambda q: (x + q[0], y + q[1], z + 0.07 * z * q[0] - 0.05 * q[1])  # noqa: E731
            tris += [(p(a), p(b), p(c)), (p(a), p(c), p(d))]
    return oracle.mesh_prep(np.array(tris, f32), 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), mat)


ORDERS = [
    ("moving_in_front_of_static", [(-3.5, (0.8, 0.0, 0.0)), (-5.5, (0.0, 0.0, 0.0))]),
    ("static_in_front_of_moving", [(-3.5, (0.0, 0.0, 0.0)), (-5.5, (0.8, 0.1, 0.0))]),
    ("moving_in_front_listed_last", [(-5.5, (0.0, 0.0, 0.0)), (-3.5, (0.8, 0.0, 0.0))]),
    ("static_in_front_listed_last", [(-5.5, (0.8, 0.1, 0.0)), (-3.5, (0.0, 0.0, 0.0))]),
    ("three_different_travels", [(-4.5, (0.0, 0.7, 0.0)), (-6.0, (-0.9, 0.0, 0.3)), (-3.2, (0.6, -0.2, 0.0))]),
    ("three_far_travel_first", [(-6.0, (300.0, 0.0, 0.0)), (-3.2, (0.6, -0.2, 0.0)), (-4.5, (0.0, 0.7, 0.0))]),
]


@pytest.mark.parametrize("name,plates", ORDERS, ids=[o[0] for o in ORDERS])
def test_two_and_three_meshes_in_one_rays_way(hip, oracle, name, plates):
    """Glass and metal plates one behind the other: a ray that has hit an earlier mesh of the scene's order searches the next
    with that hit as its bound, and the finalise step compares against the earlier mesh's own distance."""
    def kind(z):  # glass in front, metal at the back: paths go through the front plates and come back
        return abi.material(D_, (0.0, 0.0, 0.0), 1.3 if z > -4.0 else 1.5) if z > -5.0 else abi.material(M_, (0.8, 0.8, 0.7), 0.02)
    # (a travel of 300 units a whole exposure at phase 0.01 is 3 units: the mesh is uploaded that far back)
    phase = 0.01 if name == "three_far_travel_first" else 0.0
    meshes = [plate(oracle, z, kind(z), x=0.5 - phase * tv[0]) for z, tv in plates]
    sc = stage(oracle, meshes)
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=4, seed=17, max_depth=DEPTH)
    pix = grid(W, H)
    tv = [t for _, t in plates]
    sl = {}
    exp, _ = MM.restated_image(cam, sc, opts, tv, phase=phase, pixels=pix, scatters=sl)
    ids = [{o for o in v if o >= 6} for v in sl.values()]
    assert sum(len(s) >= 2 for s in ids) >= (5 if phase else 40)  # (paths that meet two of the meshes)
    got, _ = run(hip, sc, cam, opts, tv, phase=phase)
    compare(got, exp, pix, name)


def test_eight_meshes_all_moving(hip, oracle):
    """One more mesh than the tile word holds: no tile is called mesh-free, the short-path stage stays out."""
    rng = np.random.default_rng(3)
    meshes = [standin(oracle, 20 + 9 * k, mats()[("lambertian", "metal", "glass")[k % 3]], smooth=bool(k & 1), scale=14.0,
                      at=(-3.0 + 0.9 * k, -0.3 + 0.2 * (k % 3), -5.0 - 0.4 * (k % 4))) for k in range(8)]
    tv = rng.uniform(-0.6, 0.6, (8, 3)).astype(f32)
    sc = stage(oracle, meshes)
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=4, seed=19, max_depth=DEPTH)
    pix = grid(W, H)
    exp, _ = MM.restated_image(cam, sc, opts, tv, pixels=pix)
    got, _ = run(hip, sc, cam, opts, tv)
    compare(got, exp, pix)


# ---- parked and resumed paths -----------------------------------------------------------------------------------------------------
def parked_pixels():
    return grid(TM.PARK_W, TM.PARK_H, 2)


@functools.lru_cache(maxsize=None)
def parked_reference():
    """The restated pixels of the parked scene, made once for every row below (and left unchanged)."""
    from oracle import pyoracle
    sc = parked_scene(pyoracle)
    cam = scenes.camera(pyoracle, TM.PARK_W, TM.PARK_H)
    opts = abi.default_opts(spp=TM.PARK_SPP, seed=TM.PARK_SEED, max_depth=DEPTH)
    exp, _ = MM.restated_image(cam, sc, opts, PARK_TRAVELS, travels=SPHERE_TRAVELS, phase=0.5, pixels=parked_pixels())
    exp.setflags(write=False)
    return exp


PARK_TRAVELS = np.array([(0.7, 0.0, 0.1), (-0.5, 0.2, 0.0)], f32)


def parked_scene(oracle):
    return stage(oracle, [standin(oracle, 2000, mats()["metal"]), standin(oracle, 40, mats()["glass"], smooth=True, at=(-1.2, -0.2, -3.6), scale=18.0)])


@pytest.mark.parametrize("rid,env", TM.PARK_ROWS, ids=[r[0] for r in TM.PARK_ROWS])
def test_the_time_survives_every_park_and_resume(hip, oracle, monkeypatch, rid, env):
    """test_motion_gpu's rows -- the knobs that shrink the grid and the shade rounds, helpers forced -- on a 2000-triangle mesh
    (stacks beyond the LDS part) and a small one in front of moving spheres: three frames back to back, then a render_pass series."""
    import torch
    exp, pix = parked_reference(), parked_pixels()
    sc = parked_scene(oracle)
    cam = scenes.camera(oracle, TM.PARK_W, TM.PARK_H)
    opts = abi.default_opts(spp=TM.PARK_SPP, seed=TM.PARK_SEED, max_depth=DEPTH)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    h, w = TM.PARK_H, TM.PARK_W
    outs = [torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    with hip.HipScene(sc) as hs:
        hs.set_motion(SPHERE_TRAVELS)
        hs.set_mesh_motion(PARK_TRAVELS)
        hs.set_motion_phase(0.5)
        hs.set_timing(True)
        for o in outs:
            hs.render_device(cam, opts, o.data_ptr())
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            compare(o.cpu().numpy(), exp, pix, (rid, k))
        acc = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        for b, e in ((0, 1), (1, 5), (5, TM.PARK_SPP)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == TM.PARK_SPP else None)
        torch.cuda.synchronize()
        compare(out.cpu().numpy(), exp, pix, (rid, "render_pass"))
        if rid == "helpers_2":
            print(f"helper launches: {hs.helper_launches()}")
        hs.check()


# ---- every entry point -----------------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_restated_image(hip, oracle):
    """render_device, a render_pass series in uneven pieces, render_adaptive with threshold 0, two and three ranks' packed tiles
    gathered and the counting kernel, on one handle with a mesh motion, a sphere motion and a shutter."""
    import torch
    w, h, spp = 40, 24, 5
    cam = scenes.camera(oracle, w, h)
    sc = stage(oracle, [standin(oracle, 300, mats()["metal"], smooth=True)])
    opts = abi.default_opts(spp=spp, seed=11, max_depth=DEPTH)
    pix = grid(w, h)
    exp, _ = MM.restated_image(cam, sc, opts, [TRAVEL], travels=SPHERE_TRAVELS, shutter=TM.SKEW, pixels=pix)

    def img():
        return torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")

    def same(t, what):
        torch.cuda.synchronize()
        compare(t.cpu().numpy(), exp, pix, what)

    with hip.HipScene(sc) as hs:
        hs.set_shutter(TM.SKEW)
        hs.set_motion(SPHERE_TRAVELS)
        hs.set_mesh_motion([TRAVEL])
        got, _ = render(hs, cam, opts)
        compare(got, exp, pix, "render_device")
        acc, out = img(), img()
        for b, e in ((0, 1), (1, 4), (4, spp)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == spp else None)
        same(out, "render_pass 0-1, 1-4, 4-5")
        assert np.array_equal(bits(out.cpu().numpy()), bits(got))
        out = img()
        res = hs.render_adaptive(cam, opts, 0.0, 2, 2, out.data_ptr())
        same(out, "render_adaptive, threshold 0")
        assert res["samples"] == res["samples_fixed"] and np.array_equal(bits(out.cpu().numpy()), bits(got))
        for world in (2, 3):
            slot = hip.packed_pixels(w, h, 0, world)
            slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
            for r in range(world):
                o = abi.default_opts(spp=spp, seed=11, max_depth=DEPTH, tile_rank=r, tile_world=world)
                hs.render_device(cam, o, slots[r * slot * 3:].data_ptr())
            merged = img()
            hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
            same(merged, f"tile_world {world} + unpack")
            assert np.array_equal(bits(merged.cpu().numpy()), bits(got))
        out = img()
        hs.render_device(cam, abi.default_opts(spp=spp, seed=11, max_depth=DEPTH, flags=abi.FLAG_COLLECT_STATS), out.data_ptr())
        same(out, "COLLECT_STATS")
        assert np.array_equal(bits(out.cpu().numpy()), bits(got))
        assert hs.stats()["samples"] == w * h * spp and hs.stats()["mesh_hits"] > 0
        hs.check()


def test_the_low_render_and_the_full_size_features_of_an_upscaled_frame(hip, oracle):
    """An upscaled frame traces a camera of half the size and makes its features at full size, on one handle and one mesh
    motion: both are the restatement's at their own size."""
    import torch
    w, h, n = 48, 32, 2
    cam = scenes.camera(oracle, w, h)
    low = hip.upsample_camera(cam, 2)
    sc = stage(oracle, [standin(oracle, 300, mats()["lambertian"], smooth=True)])
    opts = abi.default_opts(spp=4, seed=23, max_depth=DEPTH)
    pix_low = grid(low.img_width_pix, low.img_height_pix, 2)
    exp_low, _ = MM.restated_image(low, sc, opts, [TRAVEL], phase=0.5, pixels=pix_low)
    pix = grid(w, h, 2)
    feat, mv = MM.features(cam, sc, opts, n, [TRAVEL], phase=0.5, pixels=pix)
    bufs = feature_buffers(torch, w, h)
    with hip.HipScene(sc) as hs:
        hs.set_mesh_motion([TRAVEL])
        hs.set_motion_phase(0.5)
        got_low, _ = render(hs, low, opts)
        hs.render_features(cam, opts, n, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        hs.check()
    compare(got_low, exp_low, pix_low, "the low render")
    check_features(bufs, feat, mv, pix)


# ---- the feature buffers ---------------------------------------------------------------------------------------------------------
def feature_buffers(torch, w, h):
    nan3, nan1 = (lambda: torch.full((h, w, 3), float("nan"), device="cuda")), (lambda: torch.full((h, w), float("nan"), device="cuda"))
    return dict(albedo=nan3(), normal=nan3(), depth=nan1(), coverage=nan1(), object=torch.full((h, w), -7, dtype=torch.int32, device="cuda"),
                motion=nan3())


def check_features(bufs, feat, mv, pix):
    got = {k: v.cpu().numpy() for k, v in bufs.items()}
    for k in ("albedo", "normal", "depth", "coverage"):
        bad = [(r, c) for r, c in pix if not np.array_equal(bits(got[k][r, c]), bits(getattr(feat, k)[r, c]))]
        assert not bad, (k, bad[:5])
    assert all(got["object"][r, c] == feat.object[r, c] for r, c in pix)
    bad = [(r, c) for r, c in pix if not np.array_equal(bits(got["motion"][r, c]), bits(mv[r, c]))]
    assert not bad, ("motion", bad[:5])


@pytest.mark.parametrize("case", ["flat", "smooth_checker_shutter_spheres"])
def test_feature_buffers_see_the_moved_mesh(hip, oracle, case):
    """Depth, normal, object, albedo and coverage of every sample's mesh where its own s puts it, and the motion buffer:
    w_m times the coverage of the mesh (plus the spheres' travels where they are hit)."""
    import torch
    w, h, n = 40, 24, 3
    full = case != "flat"
    cam = scenes.camera(oracle, w, h)
    patterns = {6: abi.checker((0.1, 0.3, 0.8), 0.3, (0.11, -0.07, 0.23))} if full else None
    sc = stage(oracle, [standin(oracle, 300, mats()["lambertian"], smooth=full)], patterns=patterns)
    opts = abi.default_opts(spp=2, seed=5)
    travels, shutter, phase = (SPHERE_TRAVELS, TM.SKEW, 0.5) if full else (None, None, 0.0)
    pix = grid(w, h, 2)
    feat, mv = MM.features(cam, sc, opts, n, [TRAVEL], travels=travels, phase=phase, shutter=shutter, pixels=pix)
    bufs = feature_buffers(torch, w, h)
    with hip.HipScene(sc) as hs:
        hs.set_shutter(shutter)
        if travels is not None:
            hs.set_motion(travels)
        hs.set_mesh_motion([TRAVEL])
        hs.set_motion_phase(phase)
        hs.render_features(cam, opts, n, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        hs.check()
    check_features(bufs, feat, mv, pix)
    # a pixel whose samples all hit the mesh carries exactly w_m (n * w_m * (1 / n) in float32), and there are such pixels
    inside = [(r, c) for r, c in pix if feat.object[r, c] == 6 and feat.coverage[r, c] == 1.0 and np.array_equal(mv[r, c] != 0, np.array(TRAVEL) != 0)]
    assert len(inside) >= 5
    still, mv0 = MM.features(cam, sc, opts, n, [(0.0, 0.0, 0.0)], travels=travels, phase=phase, shutter=shutter, pixels=pix)
    assert not np.array_equal(bits(still.depth), bits(feat.depth))  # (the travel does something here)


def test_features_without_a_mesh_motion_are_what_they_were(hip, oracle):
    """A handle that never had a mesh motion, one whose mesh motion was cleared, and rbrt_hip_render_features_motion on a handle
    with a sphere motion only: the same buffers, bit for bit, the motion buffer +0 on the mesh."""
    import torch
    w, h, n = 40, 24, 3
    cam = scenes.camera(oracle, w, h)
    sc = stage(oracle, [standin(oracle, 300, mats()["lambertian"], smooth=True)])
    opts = abi.default_opts(spp=2, seed=5)
    feat, mv = NA.features(cam, sc, opts, n, SPHERE_TRAVELS, 0.5, pixels=grid(w, h, 2))
    a, b = feature_buffers(torch, w, h), feature_buffers(torch, w, h)
    with hip.HipScene(sc) as hs:
        hs.set_motion(SPHERE_TRAVELS)
        hs.set_motion_phase(0.5)
        hs.render_features(cam, opts, n, **{f"d_{k}": v.data_ptr() for k, v in a.items()})
        hs.set_mesh_motion([TRAVEL])
        hs.set_mesh_motion(None)
        hs.render_features(cam, opts, n, **{f"d_{k}": v.data_ptr() for k, v in b.items()})
        torch.cuda.synchronize()
        hs.check()
    check_features(a, feat, mv, grid(w, h, 2))
    for k in a:
        assert np.array_equal(a[k].cpu().numpy().view(np.uint32), b[k].cpu().numpy().view(np.uint32)), k


# ---- the accumulation -------------------------------------------------------------------------------------------------------------
def test_the_history_follows_a_mesh_across_the_view(hip, oracle):
    """A plate crosses the view for six frames, two exposures a frame. The device's feature buffers are the restatement's; the
    moving accumulation fed with them gives np_animation.accumulate's lengths bit for bit; and pixels inside the plate keep their
    history (length k + 1) where the plain rule, on the same buffers, loses it."""
    import torch
    w, h, n, frames, step = 48, 32, 2, 6, 2.0
    cam = scenes.camera(oracle, w, h)
    tv = np.array([(0.12, 0.0, 0.0)], f32)
    sc = abi.SceneData(spheres=[scenes.EXAMPLE_SPHERES[0]], meshes=[plate(oracle, -4.5, mats()["lambertian"], x=-0.9, y=1.2, half=1.0)])
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    two = [torch.full((hip.temporal_history_bytes(w, h),), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    got_frames, lengths = [], []
    with hip.HipScene(sc) as hs:
        hs.set_mesh_motion(tv)
        for k in range(frames):
            o = abi.default_opts(spp=4, seed=100 + k, max_depth=4)
            hs.set_motion_phase(float(f32(k) * f32(step)))
            rad, ha, hb, nor, dep, cov, mv, ol = new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w), new(h, w), new(h, w, 3), new(h, w)
            assert hs.render_adaptive(cam, o, 0.0, 4, 4, rad.data_ptr())["rounds"] == 1
            hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
            hs.render_features(cam, o, n, None, nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), d_motion=mv.data_ptr())
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, cam if k else None,
                                    two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr(),
                                    d_motion=mv.data_ptr(), phase_step=step)
            torch.cuda.synchronize()
            got_frames.append(tuple(t.cpu().numpy() for t in (nor, dep, cov, mv)))
            lengths.append(ol.cpu().numpy())
        hs.check()
    hist = plain_hist = None
    zeros = np.zeros((h, w, 3), f32)
    for k, (N, z, c, Mv) in enumerate(got_frames):
        o = abi.default_opts(spp=4, seed=100 + k, max_depth=4)
        feat, mv = MM.features(cam, sc, o, n, tv, phase=float(f32(k) * f32(step)))
        assert TM.F.same_bits(N, feat.normal) and TM.F.same_bits(z, feat.depth) and TM.F.same_bits(c, feat.coverage) and TM.F.same_bits(Mv, mv), k
        _, _, el, hist, _ = NA.accumulate(zeros, zeros, feat.normal, feat.depth, feat.coverage, cam, cam, hist, Mv=mv, phase_step=step, **NT.DEFAULTS)
        _, _, pl, plain_hist, _ = NT.accumulate(zeros, zeros, feat.normal, feat.depth, feat.coverage, cam, cam, plain_hist, **NT.DEFAULTS)
        assert TM.F.same_bits(lengths[k], el), k
    on_plate = (feat.object == 1) & (feat.coverage == 1.0)
    kept = on_plate & (lengths[-1] == f32(frames))
    print(f"{int(on_plate.sum())} pixels inside the plate at frame {frames - 1}: {int(kept.sum())} with the full history, "
          f"{int((on_plate & (pl == f32(frames))).sum())} under the plain rule")
    assert int(kept.sum()) >= 8 and int((kept & (pl < f32(frames))).sum()) >= 4


# ---- the tile pass -----------------------------------------------------------------------------------------------------------------
def gate_passes(rays, ss, md, travel):
    """np_reference.bbox_hit of mesh md for each ray from its own origin o_m: rays (N, 6), ss (N,) -> bool (N,)."""
    out = np.zeros(len(rays), bool)
    for i in range(len(rays)):
        out[i] = R.bbox_hit(md.bbox_lo, md.bbox_hi, MM.origin_at(rays[i, :3], travel, ss[i]), rays[i, 3:])
    return out


def check_mesh_table(hip, oracle, monkeypatch, cam, sc, mesh_travels, *, travels=None, phase=0.0, shutter=None, n=3, seed=3):
    """No ray of the restatement passes mesh m's gate, from its own origin at its own s, in a tile whose word has bit 24 + m;
    and the image with the table is the image without it (RBRT_PRIMARY_CULL=0). Returns (table, rays hit a mesh?)."""
    opts = abi.default_opts(spp=n, seed=seed, max_depth=DEPTH)
    rays, ss = NA.primary_rays(cam, seed, n, phase, shutter=shutter)
    flat, sf = rays.reshape(-1, 6), ss.reshape(-1)
    images = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("RBRT_PRIMARY_CULL", cull)
        with hip.HipScene(sc) as hs:
            hs.set_shutter(shutter)
            if travels is not None:
                hs.set_motion(travels)
            hs.set_mesh_motion(mesh_travels)
            hs.set_motion_phase(phase)
            if cull == "1":
                table = hs.primary_cull(cam)
            try:
                images[cull], _ = render(hs, cam, opts)
                hs.check()
            except abi.RbrtError as e:  # (a NaN discriminant, sphere.rs:33: both renders meet it)
                assert e.code == abi.RBRT_ERR_NAN
                images[cull] = None
    assert (images["1"] is None) == (images["0"] is None)
    if images["1"] is not None:
        assert TM.F.same_bits(images["1"], images["0"])
    pix = np_features.all_pixels(cam)
    tile_of = np.repeat(np.array([(r // 8) * table.shape[1] + (c // 8) for r, c in pix]), n)
    words = table.reshape(-1)[tile_of]
    mw = MM.mesh_travels_of(mesh_travels)
    for m, md in enumerate(sc.meshes[:7]):
        bad = gate_passes(flat, sf, md, mw[m]) & (((words >> (24 + m)) & 1) != 0)
        assert not bad.any(), f"mesh {m}: culled in tiles {sorted(set(tile_of[bad].tolist()))[:5]} where a ray of the restatement passes its gate"
    return table


# (name, the mesh's place at the opening, its travel, the phase): the camera at the origin looks down -z
HAND_PICKED = [
    ("across_the_view", (-2.5, -0.3, -9.0), (2.0, 0.0, 0.0), 0.0),
    ("towards_the_camera", (-6.0, -0.3, -30.0), (0.0, 0.0, 8.0), 0.0),  # (the bound is a ball of radius |w| around the origin: 18 degrees wide from here)
    ("through_the_camera", (0.0, -0.3, -3.0), (0.0, 0.0, 6.0), 0.0),
    ("out_of_view_at_phase_30", (-2.5, -0.3, -9.0), (2.0, 0.0, 0.0), 30.0),
]


@pytest.mark.parametrize("name,at,travel,phase", HAND_PICKED, ids=[c[0] for c in HAND_PICKED])
def test_no_ray_passes_the_gate_of_a_mesh_its_tile_culled(hip, oracle, monkeypatch, name, at, travel, phase):
    cam = TM.axis_camera(oracle)
    sc = abi.SceneData(spheres=[((3.0, 0.0, -10.0), 0.5, abi.material(L_, (0.7, 0.4, 0.3)))],
                       meshes=[standin(oracle, 300, mats()["metal"], scale=12.0, at=at)])
    table = check_mesh_table(hip, oracle, monkeypatch, cam, sc, [travel], phase=phase)
    m_bit = (table >> 24) & 1 != 0
    print(f"{name}: mesh culled in {int(m_bit.sum())} of {table.size} tiles")
    if name == "out_of_view_at_phase_30":
        assert m_bit.all()
    elif name != "through_the_camera":
        assert m_bit.any() and not m_bit.all()


# 24 seeds chosen on the CPU so that in every case at least one restated camera ray hits a mesh: the first 24 values of k from 0
# up for which fuzz_hits(oracle, k), below, is true (most random cameras look past the small meshes)
FUZZ_SEEDS = [3, 5, 12, 15, 18, 23, 32, 41, 52, 63, 67, 72, 75, 90, 92, 105, 108, 109, 111, 125, 128, 141, 155, 156]


def fuzz_case_of(oracle, k):
    rng = np.random.default_rng(93000 + k)
    sc = PC.fuzz_scene(oracle, rng)
    while not sc.meshes:
        sc = PC.fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 49)), int(rng.integers(9, 33))
    cam = PC.fuzz_camera(oracle, rng, sc, w, h)
    mesh_travels = np.array([PC._log_uniform(rng, 1e-4, 30.0) * PC._unit(rng) * (rng.random() >= 0.25) for _ in sc.meshes], f32).reshape(-1, 3)
    travels = np.array([PC._log_uniform(rng, 1e-4, 10.0) * PC._unit(rng) * (rng.random() >= 0.5) for _ in sc.spheres], f32).reshape(-1, 3)
    shutter = tuple(float(f32(v)) for v in PC._log_uniform(rng, 1e-3, 3.0) * PC._unit(rng)) if k % 3 == 0 else None
    phase = float(f32(rng.choice([0.0, 0.0, 0.5, -1.0, 3.0])))
    return sc, cam, mesh_travels, travels if k % 2 else None, shutter, phase


def fuzz_hits(oracle, k, n=2):
    """Does a restated camera ray of fuzz case k hit a mesh?"""
    sc, cam, mw, tv, shutter, phase = fuzz_case_of(oracle, k)
    rays, ss = NA.primary_rays(cam, k, n, phase, shutter=shutter)
    obj, _, _, _ = MM.np_hits(sc, rays, ss, tv if tv is not None else np.zeros((len(sc.spheres), 3), f32), mw, 0.001, 2000.0)
    return bool((obj >= len(sc.spheres)).any())


@pytest.mark.parametrize("k", FUZZ_SEEDS)
def test_fuzzed_cameras_and_mesh_travels(hip, oracle, monkeypatch, k):
    """test_primary_cull's random scenes (with at least one mesh) and cameras; every mesh a travel log-uniform from 1e-4 to 30
    units in a random direction (one in four stays), every other case with a sphere motion, every third with a shutter, five
    phases. The seeds are those for which a restated camera ray hits a mesh."""
    sc, cam, mw, tv, shutter, phase = fuzz_case_of(oracle, k)
    table = check_mesh_table(hip, oracle, monkeypatch, cam, sc, mw, travels=tv, phase=phase, shutter=shutter, n=2, seed=k)
    assert fuzz_hits(oracle, k)
    print(f"fuzz {k}: {cam.img_width_pix}x{cam.img_height_pix}, {len(sc.spheres)} spheres, {len(sc.meshes)} meshes, phase {phase}: "
          f"{int(np.count_nonzero(table >> 24))} tiles with mesh bits")


# ---- the short-path stage ------------------------------------------------------------------------------------------------------------
def test_the_short_path_stage_next_to_a_moving_mesh(hip, oracle):
    """The mesh at rest lies left of the view's middle and sweeps to the right: tiles on the right are mesh-free for every t
    only beyond the sweep, and the second rays of the ground's tiles reach the swept box. Stage off, forced, and numpy."""
    w, h = 64, 48
    cam = scenes.camera(oracle, w, h)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES[:2]), meshes=[standin(oracle, 300, mats()["metal"], at=(-0.8, -0.6, -4.5))])
    tv = [(1.6, 0.0, 0.0)]
    opts = abi.default_opts(spp=4, seed=7, max_depth=DEPTH)
    pix = grid(w, h)
    sl = {}
    exp, _ = MM.restated_image(cam, sc, opts, tv, pixels=pix, scatters=sl)
    got = {}
    for mode in (0, 2):
        with hip.HipScene(sc) as hs:
            hs.set_mesh_motion(tv)
            hs.set_short_paths(mode)
            got[mode], _ = render(hs, cam, opts)
            if mode == 2:
                table = hs.primary_cull(cam)
                masks = hs.short_masks()
                assert masks.any()  # (the stage finished samples of this launch)
                print(f"short-path stage: {int(sum(bin(int(m)).count('1') for m in masks))} of {w * h * opts.spp} samples finished")
            hs.check()
    assert np.array_equal(bits(got[0]), bits(got[2]))
    compare(got[2], exp, pix)
    free = ((table >> 24) & 1 != 0) & (table >> 31 == 0)
    assert free.any() and not ((table >> 24) & 1 != 0).all()
    # a second ray from a mesh-free tile hits the moving mesh: a path whose first scatter is on a sphere and second on the mesh
    assert any(len(v) >= 2 and v[0] < 2 and v[1] == 2 and free[r // 8, c // 8] for (r, c, _), v in sl.items())


# ---- the handle's state ----------------------------------------------------------------------------------------------------------------
def test_the_handles_state(hip, oracle):
    """Set, replace and clear, independent of set_motion; the phase survives; a table made for one mesh motion is not reused for
    another; after the clear the plain build runs again and the image is that of a handle that never had a motion; an all-zero
    mesh motion at phase 0 is an all-zero sphere motion; trace_rays sees the mesh at rest."""
    w, h = 32, 24
    cam = scenes.camera(oracle, w, h)
    sc = scenes.example_scene(oracle, 603)  # spheres and ONE mesh: a plain scene
    n_sph = len(sc.spheres)
    opts = abi.default_opts(spp=3, seed=4, max_depth=DEPTH)
    rays = F_rays()
    a_tv, b_tv = [(0.8, 0.0, 0.0)], [(-6.0, 0.5, 0.0)]
    tv = np.random.default_rng(8).uniform(-1, 1, (n_sph, 3)).astype(f32)
    with hip.HipScene(sc) as hs:
        before = hs.info()["lds_bytes_per_wave"]
        first, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "plain"
        traced = hs.trace_rays(rays)
        hs.set_motion(np.zeros((n_sph, 3), f32))
        zero_motion, _ = render(hs, cam, opts)
        hs.set_motion(None)
        hs.set_mesh_motion([(0.0, 0.0, 0.0)])
        zero_mesh, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "general"
        assert np.array_equal(bits(zero_mesh), bits(zero_motion)) and not np.array_equal(bits(zero_mesh), bits(first))
        hs.set_mesh_motion(a_tv)
        table_a = hs.primary_cull(cam)
        moved_a, _ = render(hs, cam, opts)
        hs.set_mesh_motion(b_tv)  # replace: the tables of a_tv must not serve
        moved_b, _ = render(hs, cam, opts)
        table_b = hs.primary_cull(cam)
        assert not np.array_equal(table_a, table_b) and not np.array_equal(bits(moved_a), bits(moved_b))
        for x, y in zip(traced, hs.trace_rays(rays)):
            assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
        # independent of the sphere motion, both ways; the phase survives all of it
        hs.set_motion_phase(0.5)
        hs.set_motion(tv)
        both, _ = render(hs, cam, opts)
        hs.set_mesh_motion(None)
        spheres_only, _ = render(hs, cam, opts)
        hs.set_mesh_motion(b_tv)
        hs.set_motion(None)
        mesh_only, _ = render(hs, cam, opts)
        hs.set_motion(tv)
        both_again, _ = render(hs, cam, opts)
        assert np.array_equal(bits(both), bits(both_again))
        assert len({bits(x).tobytes() for x in (both, spheres_only, mesh_only)}) == 3
        hs.set_motion(None)
        hs.set_mesh_motion(None)
        again, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "plain"
        assert np.array_equal(bits(again), bits(first))
        assert hs.info()["lds_bytes_per_wave"] == before
        hs.check()
    pix = grid(w, h)
    for got, kw in ((moved_b, dict(mesh_travels=b_tv)), (both, dict(mesh_travels=b_tv, travels=tv, phase=0.5)),
                    (mesh_only, dict(mesh_travels=b_tv, phase=0.5))):
        exp, _ = MM.restated_image(cam, sc, opts, kw.pop("mesh_travels"), pixels=pix, **kw)
        compare(got, exp, pix)
    exp, _ = NA.restated_image(cam, sc, opts, tv, 0.5, pixels=pix)
    compare(spheres_only, exp, pix)
    assert np.array_equal(bits(first), bits(oracle.render(cam, sc, opts)[0]))


def F_rays():
    rng = np.random.default_rng(8)
    rays = np.zeros((500, 6), f32)  # from around the camera towards the objects
    rays[:, :3] = rng.uniform(-3, 3, (500, 3)) + np.array([0.0, 2.0, 3.0])
    rays[:, 3:] = (np.array([0.0, 1.0, -9.0]) + rng.uniform(-5, 5, (500, 3))) - rays[:, :3]
    return rays


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(hip, oracle):
    cam = scenes.camera(oracle, 16, 8)
    sc = stage(oracle, [standin(oracle, 61, mats()["lambertian"]), standin(oracle, 40, mats()["metal"], at=(-1.5, -0.4, -4.0))])
    opts = abi.default_opts(spp=1, seed=1)
    good = np.array([(0.5, 0.0, 0.0), (0.0, 0.25, 0.0)], f32)

    def refused(word, *a, **kw):
        with pytest.raises(abi.RbrtError) as e:
            hs.set_mesh_motion(*a, **kw)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG and word in str(e.value), str(e.value)

    with hip.HipScene(sc) as hs:
        hs.set_mesh_motion(good)
        kept, _ = render(hs, cam, opts)
        refused("n_meshes", good[:1])
        refused("n_meshes", np.zeros((3, 3), f32))
        refused("n_meshes", good, n_meshes=0)
        refused("reserved", good, reserved=1)
        refused("null travel", good, null_travel=True)
        for v in (float("nan"), float("inf"), -float("inf")):
            bad = good.copy()
            bad[1, 1] = v
            refused("not finite", bad)
        hs.set_motion_phase(7.0)
        refused("(phase + 1) * travel", [(1.0e38, 0.0, 0.0), (0.0, 0.0, 0.0)])  # (8 * 1e38 is not a float32)
        hs.set_motion_phase(0.0)
        hs.set_mesh_motion([(1.0e38, 0.0, 0.0), (0.0, 0.0, 0.0)])
        with pytest.raises(abi.RbrtError) as e:  # ... and the phase makes the same check of the mesh travels
            hs.set_motion_phase(7.0)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG and "mesh 0" in str(e.value)
        hs.set_mesh_motion(good)
        again, _ = render(hs, cam, opts)  # (refused calls left the handle's state as it was)
        assert np.array_equal(bits(again), bits(kept))
        hs.set_mesh_motion(None)
        plain, _ = render(hs, cam, opts)
        assert np.array_equal(bits(plain), bits(oracle.render(cam, sc, opts)[0])) and not np.array_equal(bits(plain), bits(kept))
    with hip.HipScene(abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))) as hs:  # no mesh: nothing to point at, and the draw is still made
        hs.set_mesh_motion(np.zeros((0, 3), f32), null_travel=True)
        a, _ = render(hs, cam, opts)
        hs.set_mesh_motion(None)
        hs.set_shutter((0.0, 0.0, 0.0))
        b, _ = render(hs, cam, opts)
        assert np.array_equal(bits(a), bits(b))
    lib = abi.load_hip()
    assert lib.rbrt_hip_scene_set_mesh_motion(None, C.byref(abi.MeshMotion())) == abi.RBRT_ERR_INVALID_ARG


# ---- the C++ host ----------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
from pathlib import Path  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "motion" / "moving_mesh.yaml"
CLI_W, CLI_H = 32, 24


def _cli(tmp_path, name, *args, env=None):
    out = tmp_path / f"{name}.png"
    r = subprocess.run([str(EXE), "-c", str(CFG), "-t", str(out), "--height", str(CLI_H), "-w", str(CLI_W), *args], capture_output=True, text=True,
                       timeout=300, env=env, cwd=ROOT)  # (the scene names its model relative to the repository's root)
    return r, out


def _host_scene():
    cwd = os.getcwd()
    os.chdir(ROOT)
    try:
        return abi.HostScene(CFG, CLI_H, CLI_W)
    finally:
        os.chdir(cwd)


def _python_image(hip, hs, mesh_travels, spp=4, seed=1, phase=0.0):
    with hip.HipScene(hs) as dev:
        dev.set_mesh_motion(mesh_travels)
        dev.set_motion_phase(phase)
        return render(dev, hs.camera, abi.default_opts(spp=spp, seed=seed))


def test_cli_the_shipped_scene_the_report_and_no_motion(hip, tmp_path):
    hs = _host_scene()
    assert hs.mesh_motion is not None and hs.mesh_motion.any() and hs.motion is None
    _, exp8 = _python_image(hip, hs, hs.mesh_motion)
    _, still8 = _python_image(hip, hs, None)
    assert not np.array_equal(exp8, still8)
    rep = tmp_path / "yaml.json"
    r, out = _cli(tmp_path, "yaml", "-s", "4", "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(TM._png(out), exp8)
    report = json.loads(rep.read_text())
    listed = report["moving_meshes"]
    assert [m["mesh"] for m in listed] == [0] and "moving_spheres" not in report
    assert [float(f32(v)) for v in listed[0]["travel"]] == [float(v) for v in hs.mesh_motion[0]]
    rep = tmp_path / "still.json"
    r, out = _cli(tmp_path, "still", "-s", "4", "--no-motion", "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(TM._png(out), still8) and "moving_meshes" not in json.loads(rep.read_text())


def test_cli_frames_follow_the_mesh_and_write_the_motion_buffer(hip, tmp_path):
    """--frames 3 --motion-step 1 --features: the last frame runs at phase 2, its motion buffer is the library's for that phase
    (w_m times the mesh's coverage), and the report names the step."""
    import torch
    hs = _host_scene()
    rep, feat = tmp_path / "frames.json", tmp_path / "f"
    r, out = _cli(tmp_path, "frames", "-s", "4", "--seed", "3", "--frames", "3", "--motion-step", "1", "--features", str(feat), "--feature-samples", "3",
                  "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    report = json.loads(rep.read_text())
    assert report["motion_step"] == 1.0 and report["frames"] == 3 and [m["mesh"] for m in report["moving_meshes"]] == [0]
    mv_file = Path(str(feat) + ".motion.pfm")
    assert mv_file.exists()
    got = abi.read_pfm(mv_file, any_value=True)
    mv = torch.full((CLI_H, CLI_W, 3), float("nan"), device="cuda")
    with hip.HipScene(hs) as dev:  # (frame k renders with seed + k at the phase k * step: the last one is k = 2)
        dev.set_mesh_motion(hs.mesh_motion)
        dev.set_motion_phase(2.0)
        dev.render_features(hs.camera, abi.default_opts(spp=4, seed=5), 3, d_motion=mv.data_ptr())
        torch.cuda.synchronize()
    m = mv.cpu().numpy()
    assert np.array_equal(bits(got), bits(m))
    assert f32(0.0) < m[..., 0].max() <= f32(1.5) and not m[..., 1:].any()  # (w times the mesh's coverage: the mesh is in view at phase 2)
    r0, _ = _cli(tmp_path, "still_frames", "-s", "4", "--seed", "3", "--frames", "3", "--motion-step", "1", "--no-motion", "--features", str(tmp_path / "g"))
    assert r0.returncode == 0 and not Path(str(tmp_path / "g") + ".motion.pfm").exists()


def test_cli_ranks_passes_and_checkpoints_take_the_mesh_motion(hip, tmp_path):
    r1, out1 = _cli(tmp_path, "g1", "-s", "3", "--gpus", "1")
    r2, out2 = _cli(tmp_path, "g2", "-s", "3", "--gpus", "2", "--oversubscribe")
    assert r1.returncode == 0 and r2.returncode == 0, (r1.stderr[-1000:], r2.stderr[-1000:])
    assert np.array_equal(TM._png(out1), TM._png(out2))
    hs = _host_scene()
    assert np.array_equal(TM._png(out1), _python_image(hip, hs, hs.mesh_motion, spp=3)[1])
    ck = tmp_path / "render.ckpt"
    args = ["-s", "9", "--seed", "3", "--pass-samples", "3", "--checkpoint", str(ck), "--gpus", "2", "--oversubscribe"]
    stop = dict(os.environ, RBRT_TEST_STOP_AFTER_PASS="1")
    r, _ = _cli(tmp_path, "full", "-s", "9", "--seed", "3")
    assert r.returncode == 0
    full8 = TM._png(tmp_path / "full.png")
    r, out = _cli(tmp_path, "a", *args, env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, "a", *args)
    assert r.returncode == 0 and "Resuming from checkpoint" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(TM._png(out), full8)  # (passes of 3 samples on two ranks with the mesh motion are the one render of 9)
    r, _ = _cli(tmp_path, "b", *args, "--no-motion", env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, "b", *args)  # the YAML's mesh motion: the motionless checkpoint is not resumed
    assert r.returncode == 0 and "does not match this render" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(TM._png(out), full8)
