"""Moving spheres (rbrt_hip_scene_set_motion) on the GPU.

Images: bit for bit against the numpy restatement (np_motion.restated_image) for spheres of every material, with a
BasicTriangle between them in the element order, with a pinhole, a lens, a shutter (the shared draw) and an environment; with
a small mesh in front, so that paths alternate between traversals and sphere bounces and every path is parked and resumed,
under the lab knobs that shrink the grid and the shade rounds and with helper launches forced; through every entry point; the
feature buffers against a numpy evaluation of the restated rays at each sample's own t. Exact properties of the handle's
state. The tile pass: no ray of the restatement hits a sphere where its tile's word says it cannot, for hand-picked and fuzzed
cameras and travels, and the image with the table is the image without it. The short-path stage, the object limit and the
C ABI's refusals."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import full_scenes as F
import np_env
import np_features
import np_lens
import np_motion as NM
import np_pattern
import np_reference as R
import np_shutter as NS
import scenes
import test_primary_cull as PC
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

f32 = np.float32
L_, M_, D_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
SKEW = (0.3, -0.2, 0.1)
DEPTH = 8
# the ground stays; the lambertian, the metal, the glass and the emissive sphere each move their own way
TRAVELS = np.array([(0.0, 0.0, 0.0), (0.9, 0.0, 0.0), (-0.4, 0.3, 0.5), (0.0, 0.6, -0.7), (-1.1, -0.2, 0.0)], f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def moving_scene(oracle, triangle=False, mesh=False):
    """The ground and a lambertian, a metal, a glass and an emissive sphere; triangle: a BasicTriangle between them in the
    element order; mesh: a small mesh (13 entries) in front of them."""
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(EM, (3.0, 2.5, 1.5)))]
    assert len(sph) == len(TRAVELS) and {int(s[2].kind) for s in sph} >= {L_, M_, D_, EM}
    kw = {}
    if triangle:
        kw = dict(triangles=[(((-4.0, 0.3, -6.0), (-1.5, 0.4, -6.5), (-2.7, 2.6, -7.0)), abi.material(M_, (0.9, 0.6, 0.3), 0.05))],
                  element_order=[0, 1, scenes.T | 0, 2, 3, 4])
    meshes = [scenes.standin_mesh(oracle, 13, 25.0, (0.5, -0.6, -4.5), (0.0, 0.4, 0.0), abi.material(M_, (0.8, 0.7, 0.6), 0.05))] if mesh else []
    return abi.SceneData(spheres=sph, meshes=meshes, **kw)


def lens_of(cam):
    return np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 40.0, 9.0)


def render(hs, cam, opts, lens=None):
    import torch
    h, w = cam.img_height_pix, cam.img_width_pix
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    hs.render_device(cam, opts, out.data_ptr(), out8.data_ptr(), lens=lens)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out8.cpu().numpy()


# ---- kinds -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pinhole", "triangle_between", "lens", "shutter", "lens_shutter", "environment"])
def test_images_are_bit_identical_to_the_restatement(hip, oracle, case):
    """20 x 12 x 4, depth 8: ragged both ways, 3 x 2 tiles."""
    w, h = 20, 12
    sc = moving_scene(oracle, triangle=case == "triangle_between")
    cam = scenes.camera(oracle, w, h)
    lens = lens_of(cam) if case.startswith("lens") else None
    shutter = SKEW if case.endswith("shutter") else None
    nodes = np_env.noise_map(8, 3) if case == "environment" else None
    opts = abi.default_opts(spp=4, seed=7, max_depth=DEPTH)
    exp, exp8 = NM.restated_image(cam, sc, opts, TRAVELS, lens=lens, shutter=shutter, nodes=nodes)
    with hip.HipScene(sc) as hs:
        if nodes is not None:
            hs.set_environment(nodes)
        hs.set_shutter(shutter)
        hs.set_motion(TRAVELS)
        got, got8 = render(hs, cam, opts, lens)
        hs.check()
        assert hs.last_trace_build() == "general"
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    still, _ = NS.restated_image(cam, sc, opts, lens, shutter if shutter else (0.0, 0.0, 0.0), nodes=nodes)
    assert not np.array_equal(bits(still), bits(exp))  # (the motion does something here)


# ---- t survives parking ----------------------------------------------------------------------------------------------------
PARK_W, PARK_H, PARK_SPP, PARK_SEED = 64, 48, 8, 9  # (384 chunks of work for 256 waves of one per CU: waves take a second chunk into used slots)


@functools.lru_cache(maxsize=None)
def parked_reference():
    """The restated image of the scene with a small mesh in front, made once for every row below (and left unchanged)."""
    from oracle import pyoracle
    sc = moving_scene(pyoracle, mesh=True)
    cam = scenes.camera(pyoracle, PARK_W, PARK_H)
    opts = abi.default_opts(spp=PARK_SPP, seed=PARK_SEED, max_depth=DEPTH)
    exp, _ = NM.restated_image(cam, sc, opts, TRAVELS)
    exp.setflags(write=False)
    return exp


# (test_lab_knobs.py's rows that shrink the grid and the shade rounds, test_all_features_gpu.py's row that forces helpers)
PARK_ROWS = [
    ("default", {}),
    ("shade_2_cont_64_1wave", {"RBRT_SHADE_ROUNDS": "2", "RBRT_SHADE_CONT_MIN": "64", "RBRT_WAVES_PER_CU": "1"}),
    ("shade_64_cont_1_1wave", {"RBRT_SHADE_ROUNDS": "64", "RBRT_SHADE_CONT_MIN": "1", "RBRT_WAVES_PER_CU": "1"}),
    ("y_low_1_1wave", {"RBRT_Y_LOW": "1", "RBRT_WAVES_PER_CU": "1"}),
    ("helpers_2", {"RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": "1", "RBRT_HELPER_MIN_LAUNCH_MI": "0", "RBRT_HELPER_MIN_FREE": "1"}),
]


@pytest.mark.parametrize("rid,env", PARK_ROWS, ids=[r[0] for r in PARK_ROWS])
def test_t_survives_every_park_and_resume(hip, oracle, monkeypatch, rid, env):
    """A small mesh in front of the moving spheres: paths alternate between traversals and sphere bounces, so every path is
    parked in the pool and resumed, with one wave per CU and two shade rounds in slots that are used again and again. Three
    frames issued back to back (helper launches join the later ones), then a render_pass series: all the restated image."""
    import torch
    exp = parked_reference()
    sc = moving_scene(oracle, mesh=True)
    cam = scenes.camera(oracle, PARK_W, PARK_H)
    opts = abi.default_opts(spp=PARK_SPP, seed=PARK_SEED, max_depth=DEPTH)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    outs = [torch.full((PARK_H, PARK_W, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
    with hip.HipScene(sc) as hs:
        hs.set_motion(TRAVELS)
        hs.set_timing(True)
        for o in outs:
            hs.render_device(cam, opts, o.data_ptr())
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert np.array_equal(bits(o.cpu().numpy()), bits(exp)), (rid, k)
        acc = torch.zeros((PARK_H, PARK_W, 3), dtype=torch.float32, device="cuda")
        out = torch.full((PARK_H, PARK_W, 3), float("nan"), dtype=torch.float32, device="cuda")
        for b, e in ((0, 1), (1, 5), (5, PARK_SPP)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == PARK_SPP else None)
        torch.cuda.synchronize()
        assert np.array_equal(bits(out.cpu().numpy()), bits(exp)), (rid, "render_pass")
        hs.check()


# ---- every entry point -----------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_restated_image(hip, oracle):
    """render_device, a render_pass series in uneven pieces, render_adaptive with threshold 0, two and three ranks' packed
    tiles gathered and the counting kernel, on one handle with a motion and a shutter."""
    import torch
    w, h, spp = 20, 12, 5
    cam = scenes.camera(oracle, w, h)
    sc = moving_scene(oracle)
    opts = abi.default_opts(spp=spp, seed=11, max_depth=DEPTH)
    exp, exp8 = NM.restated_image(cam, sc, opts, TRAVELS, shutter=SKEW)

    def img():
        return torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")

    def same(t, what):
        torch.cuda.synchronize()
        assert np.array_equal(bits(t.cpu().numpy()), bits(exp)), what

    with hip.HipScene(sc) as hs:
        hs.set_shutter(SKEW)
        hs.set_motion(TRAVELS)
        got, got8 = render(hs, cam, opts)
        assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8), "render_device"
        acc, out = img(), img()
        for b, e in ((0, 1), (1, 4), (4, spp)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == spp else None)
        same(out, "render_pass 0-1, 1-4, 4-5")
        out = img()
        res = hs.render_adaptive(cam, opts, 0.0, 2, 2, out.data_ptr())
        same(out, "render_adaptive, threshold 0")
        assert res["samples"] == res["samples_fixed"]
        for world in (2, 3):
            slot = hip.packed_pixels(w, h, 0, world)
            slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
            for r in range(world):
                o = abi.default_opts(spp=spp, seed=11, max_depth=DEPTH, tile_rank=r, tile_world=world)
                hs.render_device(cam, o, slots[r * slot * 3:].data_ptr())
            merged = img()
            hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
            same(merged, f"tile_world {world} + unpack")
        out = img()
        hs.render_device(cam, abi.default_opts(spp=spp, seed=11, max_depth=DEPTH, flags=abi.FLAG_COLLECT_STATS), out.data_ptr())
        same(out, "COLLECT_STATS")
        assert hs.stats()["samples"] == w * h * spp
        hs.check()


def np_hits(sc, rays, ts, travels, lo, hi):
    """(obj, dist, g) of np_motion.primary_rays' rays, each against the scene at its own t: np_reference.scene_hit."""
    ns = np_pattern.np_scene(sc)
    P, n = ts.shape
    obj, dist, g = np.full((P, n), -1, np.int64), np.zeros((P, n), f32), np.zeros((P, n, 3), f32)
    for p in range(P):
        for s in range(n):
            hit = R.scene_hit(NM.scene_at(ns, travels, ts[p, s]), rays[p, s, :3], rays[p, s, 3:], f32(lo), f32(hi))
            if hit is not None:
                obj[p, s], dist[p, s], g[p, s] = hit["obj"], hit["dist"], hit["normal"]
    return obj, dist, g


@pytest.mark.parametrize("shutter", [None, SKEW], ids=["motion", "motion_and_shutter"])
def test_feature_buffers_see_the_moved_spheres(hip, oracle, shutter):
    """Depth, normal, albedo and coverage of every sample's sphere where its own t puts it (a BasicTriangle between them)."""
    import torch
    w, h, n = 20, 12, 3
    cam = scenes.camera(oracle, w, h)
    sc = moving_scene(oracle, triangle=True)
    opts = abi.default_opts(spp=2, seed=5)
    rays, ts = NM.primary_rays(cam, 5, n, shutter=shutter)
    obj, dist, g = np_hits(sc, rays, ts, TRAVELS, opts.min_dist, opts.max_dist)
    exp = np_features.scatter_pixels(np_features.from_hits(sc, obj, dist, g, n), np_features.all_pixels(cam), h, w)
    bufs = dict(albedo=torch.full((h, w, 3), float("nan"), device="cuda"), normal=torch.full((h, w, 3), float("nan"), device="cuda"),
                depth=torch.full((h, w), float("nan"), device="cuda"), coverage=torch.full((h, w), float("nan"), device="cuda"),
                object=torch.full((h, w), -7, dtype=torch.int32, device="cuda"))
    with hip.HipScene(sc) as hs:
        hs.set_shutter(shutter)
        hs.set_motion(TRAVELS)
        hs.render_features(cam, opts, n, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        hs.check()
    for k in ("albedo", "normal", "depth", "coverage"):
        assert np.array_equal(bits(bufs[k].cpu().numpy()), bits(getattr(exp, k))), k
    assert np.array_equal(bufs["object"].cpu().numpy(), exp.object)
    o0, d0, g0 = np_hits(sc, rays, ts, np.zeros_like(TRAVELS), opts.min_dist, opts.max_dist)
    assert not np.array_equal(bits(d0), bits(dist))  # (the motion does something here)


# ---- exact properties ------------------------------------------------------------------------------------------------------
def test_the_handles_state(hip, oracle):
    """An all-zero motion is a zero-travel shutter, bit for bit; set_motion(NULL) restores the original bits; trace_rays sees
    the spheres at the opening with and without a motion; a plain scene runs the general build with a motion and the plain
    one again without; a motionless launch keeps its LDS bytes."""
    w, h = 32, 24
    cam = scenes.camera(oracle, w, h)
    sc = scenes.example_scene(oracle, 603)  # spheres and ONE mesh: a plain scene
    n_sph = len(sc.spheres)
    opts = abi.default_opts(spp=3, seed=4, max_depth=DEPTH)
    rng = np.random.default_rng(8)
    rays = np.zeros((500, 6), f32)  # from around the camera towards the objects
    rays[:, :3] = rng.uniform(-3, 3, (500, 3)) + np.array([0.0, 2.0, 3.0])
    rays[:, 3:] = (np.array([0.0, 1.0, -9.0]) + rng.uniform(-5, 5, (500, 3))) - rays[:, :3]
    tv = rng.uniform(-1, 1, (n_sph, 3)).astype(f32)
    with hip.HipScene(sc) as hs:
        before = hs.info()["lds_bytes_per_wave"]
        first, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "plain"
        traced = hs.trace_rays(rays)
        hs.set_shutter((0.0, 0.0, 0.0))
        zero_shutter, _ = render(hs, cam, opts)
        hs.set_shutter(None)
        hs.set_motion(np.zeros((n_sph, 3), f32))
        zero_motion, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "general"
        assert np.array_equal(bits(zero_motion), bits(zero_shutter)) and not np.array_equal(bits(zero_motion), bits(first))
        hs.set_motion(tv)
        moved, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "general" and not np.array_equal(bits(moved), bits(zero_motion))
        with_motion = hs.trace_rays(rays)
        for a, b in zip(traced, with_motion):
            assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
        hs.set_motion(None)
        again, _ = render(hs, cam, opts)
        assert hs.last_trace_build() == "plain"
        assert np.array_equal(bits(again), bits(first))
        assert hs.info()["lds_bytes_per_wave"] == before
        hs.check()
    assert np.array_equal(bits(first), bits(oracle.render(cam, sc, opts)[0]))


# ---- the tile pass ---------------------------------------------------------------------------------------------------------
def sphere_hits(rays, centres, radius, lo, hi):
    """np_reference.sphere_hit for a batch, float32 operation for operation: rays (N, 6), centres (N, 3) -> bool (N,)."""
    o, d = rays[:, :3].astype(f32), rays[:, 3:].astype(f32)
    dot = lambda a, b: ((a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]).astype(f32) + a[:, 2] * b[:, 2]).astype(f32)  # noqa: E731
    with np.errstate(all="ignore"):
        a = dot(d, d)
        l = (o - centres.astype(f32)).astype(f32)
        b = dot((d * f32(2.0)).astype(f32), l)
        c = (dot(l, l) - f32(radius) * f32(radius)).astype(f32)
        sol = (b * b - (f32(4.0) * a) * c).astype(f32)
        root = np.sqrt(sol).astype(f32)
        t1, t2 = ((-b - root) / (f32(2.0) * a)).astype(f32), ((-b + root) / (f32(2.0) * a)).astype(f32)
        second = (sol > 0) & (t1 < 0)
        t = np.where(second, t2, t1).astype(f32)
        ok = (sol >= 0) & ~(second & (t2 < 0))
        p = (o + (t[:, None] * d).astype(f32)).astype(f32)
        q = (o - p).astype(f32)
        dist = np.sqrt(dot(q, q)).astype(f32)
        return ok & ~(dist < f32(lo)) & ~(dist > f32(hi))


def check_motion_table(hip, oracle, monkeypatch, cam, sc, travels, shutter=None, n=3, seed=3):
    """No ray of np_motion.primary_rays hits sphere e, where its own t puts it, in a tile whose word has bit e; and the image
    with the table is the image without it (RBRT_PRIMARY_CULL=0, as test_shutter_gpu.py switches it off). Returns the table."""
    w, h = cam.img_width_pix, cam.img_height_pix
    travels = NM.travels_of(travels)
    opts = abi.default_opts(spp=n, seed=seed, max_depth=DEPTH)
    rays, ts = NM.primary_rays(cam, seed, n, shutter=shutter)
    flat, tf = rays.reshape(-1, 6), ts.reshape(-1)
    images = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("RBRT_PRIMARY_CULL", cull)
        with hip.HipScene(sc) as hs:
            hs.set_shutter(shutter)
            hs.set_motion(travels)
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
        assert F.same_bits(images["1"], images["0"])
    pix = np_features.all_pixels(cam)
    tile_of = np.repeat(np.array([(r // 8) * table.shape[1] + (c // 8) for r, c in pix]), n)
    words = table.reshape(-1)[tile_of]
    for e, (c, r, _) in enumerate(sc.spheres[:24]):
        centres = (np.asarray(c, f32)[None, :] + (tf[:, None] * travels[e][None, :]).astype(f32)).astype(f32)
        bad = sphere_hits(flat, centres, r, opts.min_dist, opts.max_dist) & (((words >> e) & 1) != 0)
        assert not bad.any(), f"sphere {e}: culled in tiles {sorted(set(tile_of[bad].tolist()))[:5]} where a ray of the restatement hits it"
    return table


def axis_camera(oracle, w=64, h=48, **kw):
    return scenes.camera(oracle, w, h, **dict(dict(position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), focal_mm=50.0), **kw))


def pair(static_c, moving_c, r=0.5):
    """Sphere 0 stays, sphere 1 moves."""
    return abi.SceneData(spheres=[(static_c, r, abi.material(L_, (0.7, 0.4, 0.3))), (moving_c, r, abi.material(M_, (0.8, 0.8, 0.8), 0.1))])


# (name, the moving sphere's centre at the opening, its travel): the camera at the origin looks down -z, 40 degrees wide
HAND_PICKED = [
    ("sweeps_in_from_outside", (-8.0, 0.0, -10.0), (5.0, 0.0, 0.0)),
    ("along_the_view_axis", (0.0, 0.0, -30.0), (0.0, 0.0, 25.0)),
    ("past_the_camera", (0.3, 0.0, -6.0), (0.0, 0.0, 12.0)),
    ("behind_the_camera", (6.0, 1.0, 12.0), (-4.0, 0.0, 3.0)),
    ("longer_than_the_distance", (-1.0, 0.5, -4.0), (3.0, -2.0, 40.0)),
]


@pytest.mark.parametrize("name,centre,travel", HAND_PICKED, ids=[c[0] for c in HAND_PICKED])
def test_no_ray_hits_a_moving_sphere_its_tile_culled(hip, oracle, monkeypatch, name, centre, travel):
    cam = axis_camera(oracle)
    sc = pair((3.0, 0.0, -10.0), centre)
    table = check_motion_table(hip, oracle, monkeypatch, cam, sc, [(0.0, 0.0, 0.0), travel])
    s_bit, m_bit = (table & 1) != 0, (table & 2) != 0
    print(f"{name}: static culled in {int(s_bit.sum())}, moving culled in {int(m_bit.sum())} of {table.size} tiles")
    assert s_bit.any() and not s_bit.all()  # (the static sphere is seen somewhere and nowhere else)
    if name == "sweeps_in_from_outside":
        # it ends at x = -3: the left tiles of the middle rows see it and not the static one; the right half never sees it
        assert (s_bit & ~m_bit).any() and m_bit[:, table.shape[1] // 2:].all()
    if name == "behind_the_camera":
        assert m_bit.any()  # (its ball of positions lies behind the image: the tiles whose lines miss it backwards cull it)
    if name in ("past_the_camera", "longer_than_the_distance"):
        assert not m_bit.all()


def test_a_shutter_and_a_motion_share_the_table(hip, oracle, monkeypatch):
    cam = axis_camera(oracle)
    sc = pair((3.0, 0.0, -10.0), (-8.0, 0.0, -10.0))
    table = check_motion_table(hip, oracle, monkeypatch, cam, sc, [(0.0, 0.0, 0.0), (5.0, 0.0, 0.0)], shutter=(0.5, 0.0, 0.0))
    assert ((table & 1) != 0).any() and ((table & 2) != 0).any() and (((table & 1) != 0) & ((table & 2) == 0)).any()


@pytest.mark.parametrize("k", range(24))
def test_fuzzed_cameras_and_travels(hip, oracle, monkeypatch, k):
    """The random scenes and cameras of test_primary_cull; every sphere a travel log-uniform from 1e-4 to 100 units in a random
    direction (one in four stays), every third case with a shutter."""
    rng = np.random.default_rng(91000 + k)
    sc = PC.fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 49)), int(rng.integers(9, 33))
    cam = PC.fuzz_camera(oracle, rng, sc, w, h)
    travels = np.array([PC._log_uniform(rng, 1e-4, 100.0) * PC._unit(rng) * (rng.random() >= 0.25) for _ in sc.spheres], f32).reshape(-1, 3)
    shutter = tuple(float(f32(v)) for v in PC._log_uniform(rng, 1e-3, 10.0) * PC._unit(rng)) if k % 3 == 0 else None
    table = check_motion_table(hip, oracle, monkeypatch, cam, sc, travels, shutter=shutter, n=2, seed=k)
    print(f"fuzz {k}: {w}x{h}, {len(sc.spheres)} spheres, {len(sc.meshes)} meshes: {int(np.count_nonzero(table))} tiles with bits")


# ---- the short-path stage --------------------------------------------------------------------------------------------------
def test_the_short_path_stage_with_a_moving_sphere(hip, oracle):
    """No mesh anywhere: every tile that is not background only is the stage's. Stage off, forced, and numpy."""
    w, h = 32, 24
    cam = scenes.camera(oracle, w, h)
    sc = moving_scene(oracle)
    opts = abi.default_opts(spp=4, seed=7, max_depth=DEPTH)
    exp, _ = NM.restated_image(cam, sc, opts, TRAVELS)
    got = {}
    for mode in (0, 2):
        with hip.HipScene(sc) as hs:
            hs.set_motion(TRAVELS)
            hs.set_short_paths(mode)
            got[mode], _ = render(hs, cam, opts)
            if mode == 2:
                masks = hs.short_masks()
                assert masks.any()  # (the stage finished samples of this launch)
                print(f"short-path stage: {int(sum(bin(int(m)).count('1') for m in masks))} of {w * h * opts.spp} samples finished")
            hs.check()
    assert np.array_equal(bits(got[0]), bits(got[2]))
    assert np.array_equal(bits(got[2]), bits(exp))


# ---- limits and refusals ---------------------------------------------------------------------------------------------------
def test_255_spheres_all_moving(hip, oracle):
    """full_scenes' scene at the object limit, every sphere with a travel of its own (the ground's a small one): 765 more
    words of LDS for the launch. Forty pixels against the restatement, the whole image finite."""
    w, h = 24, 16
    sc = F.limit_scene(oracle, "spheres")
    assert len(sc.spheres) == F.N_MAX
    tv = np.random.default_rng(12).uniform(-0.5, 0.5, (F.N_MAX, 3)).astype(f32)
    tv[0] *= f32(0.01)
    cam = scenes.camera(oracle, w, h)
    opts = abi.default_opts(spp=2, seed=3, max_depth=4)
    rng = np.random.default_rng(1)
    pix = sorted({(int(r), int(c)) for r, c in zip(rng.integers(0, h, 40), rng.integers(0, w, 40))})
    exp, _ = NM.restated_image(cam, sc, opts, tv, pixels=pix)
    with hip.HipScene(sc) as hs:
        hs.set_motion(tv)
        got, _ = render(hs, cam, opts)
        hs.check()
    assert np.isfinite(got).all()
    for r, c in pix:
        assert np.array_equal(bits(got[r, c]), bits(exp[r, c])), (r, c)


def test_refusals_through_the_c_abi(hip, oracle):
    lib = abi.load_hip()
    mo = abi.Motion()
    assert lib.rbrt_hip_scene_set_motion(None, C.byref(mo)) == abi.RBRT_ERR_INVALID_ARG
    assert lib.rbrt_hip_scene_set_motion(None, None) == abi.RBRT_ERR_INVALID_ARG
    cam = scenes.camera(oracle, 16, 8)
    sc = abi.SceneData(spheres=[((0.0, -1000.0, -5.0), 1000.0, abi.material(L_, (0.5, 0.5, 0.5))),
                                ((2.0, 1.0, -8.0), 1.0, abi.material(L_, (0.5, 0.5, 0.5))), ((0.0, 1.0, -8.0), 1.0, abi.material(M_, (0.8, 0.8, 0.8), 0.1))])
    opts = abi.default_opts(spp=1, seed=1)
    good = np.array([(0.0, 0.0, 0.0), (0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], f32)

    def refused(word, *a, **kw):
        with pytest.raises(abi.RbrtError) as e:
            hs.set_motion(*a, **kw)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG and word in str(e.value), str(e.value)

    with hip.HipScene(sc) as hs:
        hs.set_motion(good)
        kept, _ = render(hs, cam, opts)
        refused("n_spheres", good[:2])
        refused("n_spheres", np.zeros((4, 3), f32))
        refused("n_spheres", good, n_spheres=0)
        refused("reserved", good, reserved=1)
        refused("null travel", good, null_travel=True)
        for v in (float("nan"), float("inf"), -float("inf")):
            bad = good.copy()
            bad[2, 1] = v
            refused("not finite", bad)
        again, _ = render(hs, cam, opts)  # (a refused call leaves the handle's motion as it was)
        assert np.array_equal(bits(again), bits(kept))
        hs.set_motion(None)
        plain, _ = render(hs, cam, opts)
        assert np.array_equal(bits(plain), bits(oracle.render(cam, sc, opts)[0])) and not np.array_equal(bits(plain), bits(kept))
    far = abi.SceneData(spheres=[((3.0e38, 1.0, -8.0), 1.0, abi.material(L_, (0.5, 0.5, 0.5)))])
    with hip.HipScene(far) as hs:  # (never rendered: the sum 3e38 + 1e38 is not a float32, 3e38 - 1e38 is)
        refused("center + travel", [(1.0e38, 0.0, 0.0)])
        hs.set_motion([(-1.0e38, 0.0, 0.0)])
    with hip.HipScene(abi.SceneData(spheres=[], meshes=[scenes.standin_mesh(oracle, 61, 30.0, (0.0, 0.0, -8.0), (0.0, 0.0, 0.0), abi.material(L_, (0.5, 0.5, 0.5)))])) as hs:
        hs.set_motion(np.zeros((0, 3), f32), null_travel=True)  # (no sphere: nothing to point at, and the draw is still made)
        a, _ = render(hs, cam, opts)
        hs.set_motion(None)
        hs.set_shutter((0.0, 0.0, 0.0))
        b, _ = render(hs, cam, opts)
        assert np.array_equal(bits(a), bits(b))


# ---- the C++ host ----------------------------------------------------------------------------------------------------------
import json  # noqa: E402
import os  # noqa: E402
import subprocess  # noqa: E402
from pathlib import Path  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "motion" / "moving_spheres.yaml"
W, H = 32, 24


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _cli(tmp_path, name, *args, env=None):
    out = tmp_path / f"{name}.png"
    r = subprocess.run([str(EXE), "-c", str(CFG), "-t", str(out), "--height", str(H), "-w", str(W), *args], capture_output=True, text=True,
                       timeout=300, env=env)
    return r, out


def _python_image(hip, hs, travels, spp=4, seed=1, shutter=None):
    with hip.HipScene(hs) as dev:
        dev.set_shutter(shutter)
        dev.set_motion(travels)
        return render(dev, hs.camera, abi.default_opts(spp=spp, seed=seed))


def test_cli_yaml_keys_the_report_and_no_motion(hip, tmp_path):
    hs = abi.HostScene(CFG, H, W)
    assert hs.motion is not None and hs.motion.any()
    _, exp8 = _python_image(hip, hs, hs.motion)
    _, still8 = _python_image(hip, hs, None)
    assert not np.array_equal(exp8, still8)
    rep = tmp_path / "yaml.json"
    r, out = _cli(tmp_path, "yaml", "-s", "4", "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), exp8)
    listed = json.loads(rep.read_text())["moving_spheres"]
    assert [m["sphere"] for m in listed] == [2, 4, 5]
    for m in listed:  # (%.9g: it reads back as the float32 it was)
        assert [float(f32(v)) for v in m["travel"]] == [float(v) for v in hs.motion[m["sphere"]]]
    rep = tmp_path / "still.json"
    r, out = _cli(tmp_path, "still", "-s", "4", "--no-motion", "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), still8) and "moving_spheres" not in json.loads(rep.read_text())
    # a shutter from the command line shares the exposure with the keys
    _, both8 = _python_image(hip, hs, hs.motion, shutter=SKEW)
    r, out = _cli(tmp_path, "both", "-s", "4", "--shutter-travel", "0.3,-0.2,0.1")
    assert r.returncode == 0 and np.array_equal(_png(out), both8)


def test_cli_ranks_passes_and_checkpoints_take_the_motion(hip, tmp_path):
    r1, out1 = _cli(tmp_path, "g1", "-s", "3", "--gpus", "1")
    r3, out3 = _cli(tmp_path, "g3", "-s", "3", "--gpus", "3", "--oversubscribe")
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr[-1000:], r3.stderr[-1000:])
    assert np.array_equal(_png(out1), _png(out3))
    hs = abi.HostScene(CFG, H, W)
    assert np.array_equal(_png(out1), _python_image(hip, hs, hs.motion, spp=3)[1])
    ck = tmp_path / "render.ckpt"
    args = ["-s", "9", "--seed", "3", "--pass-samples", "3", "--checkpoint", str(ck)]
    stop = dict(os.environ, RBRT_TEST_STOP_AFTER_PASS="1")
    r, _ = _cli(tmp_path, "full", "-s", "9", "--seed", "3")
    assert r.returncode == 0
    full8 = _png(tmp_path / "full.png")
    r, out = _cli(tmp_path, "a", *args, env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, "a", *args)
    assert r.returncode == 0 and "Resuming from checkpoint" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(_png(out), full8)  # (passes of 3 samples with the motion are the one render of 9)
    r, _ = _cli(tmp_path, "b", *args, "--no-motion", env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, "b", *args)  # the YAML's motion: the motionless checkpoint is not resumed
    assert r.returncode == 0 and "does not match this render" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(_png(out), full8)
