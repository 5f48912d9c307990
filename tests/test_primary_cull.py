"""The tile pass (kernels.hip primary_cull_kernel, tile_lists_kernel, sky_resolve_kernel; DESIGN.md "The tile pass").

The library decides per 8x8 tile which sphere tests (sphere.rs:20-66) and mesh box tests (aabbox.rs:28-58) the tile's
camera rays (cam.rs:64-82) would fail; a tile whose rays fail all of them sees the background only, and its pixels
are finished by a streaming kernel instead of the trace kernel. A wrong bit changes the image, so the table is checked
on its own, ahead of the image tests: every set bit is a promise "no camera ray of this tile passes this test", and the
oracle's routines are run over the tile's rays -- all four corners of the jitter square, its middle, random jitter -- to
look for a counter-example. Cameras: the example scene's, one looking up (sky tiles: the ground sphere is BEHIND their
rays, where sphere.rs accepts a grazing line), straight down, from inside the ground sphere, from its surface, from far
away with a long lens, with mirrored pixel pitch, and a degenerate one (nothing may be culled with it).
"""
import zlib

import numpy as np
import pytest

import scenes
from np_reference import bbox_gate  # noqa: F401  (test_thin_lens reads it from here)
from rbrt_amd import abi

pytestmark = pytest.mark.gpu
f32 = np.float32
U_MAX = f32(1.0) - f32(2.0 ** -24)  # the largest value of rand's Standard f32 (np_reference.Rng.next_f32)


def _v(a):
    return np.array(list(a), f32)


def camera_rays(cam, u0, u1):
    """cam.rs:64-82 for every pixel at once, float32 operation for operation (np_reference.camera_ray): (H*W, 6)."""
    W, H = cam.img_width_pix, cam.img_height_pix
    col = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
    row = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
    col_off = col - f32(W // 2)
    row_off = row - f32(H // 2)
    col_mm = ((col_off + u0).astype(f32) - f32(0.5)) * f32(cam.mm_per_pix_hor)
    row_mm = ((row_off + u1).astype(f32) - f32(0.5)) * f32(cam.mm_per_pix_vert)
    right, up, ctr, pos = _v(cam.right), _v(cam.up), _v(cam.img_center_point), _v(cam.position)
    target = (ctr + (f32(0.001) * col_mm)[..., None] * right) - (f32(0.001) * row_mm)[..., None] * up
    d = (target - pos).astype(f32)
    with np.errstate(all="ignore"):
        ln = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32))
        d = (d / ln[..., None]).astype(f32)
    o = np.broadcast_to(pos, d.shape)
    return np.concatenate([o, d], -1).reshape(-1, 6).astype(f32)


def tiles_of(mask, W, H):
    """(H*W,) bool per pixel -> (tiles_y, tiles_x) bool: any pixel of the tile."""
    ty, tx = (H + 7) // 8, (W + 7) // 8
    m = np.zeros((ty * 8, tx * 8), bool)
    m[:H, :W] = mask.reshape(H, W)
    return m.reshape(ty, 8, tx, 8).any(axis=(1, 3))


def jitters(rng, W, H):
    z, m = np.zeros((H, W), f32), np.full((H, W), U_MAX, f32)
    yield z, z
    yield m, m
    yield z, m
    yield m, z
    yield np.full((H, W), f32(0.5)), np.full((H, W), f32(0.5))
    for _ in range(3):
        yield ((rng.integers(0, 1 << 24, (H, W)).astype(f32) * f32(2.0 ** -24)),
               (rng.integers(0, 1 << 24, (H, W)).astype(f32) * f32(2.0 ** -24)))


def check_table(hip, oracle, cam, sc, rng, max_dist=2000.0, full_scene_jitters=8, min_dist=0.001):
    """Looks for a ray that passes a test its tile's word rules out, in the table of a render with the distance window
    (min_dist, max_dist): the pass grows the tree boxes it tests by a pad that holds 1 / min_dist. Returns the table."""
    W, H = cam.img_width_pix, cam.img_height_pix
    with hip.HipScene(sc) as hs:
        table = hs.primary_cull(cam, abi.default_opts(min_dist=min_dist, max_dist=max_dist))
    n_el = len(sc.spheres)
    reach = [np.zeros(table.shape, bool) for _ in range(n_el + len(sc.meshes))]
    anything = np.zeros(table.shape, bool)
    for n, (u0, u1) in enumerate(jitters(rng, W, H)):
        rays = camera_rays(cam, u0, u1)
        if n < full_scene_jitters:  # Scene::hit itself (all triangles, brute force): what a "background only" tile promises
            _, obj, _, _ = oracle.trace_rays(sc, rays, min_dist, max_dist)
            anything |= tiles_of(obj >= 0, W, H)
        for e, sp in enumerate(sc.spheres):
            _, obj, _, _ = oracle.trace_rays(abi.SceneData(spheres=[sp]), rays, min_dist, max_dist)
            reach[e] |= tiles_of(obj >= 0, W, H)
        for m, md in enumerate(sc.meshes):
            reach[n_el + m] |= tiles_of(bbox_gate(md.bbox_lo.astype(f32), md.bbox_hi.astype(f32), rays), W, H)
    for e in range(min(n_el, 24)):
        bad = reach[e] & (((table >> e) & 1) != 0)
        assert not bad.any(), f"sphere {e}: culled in tiles {np.argwhere(bad)[:5].tolist()} that a camera ray hits it from"
    for m in range(min(len(sc.meshes), 7)):
        bad = reach[n_el + m] & (((table >> (24 + m)) & 1) != 0)
        assert not bad.any(), f"mesh {m}: box culled in tiles {np.argwhere(bad)[:5].tolist()} that a camera ray enters it from"
    # bit 31: every sphere out of reach, and every mesh -- by its box, or by the boxes of the top of its tree
    elements = np.uint32((1 << n_el) - 1)
    every = np.uint32(int(elements) | (((1 << len(sc.meshes)) - 1) << 24))
    sky = (table >> 31) != 0
    if n_el <= 24 and len(sc.meshes) <= 7:
        assert not (sky & ((table & elements) != elements)).any()
        assert not (~sky & ((table & every) == every)).any()
    else:
        assert not sky.any()
    bad = sky & anything
    assert not bad.any(), f"background-only tiles {np.argwhere(bad)[:5].tolist()} have a camera ray that hits something"
    return table, reach


CAMERAS = {
    "example": {},
    "looking_up": dict(look_at=(0.0, 0.6, -1.0), up=(0.0, 1.0, 0.0)),
    "straight_down": dict(look_at=(0.0, -1.0, -0.001), up=(0.0, 0.0, -1.0)),
    "inside_the_ground": dict(position=(0.0, -5.0, 4.0)),
    "on_the_ground": dict(position=(0.0, 0.0, -5.0), look_at=(0.3, 0.2, -1.0), up=(0.0, 1.0, 0.0)),
    "far_long_lens": dict(position=(300.0, 900.0, 2500.0), look_at=(-0.115, -0.34, -0.93), up=(0.0, 1.0, 0.0), focal_mm=900.0),
    "wide": dict(focal_mm=6.0),
    "sideways": dict(position=(-30.0, 2.0, -12.0), look_at=(1.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), focal_mm=50.0),
}


@pytest.mark.parametrize("name", list(CAMERAS))
def test_no_camera_ray_passes_a_culled_test(hip, oracle, name):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    cam = scenes.camera(oracle, 200, 136, **CAMERAS[name])
    sc = scenes.example_scene(oracle, 1203)
    table, reach = check_table(hip, oracle, cam, sc, rng)
    if name in ("example", "looking_up", "sideways"):
        assert (table >> 31).any()            # there is sky, and it is found
    if name == "inside_the_ground":
        assert not ((table >> 0) & 1).any()   # every ray hits the sphere the camera is in


def test_the_rule_is_worth_having_on_the_bench_frame(hip, oracle):
    """Config 2's camera at full size: how much the table removes (a regression here is a performance bug, not a wrong
    image): 37 % of the tiles see sky only (40 % do in truth), and the camera rays keep less than one sphere test of four."""
    rng = np.random.default_rng(5)
    cam = scenes.camera(oracle, 1024, 768)
    sc = scenes.example_scene(oracle, 3000)
    table, reach = check_table(hip, oracle, cam, sc, rng, full_scene_jitters=3)
    sky = np.count_nonzero(table >> 31) / table.size
    left = sum(np.count_nonzero(((table >> e) & 1) == 0) for e in range(4)) / table.size
    exact = sum(np.count_nonzero(r) for r in reach[:4]) / table.size
    assert sky > 0.36 and left < 1.0, (sky, left)
    assert left < exact + 0.25, (left, exact)  # within a quarter of a test per tile of what the sampled rays reach


def test_mirrored_pitch_two_meshes_many_spheres_and_degenerate_cameras(hip, oracle):
    rng = np.random.default_rng(11)
    sc = scenes.example_scene(oracle, 1203)
    second = scenes.standin_mesh(oracle, 603, 30.0, (-9.0, 0.5, -14.0), (0.0, 0.4, 0.0), abi.material(abi.MAT_METAL, (0.7, 0.7, 0.7), 0.1))
    extra = [((float(x), 0.4, float(z)), 0.4, abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5))) for x in range(-12, 13, 4) for z in (-6, -11, -17, -25)]
    sc2 = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES) + extra, meshes=[sc.meshes[0], second])  # 32 spheres: 8 beyond the mask
    cam = scenes.camera(oracle, 136, 100)
    check_table(hip, oracle, cam, sc2, rng)
    cam.mm_per_pix_hor = -cam.mm_per_pix_hor  # mirrored image: the intervals' ends swap
    check_table(hip, oracle, cam, sc2, rng)
    cam.mm_per_pix_vert = -cam.mm_per_pix_vert
    check_table(hip, oracle, cam, sc, rng)
    # degenerate: right parallel to up (no image plane), a zero pitch, a NaN position -> nothing may be culled
    for breaker in ("parallel", "zero_pitch", "nan"):
        cam = scenes.camera(oracle, 64, 48)
        if breaker == "parallel":
            cam.right[0], cam.right[1], cam.right[2] = cam.up[0], cam.up[1], cam.up[2]
        elif breaker == "zero_pitch":
            cam.mm_per_pix_hor = 0.0
            cam.mm_per_pix_vert = 0.0
        else:
            cam.position[1] = float("nan")
        with hip.HipScene(sc) as hs:
            table = hs.primary_cull(cam)
        if breaker == "zero_pitch":   # every ray is the central one: culling is legitimate, and must still be right
            check_table(hip, oracle, cam, sc, rng)
        else:
            assert not table.any(), breaker


def test_images_with_and_without_sky_tiles_equal_the_oracle(hip, oracle):
    """Whole images through the culled path against the oracle, bit for bit, for the cameras above that differ most from
    the example's (the parity suite renders the example camera everywhere), with the sample and ray counts."""
    import torch
    sc = scenes.example_scene(oracle, 1203)
    for name in ("looking_up", "straight_down", "inside_the_ground", "on_the_ground", "sideways"):
        cam = scenes.camera(oracle, 136, 100, **CAMERAS[name])
        exp, _, rays = oracle.render(cam, sc, abi.default_opts(spp=5, seed=9))
        out = torch.empty((100, 136, 3), dtype=torch.float32, device="cuda")
        with hip.HipScene(sc) as hs:
            hs.render_device(cam, abi.default_opts(spp=5, seed=9, flags=abi.FLAG_COLLECT_STATS), out.data_ptr())
            st = hs.stats()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)), name
            assert st["samples"] == 136 * 100 * 5 and st["rays"] == rays, name
            hs.render_device(cam, abi.default_opts(spp=5, seed=9), out.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32)), name


def test_cameras_change_inside_a_stream_of_frames_into_one_buffer(hip, oracle):
    """The tile lists belong to a pipeline lane and are kept while its camera stays the same. Frames with two cameras
    whose background-only tiles differ, issued back to back without synchronisation (three lanes in flight), each
    written into ONE output buffer and copied out on the same stream: every frame is its camera's image. A list made
    for the other camera, or a write that overtakes the previous frame's, would show."""
    import torch
    sc = scenes.example_scene(oracle, 1203)
    cams = [scenes.camera(oracle, 136, 100), scenes.camera(oracle, 136, 100, **CAMERAS["looking_up"]),
            scenes.camera(oracle, 136, 100, **CAMERAS["sideways"])]
    order = [0, 1, 1, 0, 2, 0, 0, 1, 2, 2, 0, 1]
    exp = [oracle.render(c, sc, abi.default_opts(spp=3, seed=4))[0] for c in cams]
    out = torch.empty((100, 136, 3), dtype=torch.float32, device="cuda")
    copies = []
    with hip.HipScene(sc) as hs:
        for k in order:
            hs.render_device(cams[k], abi.default_opts(spp=3, seed=4), out.data_ptr(), None, None)
            copies.append(out.clone())  # (same stream: ordered behind the frame, ahead of the next one)
        torch.cuda.synchronize()
        hs.check()
    for n, (k, img) in enumerate(zip(order, copies)):
        assert np.array_equal(img.cpu().numpy().view(np.uint32), exp[k].view(np.uint32)), (n, k)


def test_ranks_and_passes_with_background_tiles(hip, oracle):
    """Three ranks' packed tiles, rendered in two passes each (running sums through rbrt_hip_render_pass), on a ragged
    image whose upper half is sky: the background-only tiles take the streaming kernel in both passes, the others the
    trace kernel; merged, the image is the oracle's."""
    import torch
    from rbrt_amd import tiles
    W, H, spp = 100, 76, 5
    cam = scenes.camera(oracle, W, H, **CAMERAS["looking_up"])
    sc = scenes.example_scene(oracle, 1203)
    exp, _, _ = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=2))
    parts = []
    with hip.HipScene(sc) as hs:
        for rank in range(3):
            n = hip.packed_pixels(W, H, rank, 3)
            acc = torch.zeros(n * 3, dtype=torch.float32, device="cuda")
            out = torch.full((n * 3,), float("nan"), dtype=torch.float32, device="cuda")
            o = abi.default_opts(spp=spp, seed=2, tile_rank=rank, tile_world=3)
            hs.render_pass(cam, o, 0, 2, acc.data_ptr(), out.data_ptr())
            hs.render_pass(cam, o, 2, spp, acc.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            parts.append(out.cpu().numpy().reshape(-1, 3))
        hs.check()
    got = tiles.unpack(parts, W, H)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))


def test_tile_pass_switched_off_gives_the_same_image(hip, oracle, monkeypatch):
    import torch
    cam = scenes.camera(oracle, 136, 100)
    sc = scenes.example_scene(oracle, 1203)
    exp, _, rays = oracle.render(cam, sc, abi.default_opts(spp=4, seed=3))
    out = torch.empty((100, 136, 3), dtype=torch.float32, device="cuda")
    monkeypatch.setenv("RBRT_PRIMARY_CULL", "0")
    with hip.HipScene(sc) as hs:
        hs.render_device(cam, abi.default_opts(spp=4, seed=3, flags=abi.FLAG_COLLECT_STATS), out.data_ptr())
        assert hs.stats()["rays"] == rays
        assert np.array_equal(out.cpu().numpy().view(np.uint32), exp.view(np.uint32))


# ---- fuzz: random cameras over random scenes (round-3 review: the table's promises were checked on 8 + 3 hand-picked cameras) ----
N_FUZZ = int(__import__("os").environ.get("RBRT_FUZZ_CAMERAS", "60"))


def _log_uniform(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def fuzz_scene(oracle, rng):
    """0-8 spheres with radii from 0.01 to 1000 (log-uniform; a ground sphere in two scenes of three), 0-3 small meshes."""
    kinds = [abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC]

    def rand_mat():
        k = kinds[int(rng.integers(3))]
        return abi.material(k, tuple(rng.uniform(0.05, 0.95, 3)), float(rng.uniform(0.0, 0.6) if k == abi.MAT_METAL else rng.uniform(0.3, 2.2)))
    spheres = [((0.0, -1000.0, -5.0), 1000.0, rand_mat())] if rng.random() < 0.67 else []
    for _ in range(int(rng.integers(0, 9))):
        r = _log_uniform(rng, 0.01, 1000.0) if rng.random() < 0.4 else float(rng.uniform(0.2, 3.0))
        c = rng.uniform(-8, 8, 3) + np.array([0.0, 2.0, -10.0]) + _unit(rng) * (r if r > 20.0 else 0.0)  # (a huge one is pushed away)
        spheres.append((tuple(float(x) for x in c), r, rand_mat()))
    meshes = []
    for _ in range(int(rng.integers(0, 4))):
        n = int(rng.integers(8, 500))
        if rng.random() < 0.5:
            tri = scenes.random_soup(rng, n, extent=float(rng.uniform(0.5, 3.0)), size=float(rng.uniform(0.05, 1.0)))
            meshes.append(oracle.mesh_prep(tri, float(rng.uniform(0.5, 2.0)), tuple(rng.uniform(-1, 1, 3)),
                                           tuple(rng.uniform(-4, 4, 3) + np.array([0, 1.5, -9])), rand_mat()))
        else:
            meshes.append(scenes.standin_mesh(oracle, n + 50, float(rng.uniform(15, 60)), tuple(rng.uniform(-5, 5, 3) + np.array([0, 0, -10])),
                                              tuple(rng.uniform(-1, 1, 3)), rand_mat()))
    if not spheres and not meshes:
        spheres.append(((0.0, 1.0, -8.0), 1.0, rand_mat()))
    return abi.SceneData(spheres=spheres, meshes=meshes)


def fuzz_camera(oracle, rng, sc, w, h):
    """A camera where the table's margins are thinnest: inside a sphere, ON its surface, within 1e-3 r of it either side, low
    over the ground sphere looking along its horizon, inside or right behind a mesh's box -- or anywhere; `look_at` and `up`
    random and not orthogonal to each other (cam.rs:30-33, 55 takes whatever it is given), focal length 4-2000 mm."""
    mode = int(rng.integers(0, 8))
    pos = rng.uniform(-12, 12, 3) + np.array([0.0, 3.0, -4.0])
    look = _unit(rng)
    if sc.spheres and mode in (1, 2, 3, 4):
        c, r, _ = sc.spheres[int(rng.integers(len(sc.spheres)))]
        c = np.array(c, np.float64)
        u = _unit(rng)
        if mode == 1:    # inside
            pos = c + u * r * rng.uniform(0.0, 0.999)
        elif mode == 2:  # on the surface, to float precision
            pos = (np.asarray(c, f32) + (u * r).astype(f32)).astype(np.float64)
        elif mode == 3:  # a thousandth of the radius off the surface, either side
            pos = c + u * r * (1.0 + rng.choice([-1.0, 1.0]) * rng.uniform(1e-6, 1e-3))
        else:            # just above it, looking along its horizon (a little up or down)
            pos = c + u * r * (1.0 + _log_uniform(rng, 1e-5, 1e-1))
            t = np.cross(u, _unit(rng))
            look = t / np.linalg.norm(t) + u * rng.uniform(-0.05, 0.05)
        if mode != 4 and rng.random() < 0.5:
            look = (c - pos) / max(1e-9, np.linalg.norm(c - pos)) + _unit(rng) * rng.uniform(0.0, 1.5)  # towards the centre, roughly
    elif sc.meshes and mode in (5, 6):
        md = sc.meshes[int(rng.integers(len(sc.meshes)))]
        lo, hi = md.bbox_lo.astype(np.float64), md.bbox_hi.astype(np.float64)
        if mode == 5:    # inside the box
            pos = lo + (hi - lo) * rng.uniform(0.0, 1.0, 3)
        else:            # behind it: the box is at the camera's back, or grazed sideways
            ctr, half = 0.5 * (lo + hi), 0.5 * np.linalg.norm(hi - lo)
            u = _unit(rng)
            pos = ctr + u * half * rng.uniform(1.0, 3.0)
            look = u + _unit(rng) * rng.uniform(0.0, 1.2)
    look = look / np.linalg.norm(look)
    up = _unit(rng)
    while abs(float(np.dot(up, look))) > 0.95:  # (not parallel: a degenerate camera is another test's subject)
        up = _unit(rng)
    return oracle.camera_new(tuple(float(x) for x in pos), tuple(float(x) for x in look), tuple(float(x) for x in up), h, w,
                             _log_uniform(rng, 4.0, 2000.0))


@pytest.mark.parametrize("k", range(N_FUZZ))
def test_fuzzed_cameras_no_camera_ray_passes_a_culled_test(hip, oracle, k):
    """RBRT_FUZZ_CAMERAS (default 60) random cameras over random scenes through check_table: every bit the table sets is
    checked against the oracle's routines over the tile's rays, as for the hand-picked cameras above. Every third case also
    renders the whole image through the tile pass and compares it with the oracle's, bit for bit."""
    rng = np.random.default_rng(77000 + k)
    sc = fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 301)), int(rng.integers(9, 201))
    cam = fuzz_camera(oracle, rng, sc, w, h)
    # (the camera's far limit is the render's max_dist; the reference's 2000 most of the time)
    table, _ = check_table(hip, oracle, cam, sc, rng, full_scene_jitters=4)
    if k % 3 == 0:
        spp = int(rng.integers(1, 4))
        exp, exp8, rays = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=k, max_depth=12))
        got, got8 = hip.render_scene(cam, spp, sc, seed=k, max_depth=12)
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), (k, w, h, int(np.count_nonzero(table >> 31)))
        assert np.array_equal(got8, exp8)
