"""The short-path stage (short_paths.inl; DESIGN.md "The tile pass"): a streaming kernel in front of every trace launch
finishes the two-ray paths of the tiles no camera ray of which can pass a mesh box, and the trace kernel hands out only
the samples the stage left (one 64-bit finished mask per chunk of 64 work items). Which kernel finishes a sample must
never show: every case here compares the float32 radiance bit for bit with the CPU oracle AND with the same render with
the stage off (rbrt_hip_scene_set_short_paths), on images of a few 8x8 tiles, with poisoned sample buffers, so that a
sample neither kernel wrote is a NaN and one both wrote differently would be caught by one of the two references.

The masks come back through rbrt_hip_debug_short_masks: the tests use them to show that a case exercised both sides (the
stage finished some samples and declined others) and that the boundary shapes of the hand-out logic occurred."""
from __future__ import annotations

import numpy as np
import pytest

import np_env
import np_lens
import np_reference as R
import np_smooth
import scenes
import test_np_reference as T
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

L, M, D, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
GROUND = ((0.0, -1000.0, -5.0), 1000.0, abi.material(L, (0.02, 0.2, 0.1)))
SMALL, RAGGED = (16, 16), (20, 12)  # 2 x 2 whole tiles; 3 x 2 tiles with a ragged right and bottom edge


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in masks], np.int64)


def frame(torch, cam):
    return torch.full((cam.img_height_pix, cam.img_width_pix, 3), float("nan"), dtype=torch.float32, device="cuda")


def render(hs, cam, opts, lens=None):
    import torch
    out = frame(torch, cam)
    hs.render_device(cam, opts, out.data_ptr(), lens=lens)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def on_and_off(hs, cam, opts, lens=None):
    """(image with the stage, its finished masks, image without it) of blocking renders on one handle (mode 2: the stage
    in front of every launch; by default a blocking frame has none)."""
    hs.set_short_paths(2)
    on = render(hs, cam, opts, lens)
    masks = hs.short_masks()
    hs.set_short_paths(0)
    off = render(hs, cam, opts, lens)
    hs.set_short_paths(2)
    hs.check()
    return on, masks, off


def assert_same(got, exp, what):
    assert np.isfinite(got).all() or np.array_equal(np.isnan(got), np.isnan(exp)), f"{what}: a sample was not written"
    diff = np.argwhere(bits(got) != bits(exp))
    assert diff.size == 0, f"{what}: {len(diff)} values differ, first at {diff[:4].tolist()}"


def assert_both_sides(masks, what, ragged=False):
    """The stage finished some samples and left some to the trace kernel."""
    n = popcount(masks)
    assert n.sum() > 0, f"{what}: the stage finished nothing"
    if not ragged:
        assert (n < 64).any(), f"{what}: the stage finished every sample of every chunk"


def restated_masks(cam, sc, opts, cull):
    """The stage's rule restated on the host (np_reference), for a pinhole scene of lambertian, metal and glass spheres and
    BasicTriangles without meshes: the finished masks of the tiles on the work list (cull: the tile pass's table), sorted --
    the order of the work list is the library's business. A sample is finished when its camera ray hits nothing, when
    max_depth is 0, when its scatter fails, or when its second ray hits nothing or ends the path (max_depth 1). The stage
    gives a tile up after the launch's first two samples unless three quarters of their 128 slots finished: the chunks it
    does not do have a zero mask. (One launch: opts.spp samples.)"""
    nc, ns = T.np_cam(cam), np_smooth.np_scene(sc)
    H, W = nc["H"], nc["W"]
    lo, hi = np.float32(opts.min_dist), np.float32(opts.max_dist)
    out = []
    for ty, tx in np.argwhere((cull >> 31) == 0).tolist():
        probe = 0
        for s in range(opts.spp):
            if s == 2 and probe * 4 < 2 * 64 * 3:
                out += [0] * (opts.spp - 2)
                break
            m = 0
            for p in range(64):
                row, col = ty * 8 + p // 8, tx * 8 + p % 8
                fin = True  # (a slot beyond a ragged edge counts as finished)
                if row < H and col < W:
                    rng = R.Rng(opts.seed, row * W + col, s)
                    o, d = R.camera_ray(nc, row, col, rng)
                    hit = R.scene_hit(ns, o, d, lo, hi)
                    if hit is not None and opts.max_depth > 0:
                        ok, _, o2, d2 = R.scatter(hit["mat"], d, hit, rng)
                        if ok:
                            fin = R.scene_hit(ns, o2, d2, lo, hi) is None or opts.max_depth == 1
                m |= int(fin) << p
            probe += bin(m).count("1") if s < 2 else 0
            out.append(m)
    return sorted(out)


def assert_masks(masks, cam, sc, opts, cull, what):
    exp = restated_masks(cam, sc, opts, cull)
    assert sorted(int(m) for m in masks) == exp, f"{what}: the finished masks are not the restated rule's"


@pytest.fixture(autouse=True)
def poisoned(monkeypatch):
    monkeypatch.setenv("RBRT_HIP_LAB", "1")
    monkeypatch.setenv("RBRT_POISON_SAMPLES", "1")


# ---- scenes ------------------------------------------------------------------------------------------------------------------
def side_mesh_scene(oracle):
    """The example spheres and a 12-triangle mesh at the right edge of the view."""
    mesh = scenes.standin_mesh(oracle, 12, 30.0, (7.5, -2.4, -10.0), (0.0, 0.0, 0.0), abi.material(L, (0.9, 0.2, 0.2)))
    assert mesh.n_real == 12
    return abi.SceneData(spheres=scenes.EXAMPLE_SPHERES, meshes=[mesh])


SPHERE_SCENES = {
    "spheres": lambda o: (scenes.spheres_scene(), {}),
    "fuzzy_metal": lambda o: (abi.SceneData(spheres=[GROUND, ((0.0, 2.0, -9.0), 2.0, abi.material(M, (0.9, 0.8, 0.7), 0.95))]), {}),
    "glass": lambda o: (abi.SceneData(spheres=[GROUND, ((0.0, 2.0, -9.0), 2.0, abi.material(D, (0, 0, 0), 1.5))]), {}),
    "emitter_black_bg": lambda o: (abi.SceneData(spheres=[GROUND, ((0.0, 2.0, -9.0), 2.0, abi.material(EM, (4.0, 3.0, 2.0))),
                                                          ((-4.0, 1.0, -8.0), 1.0, abi.material(L, (0.7, 0.7, 0.7)))]),
                                   dict(flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))),
    "basic_triangles": lambda o: (scenes.triangle_scene(), {}),
}


@pytest.mark.parametrize("size", [SMALL, RAGGED], ids=["16x16", "20x12"])
@pytest.mark.parametrize("name", list(SPHERE_SCENES))
def test_scenes_without_a_mesh(hip, oracle, name, size):
    """Every tile that is not background-only is the stage's: spheres of every material, BasicTriangle elements."""
    sc, kw = SPHERE_SCENES[name](oracle)
    cam = scenes.camera(oracle, *size)
    opts = abi.default_opts(spp=4, seed=3, **kw)
    exp = oracle.render(cam, sc, opts)[0]
    with hip.HipScene(sc) as hs:
        on, masks, off = on_and_off(hs, cam, opts)
    assert_same(on, exp, f"{name} against the oracle")
    assert_same(on, off, f"{name} against the stage off")
    assert_both_sides(masks, name, ragged=size == RAGGED)


def test_finished_count_on_the_spheres_scene(hip, oracle):
    """Neither zero nor all: a test that exercised one side only would say so here."""
    sc, cam, opts = scenes.spheres_scene(), scenes.camera(oracle, *SMALL), abi.default_opts(spp=5, seed=1)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    n_work = int(np.count_nonzero((cull >> 31) == 0))
    assert n_work >= 1 and len(masks) == n_work * 5, (cull, len(masks))
    finished, total = int(popcount(masks).sum()), n_work * 5 * 64
    print(f"spheres 16x16x5: the stage finished {finished} of {total} samples")
    assert 0 < finished < total
    assert_masks(masks, cam, sc, opts, cull, "spheres")
    assert_same(on, oracle.render(cam, sc, opts)[0], "spheres")
    assert_same(on, off, "spheres, stage off")


def test_a_mesh_at_one_side(hip, oracle):
    """Tiles of all three kinds in one image: the stage's, the trace kernel's alone (the mesh box in reach), background only."""
    sc = side_mesh_scene(oracle)
    cam = scenes.camera(oracle, 96, 64)  # (12 x 8 tiles: the top row is far enough above the horizon to be background-only)
    opts = abi.default_opts(spp=3, seed=7)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    sky, mesh_free = (cull >> 31) != 0, ((cull >> 24) & 1) != 0
    assert sky.any() and (mesh_free & ~sky).any() and (~mesh_free).any(), cull
    # a chunk with a finished sample belongs to a mesh-free tile: there are at most that many, three samples each
    n = popcount(masks)
    assert 0 < np.count_nonzero(n) <= 3 * np.count_nonzero(mesh_free & ~sky)
    assert np.count_nonzero(n == 0) >= 3 * np.count_nonzero(~mesh_free)
    assert_same(on, oracle.render(cam, sc, opts)[0], "side mesh")
    assert_same(on, off, "side mesh, stage off")


@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_max_depth(hip, oracle, depth):
    sc, cam = scenes.spheres_scene(), scenes.camera(oracle, *RAGGED)
    opts = abi.default_opts(spp=3, seed=9, max_depth=depth)
    with hip.HipScene(sc) as hs:
        on, masks, off = on_and_off(hs, cam, opts)
    assert_same(on, oracle.render(cam, sc, opts)[0], f"max_depth {depth}")
    assert_same(on, off, f"max_depth {depth}, stage off")
    if depth <= 1:  # no path has a third ray: the stage finishes everything
        assert (popcount(masks) == 64).all()
    else:
        assert_both_sides(masks, f"max_depth {depth}", ragged=True)


def test_thin_lens(hip, oracle):
    sc, cam = scenes.spheres_scene(), scenes.camera(oracle, *RAGGED)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 20.0, 10.0)
    opts = abi.default_opts(spp=4, seed=11)
    with hip.HipScene(sc) as hs:
        on, masks, off = on_and_off(hs, cam, opts, lens)
    assert_same(on, oracle.render(cam, sc, opts, lens=lens)[0], "thin lens")
    assert_same(on, off, "thin lens, stage off")
    assert_both_sides(masks, "thin lens", ragged=True)


def test_environment_map(hip, oracle):
    """The oracle has no environment: the numpy restatement of the render (np_env) is the reference, on every third pixel."""
    sc, cam = scenes.spheres_scene(), scenes.camera(oracle, *SMALL)
    opts = abi.default_opts(spp=3, seed=13)
    nodes = np_env.noise_map(8, 5)
    with hip.HipScene(sc) as hs:
        hs.set_environment(nodes)
        on, masks, off = on_and_off(hs, cam, opts)
    pixels = [(r, c) for r in range(16) for c in range(16) if (r * 16 + c) % 3 == 0]
    exp = np_env.restated_image(cam, sc, opts, nodes, pixels=pixels)[0]
    for r, c in pixels:
        assert np.array_equal(bits(on[r, c]), bits(exp[r, c])), (r, c)
    assert_same(on, off, "environment, stage off")
    assert_both_sides(masks, "environment")


# ---- schedules ---------------------------------------------------------------------------------------------------------------
def test_tiles_of_three_ranks(hip, oracle):
    import torch
    sc, cam, world = side_mesh_scene(oracle), scenes.camera(oracle, 40, 24), 3
    w, h = 40, 24
    slot = hip.packed_pixels(w, h, 0, world)
    merged = {}
    with hip.HipScene(sc) as hs:
        for on in (True, False):
            hs.set_short_paths(2 if on else 0)
            slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
            finished = 0
            for r in range(world):
                hs.render_device(cam, abi.default_opts(spp=3, seed=4, tile_rank=r, tile_world=world), slots[r * slot * 3:].data_ptr())
                if on:
                    finished += int(popcount(hs.short_masks()).sum())
            out = frame(torch, cam)
            hip.unpack_tiles(0, slots.data_ptr(), w, h, world, out.data_ptr(), None, None, rank_stride_pixels=slot)
            torch.cuda.synchronize()
            merged[on] = out.cpu().numpy()
            if on:
                assert finished > 0
        hs.check()
    assert_same(merged[True], oracle.render(cam, sc, abi.default_opts(spp=3, seed=4))[0], "three ranks")
    assert_same(merged[True], merged[False], "three ranks, stage off")


def test_two_batches(hip, oracle, monkeypatch):
    """A 1 MiB workspace holds 227 samples of the 20x12 image's six tiles: 300 samples take two launches, each with its own
    stage over its own sample range."""
    monkeypatch.setenv("RBRT_HIP_WORKSPACE_MB", "1")
    sc, cam = scenes.spheres_scene(), scenes.camera(oracle, *RAGGED)
    opts = abi.default_opts(spp=300, seed=2)
    with hip.HipScene(sc) as hs:
        on, masks, off = on_and_off(hs, cam, opts)
        per_batch, n_batches = hs.last_batches()
    assert n_batches == 2 and len(masks) % (300 - per_batch) == 0, (per_batch, n_batches, len(masks))  # (the second launch's masks)
    assert_same(on, oracle.render(cam, sc, opts)[0], "two batches")
    assert_same(on, off, "two batches, stage off")
    assert_both_sides(masks, "two batches", ragged=True)


def test_two_passes(hip, oracle):
    import torch
    sc, cam = scenes.spheres_scene(), scenes.camera(oracle, *RAGGED)
    opts = abi.default_opts(spp=5, seed=6)
    exp = oracle.render(cam, sc, opts)[0]
    with hip.HipScene(sc) as hs:
        for on in (True, False):
            hs.set_short_paths(2 if on else 0)
            acc, out = frame(torch, cam), frame(torch, cam)
            hs.render_pass(cam, opts, 0, 2, acc.data_ptr())
            if on:
                assert len(hs.short_masks()) % 2 == 0 and popcount(hs.short_masks()).sum() > 0
            hs.render_pass(cam, opts, 2, 5, acc.data_ptr(), out.data_ptr())
            torch.cuda.synchronize()
            if on:
                assert len(hs.short_masks()) % 3 == 0 and popcount(hs.short_masks()).sum() > 0
            assert_same(out.cpu().numpy(), exp, f"two passes, stage {'on' if on else 'off'}")
        hs.check()


def stream_of_frames(hs, cams, opts_list):
    import torch
    outs = [frame(torch, c) for c in cams]
    for c, o, t in zip(cams, opts_list, outs):
        hs.render_device(c, o, t.data_ptr())
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in outs]


@pytest.mark.parametrize("depth", [1, 0, 3], ids=["pipeline_1", "pipeline_auto", "pipeline_3"])
@pytest.mark.parametrize("helpers", [None, "2"], ids=["", "helpers_2"])
def test_a_stream_whose_camera_changes(hip, oracle, monkeypatch, depth, helpers):
    """Four frames queued without a wait in between, each from its own camera with its own seed and sample count: the
    lanes' tile tables, masks and sample buffers are reused from frame to frame. With RBRT_HELPERS=2 every overlapped launch
    gets a helper launch, which reads the masks of the launch it joins."""
    if helpers:
        monkeypatch.setenv("RBRT_HELPERS", helpers)
        monkeypatch.setenv("RBRT_HELPER_MIN_ITEMS", "1")
        monkeypatch.setenv("RBRT_HELPER_MIN_LAUNCH_MI", "0")
        monkeypatch.setenv("RBRT_HELPER_MIN_FREE", "1")
    sc = side_mesh_scene(oracle)
    cams = [scenes.camera(oracle, 40, 24, position=(0.3 * k - 0.5, 5.0 + 0.2 * k, 4.0)) for k in range(4)]
    opts = [abi.default_opts(spp=3 + k % 3, seed=20 + k) for k in range(4)]
    exp = [oracle.render(c, sc, o)[0] for c, o in zip(cams, opts)]
    with hip.HipScene(sc) as hs:
        hs.set_pipeline(depth)
        for mode in (2, 0, 1, 2):  # (1: whichever launches the library finds running beside others)
            hs.set_short_paths(mode)
            got = stream_of_frames(hs, cams, opts)
            for k in range(4):
                assert_same(got[k], exp[k], f"stage mode {mode}, frame {k}")
            if mode == 2:
                assert popcount(hs.short_masks()).sum() > 0
        hs.check()


# ---- boundary shapes of the hand-out logic -------------------------------------------------------------------------------------
def test_chunks_finished_whole_and_not_at_all(hip, oracle):
    """The ground alone: a scattered ray leaves a convex body for good, so the stage finishes all 64 samples of every chunk
    and the trace kernel opens one empty mask after the other. Under a second huge sphere eight units above the ground,
    looking down, all but the flattest second rays hit it and have to scatter again: chunks have no finished sample at all
    although every tile is the stage's."""
    cam, opts = scenes.camera(oracle, *SMALL, look_at=(0.0, -1.0, -0.3)), abi.default_opts(spp=4, seed=5)
    ground = abi.SceneData(spheres=[GROUND])
    ceiling = abi.SceneData(spheres=[GROUND, ((0.0, 1008.0, -5.0), 1000.0, abi.material(L, (0.5, 0.6, 0.7)))])
    for sc, what in ((ground, "ground only"), (ceiling, "under a ceiling")):
        with hip.HipScene(sc) as hs:
            cull = hs.primary_cull(cam)
            on, masks, off = on_and_off(hs, cam, opts)
        assert not (cull >> 31).any() and len(masks) == 4 * cull.size, (cull, len(masks))
        n = popcount(masks)
        print(f"{what}: finished samples per chunk {n.tolist()}")
        assert (n == 64).all() if sc is ground else ((n == 0).any() and (n < 64).all()), (what, n)
        assert_masks(masks, cam, sc, opts, cull, what)
        assert_same(on, oracle.render(cam, sc, opts)[0], what)
        assert_same(on, off, f"{what}, stage off")


def test_a_chunk_with_one_sample_left(hip, oracle):
    """Near the objects most chunks lose a few samples to second rays that hit something: by the restated rule this render
    has chunks with exactly one sample left to the trace kernel."""
    sc, cam, opts = scenes.spheres_scene(), scenes.camera(oracle, 48, 32), abi.default_opts(spp=5, seed=40)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    assert (popcount(restated_masks(cam, sc, opts, cull)) == 63).any()
    assert_masks(masks, cam, sc, opts, cull, "48x32 spheres")
    assert_same(on, oracle.render(cam, sc, opts)[0], "one sample left")
    assert_same(on, off, "one sample left, stage off")


def test_the_last_chunk_is_the_only_one_of_the_stage(hip, oracle):
    """Two tiles side by side, one sample: a mesh fills one of them. Whichever way the work list runs, in one of the two
    mirrored scenes the stage's tile comes last."""
    cam, opts = scenes.camera(oracle, 16, 8), abi.default_opts(spp=1, seed=8)
    last_only = 0
    for x in (-1.0, 1.0):
        mesh = scenes.standin_mesh(oracle, 12, 30.0, (7.5 if x > 0 else -6.5, -2.4, -10.0), (0.0, 0.0, 0.0), abi.material(L, (0.9, 0.2, 0.2)))
        sc = abi.SceneData(spheres=[GROUND], meshes=[mesh])
        with hip.HipScene(sc) as hs:
            cull = hs.primary_cull(cam)
            on, masks, off = on_and_off(hs, cam, opts)
        assert cull.shape == (1, 2) and np.count_nonzero((cull >> 24) & 1) == 1 and not (cull >> 31).any(), cull
        assert len(masks) == 2 and np.count_nonzero(masks) == 1, masks
        last_only += int(masks[0] == 0 and masks[1] != 0)
        assert_same(on, oracle.render(cam, sc, opts)[0], f"mesh at x = {x}")
        assert_same(on, off, f"mesh at x = {x}, stage off")
    assert last_only >= 1


def test_a_wave_served_from_three_chunks(hip, oracle, monkeypatch):
    """One wave per CU and more than twice as many chunks as waves, each with at most 21 samples left: a wave's first
    generation step wants 64 work items, so unless the work runs out under it, it is served from at least three chunks -- and
    the work cannot run out under every wave's first step, because together two chunks each would not use it up."""
    monkeypatch.setenv("RBRT_WAVES_PER_CU", "1")
    speck = ((0.5, 0.12, -6.0), 0.12, abi.material(L, (0.8, 0.3, 0.3)))
    sc, cam = abi.SceneData(spheres=[GROUND, speck]), scenes.camera(oracle, 64, 48)
    opts = abi.default_opts(spp=24, seed=1)
    with hip.HipScene(sc) as hs:
        waves = hs.info()["trace_waves"]
        on, masks, off = on_and_off(hs, cam, opts)
    left = 64 - popcount(masks)
    assert len(masks) > 2 * waves, (len(masks), waves)
    assert left.max() <= 21 and left.sum() > 0, (left.max(), left.sum())
    assert_same(on, oracle.render(cam, sc, opts)[0], "three chunks")
    assert_same(on, off, "three chunks, stage off")


def test_the_switch_and_the_hook_on_a_fresh_handle(hip):
    with hip.HipScene(scenes.spheres_scene()) as hs:
        assert len(hs.short_masks()) == 0  # (no launch yet)
        for bad in (3, -1):
            assert hs._lib.rbrt_hip_scene_set_short_paths(hs._h, bad) == abi.RBRT_ERR_INVALID_ARG
        for mode in (0, 2, 1):
            hs.set_short_paths(mode)


def test_by_default_only_launches_that_run_beside_others_have_the_stage(hip, oracle, monkeypatch):
    """A blocking frame of one batch pays the stage's latency in full and gets none; of a call of two batches on a pipeline
    the first runs beside the second and has it, the last does not."""
    monkeypatch.setenv("RBRT_HIP_WORKSPACE_MB", "1")
    sc, cam = scenes.spheres_scene(), scenes.camera(oracle, *RAGGED)
    one, two = abi.default_opts(spp=4, seed=2), abi.default_opts(spp=300, seed=2)
    with hip.HipScene(sc) as hs:
        hs.set_pipeline(3)
        cull = hs.primary_cull(cam)
        got = render(hs, cam, one)
        assert len(hs.short_masks()) == 0
        assert_same(got, oracle.render(cam, sc, one)[0], "a blocking frame")
        got = render(hs, cam, two)
        per_batch, n_batches = hs.last_batches()
        masks = hs.short_masks()
        hs.check()
    assert n_batches == 2 and len(masks) == per_batch * np.count_nonzero((cull >> 31) == 0), (per_batch, n_batches, len(masks))
    assert popcount(masks).sum() > 0
    assert_same(got, oracle.render(cam, sc, two)[0], "two batches on a pipeline")
