"""The camera shutter (rbrt_hip_scene_set_shutter) on the GPU.

Images: bit for bit against the numpy restatement (np_shutter.restated_image) for pinhole and lens cameras, travels from zero
to one that carries the camera through a glass sphere and into a mesh's box, with a checkered ground, a smooth mesh and an
environment (the places that read the origin), through every entry point, with the tile pass, the short-path stage and helper
launches switched by their lab knobs. The feature buffers against a numpy evaluation from the restated rays. The tile pass:
every bit the shutter table sets is checked against the oracle's routines over shutter rays of the tile, for hand-picked and
fuzzed cameras, and the bench frame keeps its background-only tiles. The C ABI's refusals and the C++ host."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import np_env
import np_features
import np_lens
import np_shutter as NS
import np_smooth
import scenes
import test_primary_cull as PC
import test_thin_lens as TL
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
L_, M_, D_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
POS = scenes.CAMERA["position"]
SKEW = (0.3, -0.2, 0.1)
DEPTH = 12  # (bounces: enough for every material to be met several times, and the restatement stays quick)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def mixed_scene(oracle, near=False):
    """Spheres of all four materials and a small mesh. near: also a glass sphere one unit to the camera's right and a small
    mesh just to its left, for travels that carry the origin through the one's surface and into the other's box."""
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(EM, (3.0, 2.5, 1.5)))]
    meshes = [scenes.standin_mesh(oracle, 61, 30.0, (4.0, -1.2, -11.0), (0.0, 0.5, 0.0), abi.material(M_, (0.7, 0.6, 0.5), 0.1))]
    if near:
        sph.append(((POS[0] + 1.0, POS[1], POS[2]), 0.5, abi.material(D_, (0, 0, 0), 1.5)))
        meshes.append(scenes.standin_mesh(oracle, 61, 10.0, (POS[0] - 1.5, POS[1] - 0.3, POS[2] - 0.2), (0.0, 0.0, 0.0), abi.material(L_, (0.8, 0.3, 0.2))))
    return abi.SceneData(spheres=sph, meshes=meshes)


def lens_of(cam):
    return np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 40.0, 9.0)


def render(hip, hs, cam, opts, lens=None):
    import torch
    h, w = cam.img_height_pix, cam.img_width_pix
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    hs.render_device(cam, opts, out.data_ptr(), out8.data_ptr(), lens=lens)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out8.cpu().numpy()


def check_image(hip, oracle, sc, w, h, lensed, travel, spp=2, seed=7, nodes=None, **kw):
    cam = scenes.camera(oracle, w, h)
    lens = lens_of(cam) if lensed else None
    opts = abi.default_opts(spp=spp, seed=seed, max_depth=DEPTH, **kw)
    exp, exp8 = NS.restated_image(cam, sc, opts, lens, travel, nodes=nodes)
    with hip.HipScene(sc) as hs:
        if nodes is not None:
            hs.set_environment(nodes)
        hs.set_shutter(travel)
        got, got8 = render(hip, hs, cam, opts, lens)
        hs.check()
        table = hs.primary_cull_shutter(cam, lens, travel)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    return got, table


# ---- whole images ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("travel", [(0.0, 0.0, 0.0), (1e-6, 0.0, 0.0), SKEW, (10.0, 0.0, 0.0)], ids=["zero", "tiny", "skew", "ten_units"])
def test_ragged_images_are_bit_identical_to_the_restatement(hip, oracle, lensed, travel):
    """20 x 12: ragged both ways, 3 x 2 tiles."""
    sc = mixed_scene(oracle)
    got, table = check_image(hip, oracle, sc, 20, 12, lensed, travel)
    if travel[0] == 10.0:  # (the ground sphere is in every tile's reach: no tile is background only)
        assert not (table >> 31).any()
    if travel == (0.0, 0.0, 0.0):  # (a zero travel still draws: not the shutterless image)
        cam = scenes.camera(oracle, 20, 12)
        with hip.HipScene(sc) as hs:
            plain, _ = render(hip, hs, cam, abi.default_opts(spp=2, seed=7, max_depth=DEPTH), lens_of(cam) if lensed else None)
        assert not np.array_equal(bits(plain), bits(got))


@pytest.mark.parametrize("case", ["pinhole_skew", "lens_skew", "through_the_glass", "into_the_box"])
def test_whole_tile_images_are_bit_identical_to_the_restatement(hip, oracle, case):
    """32 x 24. through_the_glass: the travel carries the origin through the surface of a glass sphere beside the camera;
    into_the_box: to the middle of the box of a small mesh on its other side."""
    near = case in ("through_the_glass", "into_the_box")
    sc = mixed_scene(oracle, near)
    travel = SKEW
    if case == "through_the_glass":
        travel = (1.2, 0.0, 0.0)  # the sphere's surface is 0.5 to 1.5 units to the right: t = 0.42 .. 1 is inside
    if case == "into_the_box":
        md = sc.meshes[1]
        mid = 0.5 * (md.bbox_lo.astype(np.float64) + md.bbox_hi.astype(np.float64))
        assert not all(md.bbox_lo[c] <= POS[c] <= md.bbox_hi[c] for c in range(3))  # (the shutter opens outside the box)
        travel = tuple(float(f32(mid[c] - POS[c])) for c in range(3))
    check_image(hip, oracle, sc, 32, 24, case == "lens_skew", travel)


def test_a_checkered_ground_reads_the_shifted_origin(hip, oracle):
    import test_pattern_gpu as TP
    check_image(hip, oracle, TP.sphere_scene(), 20, 12, False, SKEW)


def test_a_smooth_mesh_reads_the_shifted_origin(hip, oracle):
    _, ball = np_smooth.sphere_mesh(oracle, (1.0, 1.2, -6.0), 1.2, 2, abi.material(M_, (0.8, 0.8, 0.75), 0.05))
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES[:2]), meshes=[ball])
    check_image(hip, oracle, sc, 20, 12, False, SKEW)


def test_an_environment_map_with_a_shutter(hip, oracle):
    check_image(hip, oracle, mixed_scene(oracle), 20, 12, True, SKEW, nodes=np_env.noise_map(8, 3))


# ---- every entry point -----------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_restated_image(hip, oracle):
    """render_device, a render_pass series of 2 + 3 samples, render_adaptive with threshold 0, three ranks' packed tiles
    gathered and the counting kernel, on one handle."""
    import torch
    w, h, spp = 20, 12, 5
    cam = scenes.camera(oracle, w, h)
    lens = lens_of(cam)
    sc = mixed_scene(oracle)
    opts = abi.default_opts(spp=spp, seed=11, max_depth=DEPTH)
    exp, exp8 = NS.restated_image(cam, sc, opts, lens, SKEW)

    def img():
        return torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")

    def same(t, what):
        torch.cuda.synchronize()
        assert np.array_equal(bits(t.cpu().numpy()), bits(exp)), what

    with hip.HipScene(sc) as hs:
        hs.set_shutter(SKEW)
        got, got8 = render(hip, hs, cam, opts, lens)
        assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8), "render_device"
        acc, out = img(), img()
        for b, e in ((0, 2), (2, spp)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == spp else None, lens=lens)
        same(out, "render_pass 0-2, 2-5")
        out = img()
        res = hs.render_adaptive(cam, opts, 0.0, 2, 2, out.data_ptr(), lens=lens)
        same(out, "render_adaptive, threshold 0")
        assert res["samples"] == res["samples_fixed"]
        world = 3
        slot = hip.packed_pixels(w, h, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            o = abi.default_opts(spp=spp, seed=11, max_depth=DEPTH, tile_rank=r, tile_world=world)
            hs.render_device(cam, o, slots[r * slot * 3:].data_ptr(), lens=lens)
        merged = img()
        hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        same(merged, "tile_world 3 + unpack")
        out = img()
        hs.render_device(cam, abi.default_opts(spp=spp, seed=11, max_depth=DEPTH, flags=abi.FLAG_COLLECT_STATS), out.data_ptr(), lens=lens)
        same(out, "COLLECT_STATS")
        assert hs.stats()["samples"] == w * h * spp
        hs.check()


@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
def test_feature_buffers_trace_the_shutter_rays(hip, oracle, lensed):
    import torch
    w, h, n = 20, 12, 3
    cam = scenes.camera(oracle, w, h)
    lens = lens_of(cam) if lensed else None
    sc = mixed_scene(oracle, near=True)
    opts = abi.default_opts(spp=2, seed=5)
    rays = NS.primary_rays(cam, 5, n, lens, (1.2, 0.1, 0.0))
    plain = np_features.primary_rays(cam, 5, n, lens)
    assert np.array_equal(bits(rays[..., 3:]), bits(plain[..., 3:])) and not np.array_equal(bits(rays[..., :3]), bits(plain[..., :3]))
    exp = np_features.features(oracle, cam, sc, opts, n, lens, rays=rays)
    bufs = dict(albedo=torch.full((h, w, 3), float("nan"), device="cuda"), normal=torch.full((h, w, 3), float("nan"), device="cuda"),
                depth=torch.full((h, w), float("nan"), device="cuda"), coverage=torch.full((h, w), float("nan"), device="cuda"),
                object=torch.full((h, w), -7, dtype=torch.int32, device="cuda"))
    with hip.HipScene(sc) as hs:
        hs.set_shutter((1.2, 0.1, 0.0))
        hs.render_features(cam, opts, n, lens=lens, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        hs.check()
    for k in ("albedo", "normal", "depth", "coverage"):
        assert np.array_equal(bits(bufs[k].cpu().numpy()), bits(getattr(exp, k))), k
    assert np.array_equal(bufs["object"].cpu().numpy(), exp.object)
    without = np_features.features(oracle, cam, sc, opts, n, lens, rays=plain)
    assert not np.array_equal(bits(without.depth), bits(exp.depth))  # (the shutter does something here)


def test_shutter_and_shutterless_frames_on_one_handle(hip, oracle):
    """No shutter, travel A, no shutter, travel B: each frame is its own image, the shutterless ones the oracle's, and the
    handle's LDS bytes per wave are what they were (a shutterless launch keeps its size and layout)."""
    w, h = 64, 48
    cam = scenes.camera(oracle, w, h)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))
    opts = abi.default_opts(spp=1, seed=2, max_depth=DEPTH)
    A, B = (0.5, 0.0, 0.0), (0.0, 0.4, -0.3)
    pin = oracle.render(cam, sc, opts)[0]
    rng = np.random.default_rng(5)
    pix = sorted({(int(r), int(c)) for r, c in zip(rng.integers(0, h, 160), rng.integers(0, w, 160))})
    with hip.HipScene(sc) as hs:
        before = hs.info()["lds_bytes_per_wave"]
        assert (hs.primary_cull(cam) >> 31).any()
        frames = []
        for travel in (None, A, None, B):
            hs.set_shutter(travel)
            frames.append(render(hip, hs, cam, opts)[0])
            assert hs.info()["lds_bytes_per_wave"] == before
        hs.check()
    assert np.array_equal(bits(frames[0]), bits(pin)) and np.array_equal(bits(frames[2]), bits(pin))
    for got, travel in ((frames[1], A), (frames[3], B)):
        exp, _ = NS.restated_image(cam, sc, opts, None, travel, pixels=pix)
        for r, c in pix:
            assert np.array_equal(bits(got[r, c]), bits(exp[r, c])), (travel, r, c)
        assert not np.array_equal(bits(got), bits(pin))
    # (the background-only tiles of a frame are its camera's own: the sky does not see the shutter)
    sky = np.repeat(np.repeat(TL_table_sky(hip, sc, cam, A), 8, 0), 8, 1)[:h, :w]
    assert sky.any() and np.array_equal(bits(frames[1][sky]), bits(pin[sky]))


def TL_table_sky(hip, sc, cam, travel):
    with hip.HipScene(sc) as hs:
        return (hs.primary_cull_shutter(cam, None, travel) >> 31) != 0


# ---- lab knobs: the tile pass off, the short-path stage off and forced, helper launches forced ---------------------------------
KNOBS = {"no_tile_pass": {"RBRT_PRIMARY_CULL": "0"}, "helpers_forced": {"RBRT_HELPERS": "2"}}


@pytest.mark.parametrize("knob", list(KNOBS))
def test_the_same_image_under_a_lab_knob(hip, oracle, tmp_path, knob):
    cam = scenes.camera(oracle, 64, 48)
    sc = scenes.example_scene(oracle, 603)
    with hip.HipScene(sc) as hs:
        hs.set_shutter(SKEW)
        got, _ = render(hip, hs, cam, abi.default_opts(spp=3, seed=5))
        assert (hs.primary_cull_shutter(cam, None, SKEW) >> 31).any()  # (the tile pass had background-only tiles to take)
    script = tmp_path / "knob.py"
    script.write_text(f"""import sys
sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r})
import numpy as np, torch
import rbrt_amd, scenes
from rbrt_amd import abi
from oracle import pyoracle
cam = scenes.camera(pyoracle, 64, 48)
sc = scenes.example_scene(pyoracle, 603)
with rbrt_amd.HipScene(sc) as hs:
    hs.set_shutter({SKEW!r})
    out = torch.full((48, 64, 3), float("nan"), dtype=torch.float32, device="cuda")
    hs.render_device(cam, abi.default_opts(spp=3, seed=5), out.data_ptr())
    torch.cuda.synchronize()
    hs.check()
np.save({str(tmp_path / 'knob.npy')!r}, out.cpu().numpy())
""")
    env = dict(os.environ, RBRT_HIP_LAB="1", **KNOBS[knob])
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(bits(np.load(tmp_path / "knob.npy")), bits(got))


@pytest.mark.parametrize("mode", [0, 2], ids=["short_paths_off", "short_paths_forced"])
def test_the_same_image_with_the_short_path_stage_off_and_forced(hip, oracle, mode):
    cam = scenes.camera(oracle, 32, 24)
    sc = mixed_scene(oracle)
    opts = abi.default_opts(spp=2, seed=7, max_depth=DEPTH)
    exp, _ = NS.restated_image(cam, sc, opts, None, SKEW)
    with hip.HipScene(sc) as hs:
        hs.set_shutter(SKEW)
        hs.set_short_paths(mode)
        got, _ = render(hip, hs, cam, opts)
        if mode == 2:
            assert hs.short_masks().any()  # (the stage finished samples of this launch)
        hs.check()
    assert np.array_equal(bits(got), bits(exp))


# ---- the tile pass ---------------------------------------------------------------------------------------------------------
T_MAX = f32(1.0) - f32(2.0 ** -24)


def check_shutter_table(hip, oracle, cam, lens, travel, sc, rng, n_jitters=3):
    """test_thin_lens.check_lens_table's method with rbrt_hip_debug_primary_cull_shutter: no shutter ray of a tile -- jitter
    corners, middle and random, lens points on the rim, at the centre and random, t in {0, 0.5, 1 - 2^-24, per-pixel random} --
    may hit a sphere, enter a mesh's box or hit anything at all where the tile's word says it cannot."""
    w, h = cam.img_width_pix, cam.img_height_pix
    with hip.HipScene(sc) as hs:
        table = hs.primary_cull_shutter(cam, lens, travel)
    n_el = len(sc.spheres)
    reach = [np.zeros(table.shape, bool) for _ in range(n_el + len(sc.meshes))]
    anything = np.zeros(table.shape, bool)
    n_sets = 0
    ts = [f32(0.0), f32(0.5), T_MAX, (rng.integers(0, 1 << 24, (h, w)).astype(f32) * f32(2.0 ** -24))]
    for j, (u0, u1) in enumerate(PC.jitters(rng, w, h)):
        if j >= n_jitters:
            break
        for lx, ly in (TL.lens_points(rng, w, h) if lens is not None else [(f32(0.0), f32(0.0))]):
            for t in ts:
                rays = NS.shutter_rays(cam, lens, u0, u1, lx, ly, t, travel)
                n_sets += 1
                _, obj, _, _ = oracle.trace_rays(sc, rays, 0.001, 2000.0)
                anything |= PC.tiles_of(obj >= 0, w, h)
                for e, sp in enumerate(sc.spheres[:24]):
                    _, obj, _, _ = oracle.trace_rays(abi.SceneData(spheres=[sp]), rays, 0.001, 2000.0)
                    reach[e] |= PC.tiles_of(obj >= 0, w, h)
                for m, md in enumerate(sc.meshes[:7]):
                    reach[n_el + m] |= PC.tiles_of(PC.bbox_gate(md.bbox_lo.astype(f32), md.bbox_hi.astype(f32), rays), w, h)
    for e in range(min(n_el, 24)):
        bad = reach[e] & (((table >> e) & 1) != 0)
        assert not bad.any(), f"sphere {e}: culled in tiles {np.argwhere(bad)[:5].tolist()} that a shutter ray hits it from"
    for m in range(min(len(sc.meshes), 7)):
        bad = reach[n_el + m] & (((table >> (24 + m)) & 1) != 0)
        assert not bad.any(), f"mesh {m}: box culled in tiles {np.argwhere(bad)[:5].tolist()} that a shutter ray enters it from"
    bad = ((table >> 31) != 0) & anything
    assert not bad.any(), f"background-only tiles {np.argwhere(bad)[:5].tolist()} have a shutter ray that hits something"
    return table, n_sets


def _travel(rng, lo=1e-4, hi=100.0):
    return tuple(float(f32(v)) for v in PC._log_uniform(rng, lo, hi) * PC._unit(rng))


@pytest.mark.parametrize("name", list(PC.CAMERAS))
@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
def test_no_shutter_ray_passes_a_culled_test(hip, oracle, name, lensed):
    rng = np.random.default_rng(zlib.crc32(f"shutter{name}{lensed}".encode()))
    over = PC.CAMERAS[name]
    cam, lens = TL.lens_camera(oracle, 64, 48, 7.0, 15.0, **over)
    travel = _travel(rng, 1e-3, 1.0)
    table, _ = check_shutter_table(hip, oracle, cam, lens if lensed else None, travel, scenes.example_scene(oracle, 603), rng, n_jitters=2)
    # a zero travel culls what the camera without a shutter culls: the margins grow by a rounding term only
    with hip.HipScene(scenes.example_scene(oracle, 603)) as hs:
        zero = hs.primary_cull_shutter(cam, lens if lensed else None, (0.0, 0.0, 0.0))
        base = hs.primary_cull_lens(cam, lens) if lensed else hs.primary_cull(cam)
    assert not (zero & ~base).any()


@pytest.mark.parametrize("k", range(24))
def test_fuzzed_cameras_no_shutter_ray_passes_a_culled_test(hip, oracle, k):
    """The random scenes and cameras of test_primary_cull; travels log-uniform from 1e-4 to 100 units in random directions,
    every other case with a lens."""
    rng = np.random.default_rng(73000 + k)
    sc = PC.fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 65)), int(rng.integers(9, 49))
    cam = PC.fuzz_camera(oracle, rng, sc, w, h)
    lens = None
    if k % 2:
        right = np.array(list(cam.right), np.float64)
        fwd = np.cross(np.array(list(cam.up), np.float64), right)
        fwd = fwd / np.linalg.norm(fwd)
        v = np.cross(right, fwd)
        r = PC._log_uniform(rng, 0.1, 200.0) / 2000.0
        lens = (tuple(r * right), tuple(r * v / np.linalg.norm(v)), float(f32(PC._log_uniform(rng, 1.0, 1000.0))))
    travel = _travel(rng)
    table, n_sets = check_shutter_table(hip, oracle, cam, lens, travel, sc, rng, n_jitters=2)
    print(f"fuzz {k}: {w}x{h} |travel| {np.linalg.norm(travel):.3g} lens {lens is not None}: {n_sets} ray sets, "
          f"{int(np.count_nonzero(table))} tiles with bits, {int(np.count_nonzero(table >> 31))} background-only")


def test_the_shutter_keeps_the_background_only_tiles_of_the_bench_frame(hip, oracle):
    """Config 2's scene and camera at full size, the tile pass alone, with a travel of (0.002, 0, 0): at least 0.9 times the
    pinhole's background-only tiles (the lens test's own condition)."""
    cam = scenes.camera(oracle, 1024, 768)
    sc = scenes.example_scene(oracle, 3000)
    with hip.HipScene(sc) as hs:
        pin = int(np.count_nonzero(hs.primary_cull(cam) >> 31))
        shut = int(np.count_nonzero(hs.primary_cull_shutter(cam, None, (0.002, 0.0, 0.0)) >> 31))
    print(f"background-only tiles: pinhole {pin}, shutter {shut} of {128 * 96}")
    assert pin > 0 and shut >= 0.9 * pin, (pin, shut)


# ---- the C ABI's refusals ---------------------------------------------------------------------------------------------------
def test_refusals_through_the_c_abi(hip, oracle):
    lib = abi.load_hip()
    sh = abi.Shutter()
    assert lib.rbrt_hip_scene_set_shutter(None, C.byref(sh)) == abi.RBRT_ERR_INVALID_ARG
    assert lib.rbrt_hip_scene_set_shutter(None, None) == abi.RBRT_ERR_INVALID_ARG
    cam = scenes.camera(oracle, 16, 8)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))
    opts = abi.default_opts(spp=1, seed=1)
    with hip.HipScene(sc) as hs:
        hs.set_shutter(SKEW)
        kept, _ = render(hip, hs, cam, opts)
        for bad in ((float("nan"), 0.0, 0.0), (0.0, float("inf"), 0.0), (0.0, 0.0, -float("inf"))):
            with pytest.raises(abi.RbrtError) as e:
                hs.set_shutter(bad)
            assert e.value.code == abi.RBRT_ERR_INVALID_ARG and "travel" in str(e.value)
            with pytest.raises(abi.RbrtError) as e:
                hs.primary_cull_shutter(cam, None, bad)
            assert e.value.code == abi.RBRT_ERR_INVALID_ARG
        with pytest.raises(abi.RbrtError) as e:
            hs.set_shutter(SKEW, reserved=1)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG and "reserved" in str(e.value)
        again, _ = render(hip, hs, cam, opts)  # (a refused call leaves the handle's shutter as it was)
        assert np.array_equal(bits(again), bits(kept))
        hs.set_shutter(None)
        plain, _ = render(hip, hs, cam, opts)
        assert np.array_equal(bits(plain), bits(oracle.render(cam, sc, opts)[0]))


# ---- the C++ host ----------------------------------------------------------------------------------------------------------
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "shutter" / "shutter_spheres.yaml"
W, H = 32, 24


def _travel_of(report):
    """The report's shutter_travel (%.9g: it reads back as the float32 it was)."""
    return [float(f32(v)) for v in json.loads(Path(report).read_text())["shutter_travel"]]


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _cli(tmp_path, name, *args, env=None, cfg=CFG):
    out = tmp_path / f"{name}.png"
    r = subprocess.run([str(EXE), "-c", str(cfg), "-t", str(out), "--height", str(H), "-w", str(W), *args], capture_output=True,
                       text=True, timeout=300, env=env)
    return r, out


def _python_image(hip, hs, travel, spp=4, seed=1, cam=None):
    with hip.HipScene(hs) as dev:
        dev.set_shutter(travel)
        return render(hip, dev, cam or hs.camera, abi.default_opts(spp=spp, seed=seed))


def test_cli_yaml_key_and_flag_give_the_python_image(hip, tmp_path):
    hs = abi.HostScene(CFG, H, W)
    assert hs.shutter_travel == (float(f32(0.6)), 0.0, 0.0)
    _, exp8 = _python_image(hip, hs, hs.shutter_travel)
    _, pin8 = _python_image(hip, hs, None)
    assert not np.array_equal(exp8, pin8)
    rep = tmp_path / "yaml.json"
    r, out = _cli(tmp_path, "yaml", "-s", "4", "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), exp8)
    assert _travel_of(rep) == [float(f32(0.6)), 0.0, 0.0]
    # --shutter-travel overrides the key; on a copy of the scene without the key it is the whole shutter
    _, skew8 = _python_image(hip, hs, SKEW)
    rep = tmp_path / "flag.json"
    r, out = _cli(tmp_path, "flag", "-s", "4", "--shutter-travel", "0.3,-0.2,0.1", "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), skew8)
    assert _travel_of(rep) == [float(f32(v)) for v in SKEW]
    bare = tmp_path / "bare.yaml"
    bare.write_text("".join(line + "\n" for line in CFG.read_text().splitlines() if "camera_shutter_travel" not in line))
    rep = tmp_path / "bare.json"
    r, out = _cli(tmp_path, "bare", "-s", "4", "--report", str(rep), cfg=bare)
    assert r.returncode == 0 and np.array_equal(_png(out), pin8) and "shutter_travel" not in json.loads(rep.read_text())
    r, out = _cli(tmp_path, "bare_flag", "-s", "4", "--shutter-travel", "0.3,-0.2,0.1", cfg=bare)
    assert r.returncode == 0 and np.array_equal(_png(out), skew8)


def test_cli_three_ranks_give_the_one_rank_image(hip, tmp_path):
    r1, out1 = _cli(tmp_path, "g1", "-s", "3", "--gpus", "1")
    r3, out3 = _cli(tmp_path, "g3", "-s", "3", "--gpus", "3", "--oversubscribe")
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr[-1000:], r3.stderr[-1000:])
    assert np.array_equal(_png(out1), _png(out3))
    hs = abi.HostScene(CFG, H, W)
    assert np.array_equal(_png(out1), _python_image(hip, hs, hs.shutter_travel, spp=3)[1])


def test_cli_frames_with_a_shutter(hip, tmp_path):
    """--frames 3 --camera-step ... --shutter 0.5 writes its files, and the last frame equals the same library calls
    (test_temporal_gpu's replay) on a handle whose shutter is 0.5 * step computed in float32, frame k opening at k * step."""
    import torch
    import test_temporal_gpu as TG
    w, h, n, fs, frames, seed = W, H, 4, 3, 3, 3
    step = (0.25, 0.0, -0.125)
    pfm, rep = tmp_path / "out.pfm", tmp_path / "frames.json"
    r, out = _cli(tmp_path, "frames", "-s", str(n), "--seed", str(seed), "--feature-samples", str(fs), "--frames", str(frames), "--camera-step",
                  ",".join(str(v) for v in step), "--shutter", "0.5", "--radiance", str(pfm), "--report", str(rep))
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.exists() and pfm.exists()
    travel = tuple(float(f32(0.5) * f32(v)) for v in step)
    js = json.loads(rep.read_text())
    assert _travel_of(rep) == list(travel) and js["frames"] == frames
    hsn = abi.HostScene(CFG, h, w)
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    ha, hb, nor, dep, cov, ol, rad = new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w), new(h, w), new(h, w), new(h, w, 3)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    two = [torch.zeros((hip.temporal_history_bytes(w, h),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    with hip.HipScene(hsn) as hs:
        hs.set_shutter(travel)
        prev = None
        for k in range(frames):
            cam = type(hsn.camera).from_buffer_copy(hsn.camera)
            for c in range(3):
                shift = f32(k) * f32(step[c])
                cam.position[c] = f32(hsn.camera.position[c]) + shift
                cam.img_center_point[c] = f32(hsn.camera.img_center_point[c]) + shift
            o = abi.default_opts(spp=n, seed=seed + k)
            assert hs.render_adaptive(cam, o, 0.0, n, n)["rounds"] == 1
            hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
            hs.render_features(cam, o, fs, None, nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, prev,
                                    two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr())
            torch.cuda.synchronize()
            prev = cam
        hs.check()
    wa = torch.full((h, w), float(f32((n + 1) // 2) * (f32(1) / f32(n))), dtype=torch.float32, device="cuda")
    hip.denoise_halves(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), w, h, rad.data_ptr(), rgb.data_ptr(), window_radius=0)
    torch.cuda.synchronize()
    assert TG.same(TG.read_pfm(pfm), rad.cpu().numpy())
    assert np.array_equal(_png(out), rgb.cpu().numpy())


def test_cli_checkpoint_resumes_only_with_the_same_shutter(hip, tmp_path):
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
    assert np.array_equal(_png(out), full8)  # (passes of 3 samples with the shutter are the one render of 9)
    r, _ = _cli(tmp_path, "b", *args, "--shutter-travel", "0.5,0,0", env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, "b", *args)  # the YAML's 0.6 units: the 0.5-unit checkpoint is not resumed
    assert r.returncode == 0 and "does not match this render" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(_png(out), full8)


def test_cli_adaptive_features_and_upscale_take_the_shutter(hip, tmp_path):
    """The shutter is the handle's: the adaptive path, the feature buffers and the upsampled render read it from there. Each
    run ends well and differs from the same run on the scene without the key."""
    bare = tmp_path / "bare.yaml"
    bare.write_text("".join(line + "\n" for line in CFG.read_text().splitlines() if "camera_shutter_travel" not in line))
    for name, flags in (("adaptive", ["-s", "8", "--adaptive", "0", "--min-samples", "4", "--adaptive-step", "4"]), ("upscale", ["-s", "4", "--upscale", "2"])):
        r, out = _cli(tmp_path, name, *flags)
        rb, outb = _cli(tmp_path, name + "_bare", *flags, cfg=bare)
        assert r.returncode == 0 and rb.returncode == 0, (name, r.stderr[-1000:], rb.stderr[-1000:])
        assert not np.array_equal(_png(out), _png(outb)), name
    hs = abi.HostScene(CFG, H, W)
    r, out = _cli(tmp_path, "adaptive0", "-s", "8", "--adaptive", "0", "--min-samples", "4", "--adaptive-step", "4")
    assert np.array_equal(_png(out), _python_image(hip, hs, hs.shutter_travel, spp=8)[1])  # (threshold 0 is the plain render)
    pre = tmp_path / "feat"
    r, _ = _cli(tmp_path, "features", "-s", "2", "--features", str(pre))
    rb, _ = _cli(tmp_path, "features_bare", "-s", "2", "--features", str(tmp_path / "featb"), cfg=bare)
    assert r.returncode == 0 and rb.returncode == 0, (r.stderr[-1000:], rb.stderr[-1000:])
    for plane in ("albedo", "normal", "depth", "coverage"):
        assert (tmp_path / f"feat.{plane}.pfm").exists(), plane
    assert (tmp_path / "feat.depth.pfm").read_bytes() != (tmp_path / "featb.depth.pfm").read_bytes()  # (the depths move with the origin)
