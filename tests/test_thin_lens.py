"""The thin lens (RBRT_FLAG_THIN_LENS) on the GPU.

Images: bit for bit against the numpy restatement (np_lens.restated_image) through every entry point, the tile pass on
and off, helper launches and the counting kernel. The tile pass: every bit the lens table sets is checked against the
oracle's routines over lens rays of the tile (jitter corners and middle, lens points on the rim, at the centre and at
random), for hand-picked and fuzzed cameras, and the lens keeps nearly all of the pinhole's background-only tiles on the
benchmark frame. Physics, independent of the restatement: the partially covered band at an emitter's silhouette is as
narrow as the pinhole's in focus and as wide as the thin-lens blur out of focus. The C++ host: YAML keys and CLI flags,
several ranks, checkpoints."""
from __future__ import annotations

import os
import subprocess
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

import np_lens
import scenes
import test_emissive as E
import test_primary_cull as PC
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
W, H = 32, 24
FLAG_BG = abi.FLAG_CONSTANT_BACKGROUND


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def lens_camera(oracle, w, h, aperture_mm, focus, **over):
    """scenes.camera with a lens derived as the host derives it (np_lens.lens_for)."""
    c = dict(scenes.CAMERA)
    c.update(over)
    cam = scenes.camera(oracle, w, h, **over)
    return cam, np_lens.lens_for(cam, c["look_at"], c["focal_mm"], aperture_mm, focus)


def mixed_scene(oracle):
    """Lambertian, metal and dielectric spheres, BasicTriangles and a small mesh."""
    mesh = scenes.standin_mesh(oracle, 61, 30.0, (4.0, -1.2, -11.0), (0.0, 0.5, 0.0), abi.material(abi.MAT_METAL, (0.7, 0.6, 0.5), 0.1))
    return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES), meshes=[mesh], triangles=list(scenes.TRIANGLES))


# ---- images --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["mixed_gradient", "lit_black"])
def test_one_shot_is_bit_identical_to_the_restatement(hip, oracle, case):
    cam, lens = lens_camera(oracle, W, H, 40.0, 9.0)
    if case == "mixed_gradient":
        sc, kw = mixed_scene(oracle), {}
    else:
        sc, kw = E.lit_scene(oracle), dict(flags=FLAG_BG, bg=(0.0, 0.0, 0.0))
    opts = abi.default_opts(spp=3, seed=7, **kw)
    got, got8 = hip.render_scene(cam, 3, sc, seed=7, lens=lens, **kw)
    exp, exp8 = np_lens.restated_image(cam, sc, opts, lens)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    pin, _ = hip.render_scene(cam, 3, sc, seed=7, **kw)
    assert not np.array_equal(bits(pin), bits(got))  # (the lens does something)


def test_an_all_zero_lens_still_draws(hip, oracle):
    """A zero lens puts every ray where the pinhole's goes, but the lens draws are made: the bounces see other numbers."""
    cam = scenes.camera(oracle, W, H)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))
    lens = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)
    got, _ = hip.render_scene(cam, 2, sc, seed=3, lens=lens)
    exp, _ = np_lens.restated_image(cam, sc, abi.default_opts(spp=2, seed=3), lens)
    pin, _ = hip.render_scene(cam, 2, sc, seed=3)
    assert np.array_equal(bits(got), bits(exp))
    assert not np.array_equal(bits(got), bits(pin))


def test_every_entry_point_gives_the_restated_image(hip, oracle):
    """render_device, render_pass in three ranges, three ranks' packed tiles unpacked, a stream of render_device calls at
    pipeline depth 4 (helper launches may join), the counting kernel: all the restatement's image."""
    import torch
    w, h, spp = 40, 32, 5
    cam, lens = lens_camera(oracle, w, h, 25.0, 10.0)
    sc = mixed_scene(oracle)
    opts = abi.default_opts(spp=spp, seed=11)
    exp, exp8 = np_lens.restated_image(cam, sc, opts, lens)

    def img(fill=float("nan")):
        return torch.full((h, w, 3), fill, dtype=torch.float32, device="cuda")

    def same(t, what):
        torch.cuda.synchronize()
        assert np.array_equal(bits(t.cpu().numpy()), bits(exp)), what

    with hip.HipScene(sc) as hs:
        out, out8 = img(), torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        hs.render_device(cam, opts, out.data_ptr(), out8.data_ptr(), lens=lens)
        same(out, "render_device")
        assert np.array_equal(out8.cpu().numpy(), exp8)
        acc, out = img(), img()
        for b, e in ((0, 2), (2, 3), (3, spp)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == spp else None, lens=lens)
        same(out, "render_pass 0-2, 2-3, 3-5")
        world = 3
        slot = hip.packed_pixels(w, h, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            o = abi.default_opts(spp=spp, seed=11, tile_rank=r, tile_world=world)
            hs.render_device(cam, o, slots[r * slot * 3:].data_ptr(), lens=lens)
        merged = img()
        hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        same(merged, "tile_world 3 + unpack")
        hs.set_pipeline(4)
        hs.set_timing(True)
        outs = [img() for _ in range(8)]
        for o in outs:
            hs.render_device(cam, opts, o.data_ptr(), lens=lens)
        for n, o in enumerate(outs):
            same(o, f"stream frame {n}")
        out = img()
        hs.render_device(cam, abi.default_opts(spp=spp, seed=11, flags=abi.FLAG_COLLECT_STATS), out.data_ptr(), lens=lens)
        same(out, "COLLECT_STATS")
        assert hs.stats()["samples"] == w * h * spp
        hs.check()


def test_the_same_image_with_the_tile_pass_off(hip, oracle, tmp_path):
    cam, lens = lens_camera(oracle, 64, 48, 30.0, 8.0)
    sc = scenes.example_scene(oracle, 603)
    got, _ = hip.render_scene(cam, 3, sc, seed=5, lens=lens)
    script = tmp_path / "off.py"
    script.write_text(f"""import sys
sys.path.insert(0, {str(ROOT)!r}); sys.path.insert(0, {str(ROOT / 'tests')!r})
import numpy as np
import rbrt_amd, scenes
from oracle import pyoracle
cam = scenes.camera(pyoracle, 64, 48)
sc = scenes.example_scene(pyoracle, 603)
lens = {tuple(lens)!r}
got, _ = rbrt_amd.render_scene(cam, 3, sc, seed=5, lens=lens)
np.save({str(tmp_path / 'off.npy')!r}, got)
""")
    env = dict(os.environ, RBRT_HIP_LAB="1", RBRT_PRIMARY_CULL="0")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    off = np.load(tmp_path / "off.npy")
    assert np.array_equal(bits(off), bits(got))
    with hip.HipScene(sc) as hs:
        assert (hs.primary_cull_lens(cam, lens) >> 31).any()  # (the tile pass had background-only tiles to take)


def test_pinhole_and_lens_frames_on_one_handle(hip, oracle):
    """Pinhole, lens, pinhole, lens focused elsewhere -- one handle, one base camera: each frame is its own camera's image
    (a tile table made for one of them and used for another would show in the background-only tiles)."""
    import torch
    w, h, spp = 64, 48, 2
    cam, lens1 = lens_camera(oracle, w, h, 60.0, 4.0)
    _, lens2 = lens_camera(oracle, w, h, 60.0, 30.0)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))
    opts = abi.default_opts(spp=spp, seed=2)
    pin = oracle.render(cam, sc, opts)[0]
    exp = [pin, np_lens.restated_image(cam, sc, opts, lens1)[0], pin, np_lens.restated_image(cam, sc, opts, lens2)[0]]
    with hip.HipScene(sc) as hs:
        assert (hs.primary_cull(cam) >> 31).any()
        for n, lens in enumerate((None, lens1, None, lens2)):
            out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
            hs.render_device(cam, opts, out.data_ptr(), lens=lens)
            torch.cuda.synchronize()
            assert np.array_equal(bits(out.cpu().numpy()), bits(exp[n])), n
        hs.check()


# ---- the tile pass -------------------------------------------------------------------------------------------------------
RIM = 1.0 - 2.0 ** -20


def _lattice(x):
    """The nearest value 2 u - 1 can take (u a multiple of 2^-24), towards zero."""
    return np.trunc(np.asarray(x, np.float64) * 2.0 ** 23) / 2.0 ** 23


def lens_points(rng, W_, H_):
    """Lens points (lx, ly): eight on the rim, the centre, and per-pixel random points of the disc."""
    for k in range(8):
        a = 2.0 * np.pi * k / 8.0 + 0.1
        yield f32(_lattice(RIM * np.cos(a))), f32(_lattice(RIM * np.sin(a)))
    yield f32(0.0), f32(0.0)
    r = np.sqrt(rng.uniform(0.0, 1.0, (H_, W_))) * RIM
    a = rng.uniform(0.0, 2.0 * np.pi, (H_, W_))
    yield _lattice(r * np.cos(a)).astype(f32), _lattice(r * np.sin(a)).astype(f32)


def check_lens_table(hip, oracle, cam, lens, sc, rng, n_jitters=5, full_scene=True):
    """PC.check_table for lens rays: every bit of rbrt_hip_debug_primary_cull_lens against the oracle's routines over the
    tile's lens rays. Returns (table, number of ray sets checked)."""
    w, h = cam.img_width_pix, cam.img_height_pix
    with hip.HipScene(sc) as hs:
        table = hs.primary_cull_lens(cam, lens)
    n_el = len(sc.spheres)
    reach = [np.zeros(table.shape, bool) for _ in range(n_el + len(sc.meshes))]
    anything = np.zeros(table.shape, bool)
    n_sets = 0
    for j, (u0, u1) in enumerate(PC.jitters(rng, w, h)):
        if j >= n_jitters:
            break
        for lx, ly in lens_points(rng, w, h):
            rays = np_lens.lens_rays(cam, lens, u0, u1, lx, ly)
            n_sets += 1
            if full_scene:
                _, obj, _, _ = oracle.trace_rays(sc, rays, 0.001, 2000.0)
                anything |= PC.tiles_of(obj >= 0, w, h)
            for e, sp in enumerate(sc.spheres[:24]):
                _, obj, _, _ = oracle.trace_rays(abi.SceneData(spheres=[sp]), rays, 0.001, 2000.0)
                reach[e] |= PC.tiles_of(obj >= 0, w, h)
            for m, md in enumerate(sc.meshes[:7]):
                reach[n_el + m] |= PC.tiles_of(PC.bbox_gate(md.bbox_lo.astype(f32), md.bbox_hi.astype(f32), rays), w, h)
    for e in range(min(n_el, 24)):
        bad = reach[e] & (((table >> e) & 1) != 0)
        assert not bad.any(), f"sphere {e}: culled in tiles {np.argwhere(bad)[:5].tolist()} that a lens ray hits it from"
    for m in range(min(len(sc.meshes), 7)):
        bad = reach[n_el + m] & (((table >> (24 + m)) & 1) != 0)
        assert not bad.any(), f"mesh {m}: box culled in tiles {np.argwhere(bad)[:5].tolist()} that a lens ray enters it from"
    if full_scene:
        bad = ((table >> 31) != 0) & anything
        assert not bad.any(), f"background-only tiles {np.argwhere(bad)[:5].tolist()} have a lens ray that hits something"
    return table, n_sets


@pytest.mark.parametrize("name", list(PC.CAMERAS))
@pytest.mark.parametrize("aperture,focus", [(7.0, 15.0), (400.0, 3.0)])
def test_no_lens_ray_passes_a_culled_test(hip, oracle, name, aperture, focus):
    rng = np.random.default_rng(zlib.crc32(f"{name}{aperture}".encode()))
    over = PC.CAMERAS[name]
    cam, lens = lens_camera(oracle, 96, 64, aperture, focus, **over)
    sc = scenes.example_scene(oracle, 603)
    table, _ = check_lens_table(hip, oracle, cam, lens, sc, rng)
    if name in ("example", "looking_up", "sideways") and aperture < 10.0:
        assert (table >> 31).any()  # (a small lens keeps the sky)


N_FUZZ_LENS = int(os.environ.get("RBRT_FUZZ_LENS_CAMERAS", "48"))


@pytest.mark.parametrize("k", range(N_FUZZ_LENS))
def test_fuzzed_lens_cameras_no_lens_ray_passes_a_culled_test(hip, oracle, k):
    """Random scenes and cameras of test_primary_cull, with a lens near the margins: apertures from 0.1 mm to 2 m, focus
    planes from a hundredth of the image plane's distance (the lens may reach the focus surface: nothing may then be
    culled) to 1000 units. Every third case also renders the image against the restatement's pixels, a few of them."""
    rng = np.random.default_rng(91000 + k)
    sc = PC.fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 97)), int(rng.integers(9, 65))
    cam = PC.fuzz_camera(oracle, rng, sc, w, h)
    right = np.array(list(cam.right), np.float64)
    fwd = np.cross(np.array(list(cam.up), np.float64), right)
    fwd = fwd / np.linalg.norm(fwd)
    plane = abs(float(np.dot(np.array(list(cam.img_center_point), np.float64) - np.array(list(cam.position), np.float64), fwd)))
    aperture = PC._log_uniform(rng, 0.1, 2000.0)
    focus = plane * PC._log_uniform(rng, 0.01, 1000.0 / max(plane, 1e-3))
    r = aperture / 2000.0
    v = np.cross(right, fwd)
    lens = (tuple(r * right), tuple(r * v / np.linalg.norm(v)), float(f32(focus / plane)))
    table, n_sets = check_lens_table(hip, oracle, cam, lens, sc, rng, n_jitters=3)
    print(f"fuzz {k}: {w}x{h} aperture {aperture:.3g} mm focus_scale {lens[2]:.3g}: {n_sets} ray sets, "
          f"{int(np.count_nonzero(table))} tiles with bits, {int(np.count_nonzero(table >> 31))} background-only")
    if k % 3 == 0:
        opts = abi.default_opts(spp=1, seed=k, max_depth=8)
        try:
            got, _ = hip.render_scene(cam, 1, sc, seed=k, max_depth=8, lens=lens)
        except abi.RbrtError as e:  # (a NaN discriminant: the reference would have panicked, sphere.rs:33)
            assert e.code == abi.RBRT_ERR_NAN
            return
        nc, ns = np_lens.T.np_cam(cam), E.np_scene(sc)
        bg = np.array(list(opts.bg), f32)
        for row, col in zip(rng.integers(0, h, 6), rng.integers(0, w, 6)):
            rgen = np_lens.R.Rng(k, int(row) * w + int(col), 0)
            o, d = np_lens.camera_ray_lens(nc, lens, int(row), int(col), rgen)
            try:
                c = E.colorize_emissive(o, d, ns, bg, False, 8, rgen)
            except np_lens.R.NanDiscriminant:
                continue
            assert np.array_equal(bits(got[row, col]), bits(c)), (k, row, col)


def test_the_lens_keeps_the_background_only_tiles_of_the_bench_frame(hip, oracle):
    """Config 2's scene and camera at full size with a 28 mm f/4 lens (7 mm) focused at 15: at least 0.9 times the pinhole's
    background-only tiles (a tile pass that simply stopped culling lens rays would keep none)."""
    cam, lens = lens_camera(oracle, 1024, 768, 7.0, 15.0)
    sc = scenes.example_scene(oracle, 3000)
    with hip.HipScene(sc) as hs:
        pin = int(np.count_nonzero(hs.primary_cull(cam) >> 31))
        lensed = int(np.count_nonzero(hs.primary_cull_lens(cam, lens) >> 31))
    print(f"background-only tiles: pinhole {pin}, lens {lensed} of {128 * 96}")
    assert pin > 0 and lensed >= 0.9 * pin, (pin, lensed)


# ---- physics ---------------------------------------------------------------------------------------------------------------
def _band(row, L):
    """Partially covered pixels (0 < value < L) on each side of the middle of a row through an emitter's silhouette."""
    part = (row > 0.0) & (row < L)
    mid = len(row) // 2
    return int(np.count_nonzero(part[:mid])), int(np.count_nonzero(part[mid:]))


def test_defocus_blur_has_the_thin_lens_width(hip, oracle):
    """An emitter (L = 1) at distance S in front of a black background: a pixel is the fraction of its rays that hit it.
    Focused on the sphere the band of partial pixels at the silhouette is the pinhole's (at most 2 px); focused at 3 S its
    width is the thin-lens blur A |S - D| / D at the sphere, through f / S onto the sensor, plus the pixel's own width."""
    import torch
    S, R_, f_mm, w, h, spp = 10.0, 0.5, 100.0, 128, 8, 1024
    sc = abi.SceneData(spheres=[((0.0, 0.0, -S), R_, abi.material(abi.MAT_EMISSIVE, (1.0, 1.0, 1.0)))])
    over = dict(position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), focal_mm=f_mm)
    opts = abi.default_opts(spp=spp, seed=1, flags=FLAG_BG, bg=(0.0, 0.0, 0.0), max_depth=4)

    def render(lens):
        cam = scenes.camera(oracle, w, h, **over)
        out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        with hip.HipScene(sc) as hs:
            hs.render_device(cam, opts, out.data_ptr(), lens=lens)
            torch.cuda.synchronize()
            hs.check()
        return out.cpu().numpy()[h // 2, :, 0], cam

    pin, cam = render(None)
    mm_per_pix = float(cam.mm_per_pix_hor)
    bl, br = _band(pin, 1.0)
    assert 1 <= bl <= 2 and 1 <= br <= 2, (bl, br)
    aperture = 300.0
    _, lens_focused = lens_camera(oracle, w, h, aperture, S, **over)
    row, _ = render(lens_focused)
    bl, br = _band(row, 1.0)
    assert bl <= 2 and br <= 2, (bl, br)
    D = 3.0 * S
    _, lens_far = lens_camera(oracle, w, h, aperture, D, **over)
    row, _ = render(lens_far)
    blur_px = (aperture / 1000.0) * abs(S - D) / D * (f_mm / S) / mm_per_pix  # (scene units -> mm on the sensor -> pixels)
    assert blur_px >= 6.0
    bl, br = _band(row, 1.0)
    print(f"predicted blur {blur_px:.2f} px; partial pixels {bl} left, {br} right")
    for b in (bl, br):
        assert abs(b - (blur_px + 1.0)) <= 1.5, (b, blur_px)


# ---- the C++ host ----------------------------------------------------------------------------------------------------------
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "defocus_spheres.yaml"


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def _cli(tmp_path, name, *args, env=None, cfg=CFG):
    out = tmp_path / f"{name}.png"
    r = subprocess.run([str(EXE), "-c", str(cfg), "-t", str(out), "--height", str(H), "-w", str(W), *args], capture_output=True,
                       text=True, timeout=300, env=env)
    return r, out


def test_cli_yaml_keys_and_flags_give_the_python_image(hip, tmp_path):
    hs = abi.HostScene(CFG, H, W)
    assert hs.lens is not None
    _, exp8 = hip.render_scene(hs.camera, 4, hs, seed=1, lens=hs.lens)
    _, pin8 = hip.render_scene(hs.camera, 4, hs, seed=1)
    assert not np.array_equal(exp8, pin8)
    r, out = _cli(tmp_path, "yaml", "-s", "4")
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), exp8)
    # the same lens from the flags, on a copy of the scene without the lens keys
    text = "".join(line + "\n" for line in CFG.read_text().splitlines() if "camera_aperture_mm" not in line and "camera_focus_distance" not in line)
    bare = tmp_path / "bare.yaml"
    bare.write_text(text)
    r, out = _cli(tmp_path, "flags", "-s", "4", "--aperture", "7", "--focus-distance", "10", cfg=bare)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), exp8)
    r, out = _cli(tmp_path, "pinhole", "-s", "4", "--aperture", "0")
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), pin8)
    r, _ = _cli(tmp_path, "bad", "-s", "4", "--aperture", "5", cfg=bare)
    assert r.returncode != 0 and "camera_focus_distance" in r.stderr


def test_cli_three_ranks_give_the_one_rank_image(hip, tmp_path):
    r1, out1 = _cli(tmp_path, "g1", "-s", "3", "--gpus", "1")
    r3, out3 = _cli(tmp_path, "g3", "-s", "3", "--gpus", "3", "--oversubscribe")
    assert r1.returncode == 0 and r3.returncode == 0, (r1.stderr[-1000:], r3.stderr[-1000:])
    assert np.array_equal(_png(out1), _png(out3))


def test_cli_checkpoint_resumes_only_with_the_same_lens(hip, tmp_path):
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
    assert np.array_equal(_png(out), full8)
    r, _ = _cli(tmp_path, "b", *args, "--aperture", "12", env=stop)
    assert r.returncode == 101 and ck.exists()
    r, out = _cli(tmp_path, "b", *args)  # the YAML's 7 mm: the 12 mm checkpoint is not resumed
    assert r.returncode == 0 and "does not match this render" in r.stdout, r.stdout[-1000:]
    assert np.array_equal(_png(out), full8)
