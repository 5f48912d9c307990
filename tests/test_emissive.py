"""Emissive materials (RBRT_MAT_EMISSIVE) and the constant background (RBRT_FLAG_CONSTANT_BACKGROUND) on the GPU.

The expected images come from `colorize_emissive` below, a restatement on top of the numpy restatement of the reference
(np_reference.py): an emissive closest hit returns its radiance L at every depth, before the depth check, without a
scatter and without a random draw; an escaped ray returns bg itself under the flag. Everything else is the reference's
colorize. Images are small so that the restatement stays fast."""
from __future__ import annotations

import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_reference as R
import scenes
import test_np_reference as T
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
W, H = 32, 24
EM, L_, M_ = abi.MAT_EMISSIVE, abi.MAT_LAMBERTIAN, abi.MAT_METAL
FLAG = abi.FLAG_CONSTANT_BACKGROUND


def colorize_emissive(o, d, scene, bg, constant_bg, depth, rng, min_dist=f32(0.001), max_dist=f32(2000.0)):
    hit = R.scene_hit(scene, o, d, min_dist, max_dist)
    if hit is not None:
        kind, albedo, _ = hit["mat"]
        if kind == EM:
            return albedo.copy()  # L at any depth, no scatter, no draw
        if depth > 0:
            ok, att, no, nd = R.scatter(hit["mat"], d, hit, rng)
            if ok:
                return att * colorize_emissive(no, nd, scene, bg, constant_bg, depth - 1, rng, min_dist, max_dist)
        return R.vec(0, 0, 0)
    if constant_bg:
        return bg.copy()
    t = f32(0.5) * f32(d[1] + R.F1)
    return t * R.vec(1, 1, 1) + f32(R.F1 - t) * bg


def np_scene(sc):
    """An abi.SceneData as np_reference's scene dict: spheres, BasicTriangles, their order and meshes."""
    order = None if sc.element_order is None else [("t" if e >> 31 else "s", e & 0x7FFFFFFF) for e in sc.element_order]
    return dict(spheres=[(np.array(c, f32), f32(r), T.np_mat(m)) for c, r, m in sc.spheres],
                meshes=[T.np_mesh(m) for m in sc.meshes],
                triangles=[(np.array(c, f32), T.np_mat(m)) for c, m in sc.triangles], order=order)


def restated_image(cam, sc, opts):
    """(radiance, rgb8) of the whole image by the restatement, for a scene of abi types and render options."""
    nc, ns = T.np_cam(cam), np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & FLAG)
    rad = np.zeros((cam.img_height_pix, cam.img_width_pix, 3), f32)
    for row in range(cam.img_height_pix):
        for col in range(cam.img_width_pix):
            color = R.vec(0, 0, 0)
            for s in range(opts.spp):
                rng = R.Rng(opts.seed, row * nc["W"] + col, s)
                o, d = R.camera_ray(nc, row, col, rng)
                color = color + colorize_emissive(o, d, ns, bg, const, opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist))
            rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    rgb = np.vectorize(R.quantise, otypes=[np.uint8])(rad)
    return rad, rgb


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def lit_scene(oracle, lamp=(3.0, 2.5, 1.5), albedos=None, with_triangles=True):
    """The example spheres (lambertian, metal, dielectric), an emissive sphere, an emissive BasicTriangle between lambertian
    and metal triangles, and an emissive small mesh. `albedos`: replaces every lambertian / metal albedo."""
    sph = list(scenes.EXAMPLE_SPHERES)
    if albedos is not None:
        sph = [(c, r, abi.material(m.kind, albedos[i % len(albedos)], m.param)) for i, (c, r, m) in enumerate(sph)]
    sph.append(((3.5, 1.0, -7.0), 1.0, abi.material(EM, lamp)))
    lam = abi.material(L_, albedos[0] if albedos else (0.8, 0.3, 0.1))
    met = abi.material(M_, albedos[1] if albedos else (0.9, 0.85, 0.8), 0.02)
    tris = [
        (((-9.0, 0.0, -19.0), (3.0, 0.0, -21.0), (3.0, 7.0, -21.0)), met),
        (((-4.0, 0.3, -6.0), (-1.5, 0.4, -6.5), (-2.7, 2.6, -7.0)), abi.material(EM, (lamp[2], lamp[0], lamp[1]))),
        (((2.0, 0.02, -6.0), (5.5, 0.02, -7.0), (3.0, 0.02, -9.5)), lam),
    ]
    mesh = scenes.standin_mesh(oracle, 61, 30.0, (5.0, -1.2, -12.5), (0.0, 0.0, 0.0), abi.material(EM, (lamp[1], lamp[1], lamp[0])))
    return abi.SceneData(spheres=sph, meshes=[mesh], triangles=tris if with_triangles else [])


@pytest.mark.parametrize("bg_case,max_depth,spp", [("gradient", 50, 2), ("black", 0, 2), ("black", 1, 2), ("black", 50, 4)])
def test_bit_identical_to_the_restatement(hip, oracle, bg_case, max_depth, spp):
    cam = scenes.camera(oracle, W, H)
    sc = lit_scene(oracle)
    kw = dict(max_depth=max_depth)
    if bg_case == "black":
        kw.update(flags=FLAG, bg=(0.0, 0.0, 0.0))
    opts = abi.default_opts(spp=spp, seed=3, **kw)
    got, got8 = hip.render_scene(cam, spp, sc, seed=3, **kw)
    exp, exp8 = restated_image(cam, sc, opts)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    # the emitters are in the picture: some pixels carry more light than the sky gradient alone can give
    assert (got > 1.0).any()


def test_camera_inside_an_emitter(hip, oracle):
    L = (0.5, 0.25, 0.125)
    cam = scenes.camera(oracle, W, H)
    pos = tuple(float(x) for x in cam.position)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES) + [(pos, 2.0, abi.material(EM, L))])
    for kw in (dict(), dict(flags=FLAG, bg=(0.0, 0.0, 0.0))):
        got, _ = hip.render_scene(cam, 4, sc, seed=5, **kw)
        assert np.array_equal(bits(got), bits(np.broadcast_to(np.array(L, f32), got.shape)))


def test_doubling_every_emitter_doubles_every_radiance(hip, oracle):
    cam = scenes.camera(oracle, W, H)
    albedos = [(0.5, 0.7, 0.9), (0.9, 0.6, 0.5), (0.55, 0.85, 0.65)]
    kw = dict(flags=FLAG, bg=(0.0, 0.0, 0.0), max_depth=16)
    img1, _ = hip.render_scene(cam, 4, lit_scene(oracle, (1.5, 0.75, 3.0), albedos), seed=8, **kw)
    img2, _ = hip.render_scene(cam, 4, lit_scene(oracle, (3.0, 1.5, 6.0), albedos), seed=8, **kw)
    assert (img1 > 0).any(axis=2).mean() > 0.1  # (the sky is black: paths that escape carry nothing)
    assert np.array_equal(bits(img2), bits(img1 * f32(2.0)))


def test_background_only_tiles_under_the_flag(hip, oracle):
    import torch
    w, h = 64, 48
    cam = scenes.camera(oracle, w, h)  # the example camera: the top tiles see the sky only
    sc = lit_scene(oracle, with_triangles=False)  # (the tile pass proves tiles empty of spheres and meshes only)
    bg = (0.125, 0.0, 0.375)
    opts = abi.default_opts(spp=2, seed=4, flags=FLAG, bg=bg)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        sky = (cull >> 31) & 1
        assert sky.any() and not sky.all(), cull
        out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(cam, opts, out.data_ptr())
        torch.cuda.synchronize()
        hs.check()
        got = out.cpu().numpy()
    exp, _ = restated_image(cam, sc, opts)
    assert np.array_equal(bits(got), bits(exp))
    for ty, tx in np.argwhere(sky):
        tile = got[ty * 8:(ty + 1) * 8, tx * 8:(tx + 1) * 8]
        assert np.array_equal(bits(tile), bits(np.broadcast_to(np.array(bg, f32), tile.shape)))


def test_an_emitter_never_hit_changes_nothing(hip, oracle):
    """No ground sphere; the emitter is farther than max_dist from every point a ray can start from (the camera and the
    objects lie within 25 units of the origin), so the image is the reference's, which the C++ oracle computes."""
    cam = scenes.camera(oracle, W, H)
    far = ((0.0, 0.0, 2100.0), 5.0)
    base = list(scenes.EXAMPLE_SPHERES[1:]) + [tuple(scenes.TRIANGLES[0])]
    spheres = base[:-1]
    lit = abi.SceneData(spheres=spheres + [(*far, abi.material(EM, (100.0, 100.0, 100.0)))], triangles=[base[-1]])
    matte = abi.SceneData(spheres=spheres + [(*far, abi.material(L_, (0.5, 0.5, 0.5)))], triangles=[base[-1]])
    got, got8 = hip.render_scene(cam, 4, lit, seed=2)
    exp, exp8, _ = oracle.render(cam, matte, abi.default_opts(spp=4, seed=2))
    assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8)


def test_product_paths_agree(hip, oracle):
    import torch
    cam = scenes.camera(oracle, 64, 48)
    sc = lit_scene(oracle)
    spp = 7
    opts = abi.default_opts(spp=spp, seed=6, flags=FLAG, bg=(0.0, 0.0, 0.0))

    def img(fill=float("nan")):
        return torch.full((48, 64, 3), fill, dtype=torch.float32, device="cuda")

    with hip.HipScene(sc) as hs:
        ref = img()
        hs.render_device(cam, opts, ref.data_ptr())
        # passes 0-3, 3-7 of 7
        acc, out = img(), img()
        hs.render_pass(cam, opts, 0, 3, acc.data_ptr())
        hs.render_pass(cam, opts, 3, spp, acc.data_ptr(), out.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
        # three ranks' packed tiles, de-interleaved
        world = 3
        slot = hip.packed_pixels(64, 48, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            o = abi.default_opts(spp=spp, seed=6, flags=FLAG, bg=(0.0, 0.0, 0.0), tile_rank=r, tile_world=world)
            hs.render_device(cam, o, slots[r * slot * 3:].data_ptr())
        merged = img()
        hip.unpack_tiles(0, slots.data_ptr(), 64, 48, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        torch.cuda.synchronize()
        assert torch.equal(merged.view(torch.int32), ref.view(torch.int32))
        # pipeline depth 1 against 8
        outs = []
        for depth in (1, 8):
            hs.set_pipeline(depth)
            o = img()
            hs.render_device(cam, opts, o.data_ptr())
            torch.cuda.synchronize()
            outs.append(o)
        hs.check()
    assert torch.equal(outs[0].view(torch.int32), ref.view(torch.int32))
    assert torch.equal(outs[1].view(torch.int32), ref.view(torch.int32))
    assert (ref.cpu().numpy() > 1.0).any()


def test_debug_scatter_of_an_emitter_draws_nothing(hip):
    n = 4
    kind = [EM, EM, L_, EM]
    albedo = [(1.0, 2.0, 3.0)] * n
    param = [0.0, 1.5, 0.0, 0.3]
    in_dir = np.tile(np.array([0.0, -1.0, -1.0], f32), (n, 1))
    point = np.zeros((n, 3), f32)
    normal = np.tile(np.array([0.0, 1.0, 0.0], f32), (n, 1))
    st = np.array([[0x12345678, 0x9ABCDEF1], [1, 2], [0x12345678, 0x9ABCDEF1], [0xFFFFFFFF, 7]], np.uint32)
    _, ok, st_after = hip.debug_scatter(kind, albedo, param, in_dir, point, normal, st)
    em = np.array(kind) == EM
    assert (ok[em] == 0).all() and np.array_equal(st_after[em], st[em])
    assert ok[2] == 1 and not np.array_equal(st_after[2], st[2])  # (a lambertian does draw)


def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def test_cli_background_matches_the_python_path(hip, tmp_path):
    exe = ROOT / "rbrt_amd" / "bin" / "rbrt"
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    hs = abi.HostScene(cfg, H, W)
    _, exp8 = hip.render_scene(hs.camera, 4, hs, seed=1, flags=FLAG, bg=(0.0, 0.0, 0.0))
    outs = []
    for gpus in ("1", "2"):
        out = tmp_path / f"g{gpus}.png"
        r = subprocess.run([str(exe), "-c", str(cfg), "--background", "0,0,0", "-t", str(out), "--height", str(H), "-w", str(W),
                            "-s", "4", "--gpus", gpus, "--oversubscribe"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(_png(out))
    assert np.array_equal(outs[0], exp8) and np.array_equal(outs[1], exp8)
    # without --background the image is the gradient's, as before
    out = tmp_path / "sky.png"
    r = subprocess.run([str(exe), "-c", str(cfg), "-t", str(out), "--height", str(H), "-w", str(W), "-s", "4"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    _, sky8 = hip.render_scene(hs.camera, 4, hs, seed=1)
    assert np.array_equal(_png(out), sky8) and not np.array_equal(sky8, exp8)
