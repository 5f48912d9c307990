"""The numpy restatement of the camera shutter (tests/np_shutter.py) pinned by itself: the draw counts, the direction keeps
its bits, the origin is a product and a sum in float32, a scene of background only does not see the shutter, and the blur of
an emitter's edge has the width geometry gives it. No GPU: test_shutter_gpu.py compares the kernels with this restatement."""
from __future__ import annotations

import struct

import numpy as np

import np_lens
import np_reference as R
import np_shutter as NS
import scenes
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32
W, H = 12, 9
LENS = ((0.04, 0.0, 0.0), (0.0, 0.03, 0.01), 300.0)
SKEW = (0.3, -0.2, 0.1)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def small_scene():
    return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))


def test_a_zero_travel_is_the_lens_image_one_draw_later_not_the_shutterless_one(oracle):
    cam = scenes.camera(oracle, W, H)
    sc = small_scene()
    opts = abi.default_opts(spp=2, seed=5, max_depth=6)
    nc, ns = T.np_cam(cam), NS.np_pattern.np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    for lens in (None, LENS):
        got, _ = NS.restated_image(cam, sc, opts, lens, (0.0, 0.0, 0.0))
        exp = np.zeros((H, W, 3), f32)
        for row in range(H):
            for col in range(W):
                color = R.vec(0, 0, 0)
                for s in range(opts.spp):
                    rng = R.Rng(opts.seed, row * W + col, s)
                    o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
                    rng.next_f32()  # the shutter's draw, and nothing else
                    color = color + NS.np_pattern.colorize(o, d, ns, bg, False, opts.max_depth, rng)
                exp[row, col] = color * f32(R.F1 / f32(opts.spp))
        assert np.array_equal(bits(got), bits(exp))
        plain, _ = NS.restated_image(cam, sc, opts, lens, None)
        assert not np.array_equal(bits(got), bits(plain))  # (the draw counts: the bounces see other numbers)
        same, _ = np_lens.restated_image(cam, sc, opts, lens)
        assert np.array_equal(bits(plain), bits(same))  # (travel None is the restatement there was)


def test_directions_keep_their_bits_and_origins_are_a_product_and_a_sum(oracle):
    cam = scenes.camera(oracle, W, H)
    nc = T.np_cam(cam)
    rnd = np.random.default_rng(3)
    for travel in ((1e-6, 0.0, 0.0), SKEW, (10.0, -7.0, 3.0), tuple(rnd.normal(0, 1, 3))):
        for lens in (None, LENS):
            for row, col, s in ((0, 0, 0), (H - 1, W - 1, 1), (4, 7, 2), (2, 3, 9)):
                a, b = R.Rng(11, row * W + col, s), R.Rng(11, row * W + col, s)
                o0, d0 = R.camera_ray(nc, row, col, a) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, a)
                o1, d1 = NS.camera_ray_shutter(nc, lens, travel, row, col, b)
                assert np.array_equal(bits(d0), bits(d1))
                assert b.draws == a.draws + 1
                t = float(a.next_f32())  # the draw the shutter took
                r32 = lambda x: struct.unpack("f", struct.pack("f", x))[0]  # noqa: E731  (round a Python float to float32)
                for c in range(3):
                    want = r32(float(o0[c]) + r32(t * r32(float(travel[c]))))  # (a double product or sum of floats rounds once)
                    assert struct.pack("f", want) == struct.pack("f", float(o1[c])), (travel, lens, row, col, c)


def test_shutter_rays_are_camera_ray_shutter_for_the_same_draws(oracle):
    cam = scenes.camera(oracle, W, H)
    nc = T.np_cam(cam)
    for lens in (None, LENS):
        u0, u1, lx, ly, t = (np.zeros((H, W), f32) for _ in range(5))
        want = np.zeros((H * W, 6), f32)
        for row in range(H):
            for col in range(W):
                rng = R.Rng(4, row * W + col, 0)
                probe = R.Rng(4, row * W + col, 0)
                u0[row, col], u1[row, col] = probe.next_f32(), probe.next_f32()
                if lens is not None:
                    while True:
                        x, y = f32(R.F2 * probe.next_f32()) - R.F1, f32(R.F2 * probe.next_f32()) - R.F1
                        if f32(f32(x * x) + f32(y * y)) < R.F1:
                            break
                    lx[row, col], ly[row, col] = x, y
                t[row, col] = probe.next_f32()
                o, d = NS.camera_ray_shutter(nc, lens, SKEW, row, col, rng)
                want[row * W + col, :3], want[row * W + col, 3:] = o, d
        got = NS.shutter_rays(cam, lens, u0, u1, lx, ly, t, SKEW)
        assert np.array_equal(bits(got), bits(want))


def test_a_scene_of_background_only_does_not_see_the_shutter(oracle):
    cam = scenes.camera(oracle, W, H)
    empty = abi.SceneData(spheres=[])
    for lens in (None, LENS):
        for kw in (dict(), dict(flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.25, 0.5, 0.125))):
            opts = abi.default_opts(spp=2, seed=9, **kw)
            plain, _ = NS.restated_image(cam, empty, opts, lens, None)
            for travel in ((0.0, 0.0, 0.0), SKEW, (1e4, -3e3, 77.0)):
                got, _ = NS.restated_image(cam, empty, opts, lens, travel)
                assert np.array_equal(bits(got), bits(plain))
            if kw:
                assert np.array_equal(bits(plain), bits(np.broadcast_to(np.array(kw["bg"], f32), plain.shape)))


def test_the_blur_of_an_edge_is_a_linear_ramp_of_the_geometric_width(oracle):
    """An emitter (L = 1) fills the half plane x < 0 at distance D in front of a black constant background; the camera at the
    origin looks down -z and travels DELTA along +x, perpendicular to the view and to the edge. The ray of a sample with
    image-plane coordinate x_s (scene units, plane_dist in front of the position) and shutter draw t meets the emitter's
    plane at x = t DELTA + D x_s / plane_dist, and hits it when that is negative: with t uniform the coverage at x_s is
    clamp(-D x_s / (plane_dist DELTA), 0, 1), a linear ramp from 1 to 0 over plane_dist DELTA / D on the image plane, which is
    DELTA plane_dist / (D pitch) pixels. A pixel's expectation p is the mean of the ramp over its width (the jitter is
    uniform); its value is the mean of n = 192 Bernoulli(p) samples, sigma = sqrt(p (1 - p) / n); every pixel of the row
    must lie within 6 sigma (pixels wholly beside the ramp: exactly 0 or 1)."""
    n, w, h = 192, 24, 3
    D, f_mm = 10.0, 50.0
    cam = scenes.camera(oracle, w, h, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), focal_mm=f_mm)
    nc = T.np_cam(cam)
    plane_dist = float(np.linalg.norm(nc["img_center_point"] - nc["position"]))
    pitch = 0.001 * float(nc["mm_per_pix_hor"])  # scene units per pixel on the image plane
    ramp_px = 7.0
    delta = ramp_px * pitch * D / plane_dist
    assert abs(delta * plane_dist / (D * pitch) - ramp_px) < 1e-9
    em = abi.material(abi.MAT_EMISSIVE, (1.0, 1.0, 1.0))
    sc = abi.SceneData(spheres=[], triangles=[(((0.0, -500.0, -D), (0.0, 500.0, -D), (-1000.0, 0.0, -D)), em)])
    opts = abi.default_opts(spp=n, seed=21, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0), max_depth=2)
    row = h // 2
    got, _ = NS.restated_image(cam, sc, opts, None, (delta, 0.0, 0.0), pixels=[(row, c) for c in range(w)])
    got = got[row, :, 0].astype(np.float64)
    # the expectation: the ramp averaged over the pixel, on a fine grid of the jitter
    u = (np.arange(4096) + 0.5) / 4096.0
    worst = 0.0
    for col in range(w):
        x_s = ((col - w // 2) + u - 0.5) * pitch
        p = float(np.mean(np.clip(-D * x_s / (plane_dist * delta), 0.0, 1.0)))
        sigma = np.sqrt(p * (1.0 - p) / n)
        worst = max(worst, abs(got[col] - p) / sigma if sigma > 0 else 0.0)
        assert abs(got[col] - p) <= 6.0 * sigma + 1e-12, (col, got[col], p, sigma)
    partial = int(np.count_nonzero((got > 0.0) & (got < 1.0)))
    print(f"ramp {ramp_px} px: {partial} partial pixels, worst deviation {worst:.2f} sigma")
    assert ramp_px - 1 <= partial <= ramp_px + 2  # (the ramp plus the pixels its two ends cut)
    plain, _ = NS.restated_image(cam, sc, opts, None, None, pixels=[(row, c) for c in range(w)])
    assert int(np.count_nonzero((plain[row, :, 0] > 0.0) & (plain[row, :, 0] < 1.0))) <= 1  # (without a shutter: a sharp edge)
