"""The numpy restatement of moving spheres (tests/np_motion.py) pinned by itself: single samples against a scalar evaluation,
an all-zero motion is a zero-travel shutter, a motion and a shutter share one draw, and the blur of a moving emitter's edge has
the width geometry gives it. No GPU: test_motion_gpu.py compares the kernels with this restatement."""
from __future__ import annotations

import struct

import numpy as np

import np_lens
import np_motion as NM
import np_pattern
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


def r32(x):
    """A Python float rounded to float32 (a double product or sum of two floats rounds once)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def small_scene():
    return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES))


def small_travels(n, seed=2):
    tv = np.random.default_rng(seed).uniform(-0.8, 0.8, (n, 3)).astype(f32)
    tv[0] = 0.0  # (the ground stays)
    return tv


def test_single_samples_against_a_scalar_evaluation(oracle):
    cam = scenes.camera(oracle, W, H)
    sc = small_scene()
    nc, ns = T.np_cam(cam), np_pattern.np_scene(sc)
    tv = small_travels(len(sc.spheres))
    for lens, shutter in ((None, None), (LENS, None), (None, SKEW), (LENS, SKEW)):
        for row, col, seed in ((0, 0, 1), (4, 6, 2), (H - 1, W - 1, 3), (5, 3, 4), (6, 8, 5)):
            opts = abi.default_opts(spp=1, seed=seed, max_depth=6)
            got, _ = NM.restated_image(cam, sc, opts, tv, lens=lens, shutter=shutter, pixels=[(row, col)])
            rng = R.Rng(seed, row * W + col, 0)
            o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
            t = float(rng.next_f32())
            if shutter is not None:
                o = np.array([r32(float(o[c]) + r32(t * r32(shutter[c]))) for c in range(3)], f32)
            moved = dict(ns)
            moved["spheres"] = [(np.array([r32(float(c[k]) + r32(t * float(tv[i][k]))) for k in range(3)], f32), r, m)
                                for i, (c, r, m) in enumerate(ns["spheres"])]
            want = np_pattern.colorize(o, d, moved, np.array(list(opts.bg), f32), False, opts.max_depth, rng)
            assert np.array_equal(bits(got[row, col]), bits(want)), (lens, shutter, row, col)


def test_an_all_zero_motion_is_a_zero_travel_shutter(oracle):
    cam = scenes.camera(oracle, W, H)
    sc = small_scene()
    opts = abi.default_opts(spp=2, seed=5, max_depth=6)
    zero = np.zeros((len(sc.spheres), 3), f32)
    for lens in (None, LENS):
        got, _ = NM.restated_image(cam, sc, opts, zero, lens=lens)
        exp, _ = NS.restated_image(cam, sc, opts, lens, (0.0, 0.0, 0.0))
        assert np.array_equal(bits(got), bits(exp))
        plain, _ = NS.restated_image(cam, sc, opts, lens, None)
        assert not np.array_equal(bits(got), bits(plain))  # (the draw counts)


def test_a_motion_and_a_shutter_consume_one_draw(oracle):
    cam = scenes.camera(oracle, W, H)
    nc = T.np_cam(cam)
    for lens in (None, LENS):
        for row, col, s in ((0, 0, 0), (H - 1, W - 1, 1), (4, 7, 2)):
            a, b, c = (R.Rng(11, row * W + col, s) for _ in range(3))
            o0, d0 = R.camera_ray(nc, row, col, a) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, a)
            o1, d1, t1 = NM.camera_ray_motion(nc, lens, None, row, col, b)
            o2, d2, t2 = NM.camera_ray_motion(nc, lens, SKEW, row, col, c)
            assert b.draws == a.draws + 1 and c.draws == a.draws + 1
            assert np.array_equal(bits(o0), bits(o1)) and np.array_equal(bits(d0), bits(d1)) and np.array_equal(bits(d0), bits(d2))
            assert bits(t1) == bits(t2) == bits(a.next_f32())  # the same draw, the one behind the ray's
            so, sd = NS.camera_ray_shutter(nc, lens, SKEW, row, col, R.Rng(11, row * W + col, s))
            assert np.array_equal(bits(o2), bits(so)) and np.array_equal(bits(d2), bits(sd))
    # ... and a shutter with an all-zero motion is the shutter's image
    sc = small_scene()
    opts = abi.default_opts(spp=2, seed=6, max_depth=5)
    got, _ = NM.restated_image(cam, sc, opts, np.zeros((len(sc.spheres), 3), f32), shutter=SKEW)
    exp, _ = NS.restated_image(cam, sc, opts, None, SKEW)
    assert np.array_equal(bits(got), bits(exp))


def test_the_blur_of_a_moving_edge_has_the_projected_travel_as_its_width(oracle):
    """An emissive sphere (L = 1, radius r) in front of a black constant background, its centre at (-r, 0, -D) at the opening:
    the line x = 0 is tangent to it at depth D. It travels DELTA along +x, perpendicular to the view, while the camera at the
    origin stays. A sample with the image-plane point (x_s, y_s, -plane_dist) and the draw t hits the sphere when the line
    through the origin and that point passes within r of (-r + t DELTA, 0, -D): with t uniform the right edge becomes a ramp
    whose width on the image plane is the projected travel, DELTA plane_dist / D, which is DELTA plane_dist / (D pitch)
    pixels. A pixel's expectation p is that indicator averaged over the jitter square and t, on a fine grid; its value is the
    mean of n = 192 Bernoulli(p) samples, sigma = sqrt(p (1 - p) / n); every pixel of the row must lie within 6 sigma (a pixel
    wholly beside the ramp: exactly 0 or 1), and the number of partial pixels is the ramp's width."""
    n, w, h = 192, 24, 3
    D, r, f_mm = 10.0, 1.0, 400.0  # (a long lens: the 24 pixels are 0.09 rad wide, the sphere's other edge is 0.2 rad away and
    # the ramp, 0.026 rad, is straight to well inside a pixel)
    cam = scenes.camera(oracle, w, h, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), focal_mm=f_mm)
    nc = T.np_cam(cam)
    plane_dist = float(np.linalg.norm(nc["img_center_point"] - nc["position"]))
    pitch_x, pitch_y = 0.001 * float(nc["mm_per_pix_hor"]), 0.001 * float(nc["mm_per_pix_vert"])
    ramp_px = 7.0
    delta = ramp_px * pitch_x * D / plane_dist
    em = abi.material(abi.MAT_EMISSIVE, (1.0, 1.0, 1.0))
    sc = abi.SceneData(spheres=[((-r, 0.0, -D), r, em)])
    opts = abi.default_opts(spp=n, seed=21, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0), max_depth=2)
    row = h // 2
    pix = [(row, c) for c in range(w)]
    got, _ = NM.restated_image(cam, sc, opts, [(delta, 0.0, 0.0)], pixels=pix)
    got = got[row, :, 0].astype(np.float64)
    # the expectation, float64: the indicator on a grid of the two jitter draws and t
    u0 = ((np.arange(64) + 0.5) / 64.0)[:, None, None]
    u1 = ((np.arange(8) + 0.5) / 8.0)[None, :, None]
    t = ((np.arange(256) + 0.5) / 256.0)[None, None, :]
    worst = 0.0
    for col in range(w):
        x_s = ((col - w // 2) + u0 - 0.5) * pitch_x
        y_s = -((row - h // 2) + u1 - 0.5) * pitch_y
        ln = np.sqrt(x_s * x_s + y_s * y_s + plane_dist * plane_dist)
        dx, dy, dz = x_s / ln, y_s / ln, -plane_dist / ln
        cx, cz = -r + t * delta, -D
        along = cx * dx + cz * dz  # (the centre's y is 0)
        dist2 = cx * cx + cz * cz - along * along
        p = float(np.mean(dist2 < r * r))
        sigma = np.sqrt(p * (1.0 - p) / n)
        if sigma > 0.0:  # (the grid itself is off by at most a cell's share of the ramp: far inside a sigma)
            worst = max(worst, abs(got[col] - p) / sigma)
        assert abs(got[col] - p) <= 6.0 * sigma + 1e-12, (col, got[col], p, sigma)
    partial = int(np.count_nonzero((got > 0.0) & (got < 1.0)))
    print(f"ramp {ramp_px} px: {partial} partial pixels, worst deviation {worst:.2f} sigma")
    assert ramp_px - 1 <= partial <= ramp_px + 2  # (the ramp plus the pixels its two ends cut)
    still, _ = NS.restated_image(cam, sc, opts, None, None, pixels=pix)
    assert int(np.count_nonzero((still[row, :, 0] > 0.0) & (still[row, :, 0] < 1.0))) <= 1  # (without a motion: a sharp edge)
