"""The numpy restatement of moving meshes (tests/np_mesh_motion.py) pinned by itself: single samples against a scalar
evaluation written with explicit loops, zero travels at phase 0 are np_motion with zero sphere travels, the one shared draw,
an exact case in which shifting the ray is shifting the vertices bit for bit, and the blur of a moving mesh edge has the width
geometry gives it. No GPU: test_mesh_motion_gpu.py compares the kernels with this restatement."""
from __future__ import annotations

import struct

import numpy as np

import np_animation as NA
import np_mesh_motion as MM
import np_motion as NM
import np_pattern
import np_reference as R
import np_smooth as S
import scenes
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32
W, H = 12, 9
SKEW = (0.3, -0.2, 0.1)
L_, M_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_EMISSIVE


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def r32(x):
    """A Python float rounded to float32 (a double product, sum or difference of two floats rounds once)."""
    return struct.unpack("f", struct.pack("f", x))[0]


def two_mesh_scene(oracle, smooth=False):
    """The example spheres, a 13-triangle stand-in in front of them and a 5-triangle one beside it (metal, lambertian)."""
    a = scenes.standin_mesh(oracle, 13, 25.0, (0.5, -0.6, -4.5), (0.0, 0.4, 0.0), abi.material(M_, (0.8, 0.7, 0.6), 0.05))
    b = S.standin_smooth(oracle, 5, 30.0, (-2.0, -0.5, -5.5), abi.material(L_, (0.7, 0.3, 0.2)), "file") if smooth else \
        scenes.standin_mesh(oracle, 5, 30.0, (-2.0, -0.5, -5.5), (0.0, 0.0, 0.0), abi.material(L_, (0.7, 0.3, 0.2)))
    return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES), meshes=[a, b])


MESH_TRAVELS = np.array([(0.9, 0.1, 0.0), (-0.5, 0.0, 0.6)], f32)


def scalar_scene_hit(ns, o, d, lo, hi, mw, s):
    """The rule with explicit loops over components: elements through np_reference, every mesh from its own origin."""
    best = R.scene_hit(dict(ns, meshes=[]), o, d, lo, hi)
    closest = best["dist"] if best is not None else np.finfo(f32).max
    n_elem = len(ns["spheres"]) + len(ns.get("triangles", []))
    for m, mesh in enumerate(ns["meshes"]):
        om = np.zeros(3, f32)
        for c in range(3):
            prod = r32(float(s) * float(mw[m][c]))
            om[c] = r32(float(o[c]) - prod)
        h = R.mesh_hit(mesh, om, d, lo, hi)
        if h is None:
            continue
        _, face, dist, t, idx = h
        if not dist < closest:
            continue
        closest = dist
        p = np.zeros(3, f32)
        for c in range(3):
            p[c] = r32(float(o[c]) + r32(float(t) * float(d[c])))
        best = dict(point=p, normal=S.shading_normal(mesh, idx, om, d), dist=dist, t=t, mat=mesh["mat"], obj=n_elem + m, tri=idx)
    return best


def scalar_colorize(o, d, ns, bg, depth, rng, lo, hi, mw, s):
    hit = scalar_scene_hit(ns, o, d, lo, hi, mw, s)
    if hit is None:
        t = f32(0.5) * f32(d[1] + R.F1)
        return t * R.vec(1, 1, 1) + f32(R.F1 - t) * bg
    if depth > 0:
        ok, att, no, nd = R.scatter(hit["mat"], d, hit, rng)
        if ok:
            return att * scalar_colorize(no, nd, ns, bg, depth - 1, rng, lo, hi, mw, s)
    return R.vec(0, 0, 0)


def test_single_samples_against_a_scalar_evaluation(oracle):
    cam = scenes.camera(oracle, W, H)
    nc = T.np_cam(cam)
    sphere_tv = np.array([(0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.0, 0.3, 0.0), (-0.2, 0.0, 0.1)], f32)
    n_mesh_hits = 0
    for smooth in (False, True):
        sc = two_mesh_scene(oracle, smooth)
        ns = np_pattern.np_scene(sc)
        for shutter, travels, phase in ((None, None, 0.0), (SKEW, None, 0.5), (None, sphere_tv, -3.0), (SKEW, sphere_tv, 40.0)):
            for row, col, seed in ((0, 0, 1), (4, 6, 2), (H - 1, W - 1, 3), (5, 3, 4), (6, 8, 5), (7, 5, 6)):
                opts = abi.default_opts(spp=1, seed=seed, max_depth=6)
                got, _ = MM.restated_image(cam, sc, opts, MESH_TRAVELS, travels=travels, phase=phase, shutter=shutter, pixels=[(row, col)])
                rng = R.Rng(seed, row * W + col, 0)
                o, d = R.camera_ray(nc, row, col, rng)
                t = float(rng.next_f32())
                if shutter is not None:
                    o = np.array([r32(float(o[c]) + r32(t * r32(shutter[c]))) for c in range(3)], f32)
                s = r32(r32(phase) + t)
                tv = sphere_tv if travels is not None else np.zeros_like(sphere_tv)
                moved = dict(ns)
                moved["spheres"] = [(np.array([r32(float(c[k]) + r32(s * float(tv[i][k]))) for k in range(3)], f32), r, m)
                                    for i, (c, r, m) in enumerate(ns["spheres"])]
                first = scalar_scene_hit(moved, o, d, f32(opts.min_dist), f32(opts.max_dist), MESH_TRAVELS, s)
                n_mesh_hits += int(first is not None and first["tri"] >= 0)
                want = scalar_colorize(o, d, moved, np.array(list(opts.bg), f32), opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist),
                                       MESH_TRAVELS, s)
                assert np.array_equal(bits(got[row, col]), bits(want)), (smooth, shutter, phase, row, col)
    assert n_mesh_hits >= 4  # (the samples do meet the meshes)


def test_zero_travels_at_phase_zero_are_np_motion_with_zero_sphere_travels(oracle):
    cam = scenes.camera(oracle, W, H)
    sc = two_mesh_scene(oracle, smooth=True)
    opts = abi.default_opts(spp=2, seed=5, max_depth=6)
    got, got8 = MM.restated_image(cam, sc, opts, np.zeros((2, 3), f32))
    exp, exp8 = NM.restated_image(cam, sc, opts, np.zeros((len(sc.spheres), 3), f32))
    assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8)
    moved, _ = MM.restated_image(cam, sc, opts, MESH_TRAVELS)
    assert not np.array_equal(bits(moved), bits(exp))  # (the travels do something here)
    # ... and with sphere travels and a phase it is np_animation's image
    tv = np.array([(0.0, 0.0, 0.0), (0.4, 0.0, 0.0), (0.0, 0.3, 0.0), (-0.2, 0.0, 0.1)], f32)
    got, _ = MM.restated_image(cam, sc, opts, np.zeros((2, 3), f32), travels=tv, phase=0.5, shutter=SKEW)
    exp, _ = NA.restated_image(cam, sc, opts, tv, 0.5, shutter=SKEW)
    assert np.array_equal(bits(got), bits(exp))


def test_the_draw_is_the_one_the_shutter_and_the_spheres_share(oracle):
    """restated_image consumes, per sample, np_motion.camera_ray_motion's draws and then colorize's: a sample whose path
    meets nothing draws exactly once more than the plain camera ray, with or without a shutter."""
    cam = scenes.camera(oracle, W, H, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0))
    nc = T.np_cam(cam)
    sc = abi.SceneData(spheres=[], meshes=[dyadic_mesh(oracle, (0.0, 0.0, 0.0), False)])
    ns = np_pattern.np_scene(sc)
    n_hits = 0
    for shutter in (None, SKEW):
        for row, col, k in ((0, 0, 0), (H - 1, W - 1, 1), (4, 6, 2)):
            a, b = R.Rng(11, row * W + col, k), R.Rng(11, row * W + col, k)
            R.camera_ray(nc, row, col, a)
            o, d, t = NM.camera_ray_motion(nc, None, shutter, row, col, b)
            assert b.draws == a.draws + 1 and bits(t) == bits(a.next_f32())
            # the time of the mesh is phase + that very t
            s = NA.spheres_time(2.0, t)
            hit = MM.scene_hit(ns, o, d, f32(0.001), f32(2000.0), [(0.25, 0.0, 0.0)], s)
            om = MM.origin_at(o, (0.25, 0.0, 0.0), f32(f32(2.0) + t))
            ref = R.mesh_hit(ns["meshes"][0], om, d, f32(0.001), f32(2000.0))
            assert (hit is None) == (ref is None)
            if hit is not None:
                n_hits += 1
                assert bits(hit["dist"]) == bits(ref[2]) and bits(hit["t"]) == bits(ref[3])
    assert n_hits >= 3


def dyadic_mesh(oracle, shift, smooth):
    """Five triangles (one more than a leaf holds) in the plane z = -4, dyadic coordinates, translated by `shift`."""
    tris = np.array([[(x, y, -4.0), (x + 4.0, y, -4.0), (x, y + 4.0, -4.0)] for x, y in
                     ((-2.0, -2.0), (-1.5, -1.0), (0.5, -2.5), (-3.0, 0.25), (1.0, 1.0))], f32)
    md = oracle.mesh_prep(tris, 1.0, (0.0, 0.0, 0.0), shift, abi.material(L_, (0.5, 0.5, 0.5)))
    if smooth:
        cn = np.array([[(0.5, 0.25, 1.0), (-0.25, 0.5, 1.0), (0.125, -0.5, 1.0)]] * len(tris), f32) * np.arange(1, 6, dtype=f32)[:, None, None]
        md = S.with_normals(md, cn)
    return md


def test_shifting_the_ray_is_shifting_the_vertices_bit_for_bit(oracle):
    """w = (2, 0, 0), s = 1, every coordinate dyadic: o - 1 * w is exact, the triangle tests of (o - w, d) against the mesh at
    rest and of (o, d) against the mesh moved by w see the same s = o - v0 exactly, and t d is exact, so t, the index, dist and
    the smooth normal agree bit for bit."""
    w = (2.0, 0.0, 0.0)
    n_hits = 0
    for smooth in (False, True):
        rest = np_pattern.np_scene(abi.SceneData(spheres=[], meshes=[dyadic_mesh(oracle, (0.0, 0.0, 0.0), smooth)]))
        moved = np_pattern.np_scene(abi.SceneData(spheres=[], meshes=[dyadic_mesh(oracle, w, smooth)]))
        for ox in np.arange(-3.0, 6.0, 0.375):
            for oy, d in ((-1.25, (0.0, 0.0, -1.0)), (0.5, (0.25, -0.125, -1.0)), (1.75, (-0.5, 0.25, -2.0))):
                o, d = np.array((ox, oy, 1.0), f32), np.array(d, f32)
                a = MM.scene_hit(rest, o, d, f32(0.001), f32(2000.0), [w], f32(1.0))
                b = S.scene_hit(moved, o, d, f32(0.001), f32(2000.0))
                assert (a is None) == (b is None), (ox, oy)
                if a is None:
                    continue
                n_hits += 1
                assert bits(a["t"]) == bits(b["t"]) and a["tri"] == b["tri"] and bits(a["dist"]) == bits(b["dist"]), (ox, oy)
                assert np.array_equal(bits(a["normal"]), bits(b["normal"])) and np.array_equal(bits(a["point"]), bits(b["point"]))
    assert n_hits >= 40


def test_the_blur_of_a_moving_mesh_edge_has_the_projected_travel_as_its_width(oracle):
    """An emissive quad (two triangles, L = 1) at depth D in front of a black constant background, its right edge on x = 0
    at the opening. It travels DELTA along +x while the camera at the origin stays. A sample with the image-plane point
    (x_s, y_s, -plane_dist) and the draw t hits it when its line meets the plane z = -D left of t DELTA: with t uniform the
    edge becomes a ramp DELTA plane_dist / (D pitch) pixels wide. A pixel's expectation p is that indicator averaged over the
    jitter square and t on a fine grid; its value is the mean of n = 192 Bernoulli(p) samples, sigma = sqrt(p (1 - p) / n);
    every pixel of the row lies within 6 sigma, as in test_np_motion.py."""
    n, w, h = 192, 24, 3
    D, f_mm = 10.0, 400.0
    cam = scenes.camera(oracle, w, h, position=(0.0, 0.0, 0.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), focal_mm=f_mm)
    nc = T.np_cam(cam)
    plane_dist = float(np.linalg.norm(nc["img_center_point"] - nc["position"]))
    pitch_x, pitch_y = 0.001 * float(nc["mm_per_pix_hor"]), 0.001 * float(nc["mm_per_pix_vert"])
    ramp_px = 7.0
    delta = ramp_px * pitch_x * D / plane_dist
    # (three strips of two triangles: the reference's scan works in chunks of eight entries and drops a shorter tail, so a mesh
    # of fewer than five triangles -- one padded leaf -- is never hit)
    quad = np.array([t for y0, y1 in ((-4, -1), (-1, 2), (2, 4))
                     for t in ([(-8, y0, -D), (0, y0, -D), (0, y1, -D)], [(-8, y0, -D), (0, y1, -D), (-8, y1, -D)])], f32)
    sc = abi.SceneData(spheres=[], meshes=[oracle.mesh_prep(quad, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), abi.material(EM, (1.0, 1.0, 1.0)))])
    opts = abi.default_opts(spp=n, seed=21, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0), max_depth=2)
    row = h // 2
    pix = [(row, c) for c in range(w)]
    got, _ = MM.restated_image(cam, sc, opts, [(delta, 0.0, 0.0)], pixels=pix)
    got = got[row, :, 0].astype(np.float64)
    u0 = ((np.arange(64) + 0.5) / 64.0)[:, None, None]
    u1 = ((np.arange(8) + 0.5) / 8.0)[None, :, None]
    t = ((np.arange(256) + 0.5) / 256.0)[None, None, :]
    worst = 0.0
    for col in range(w):
        x_s = ((col - w // 2) + u0 - 0.5) * pitch_x
        y_s = -((row - h // 2) + u1 - 0.5) * pitch_y
        x_hit = x_s * (D / plane_dist) + 0.0 * y_s  # where the line meets the plane z = -D
        p = float(np.mean(x_hit < t * delta))
        sigma = np.sqrt(p * (1.0 - p) / n)
        if sigma > 0.0:
            worst = max(worst, abs(got[col] - p) / sigma)
        assert abs(got[col] - p) <= 6.0 * sigma + 1e-12, (col, got[col], p, sigma)
    partial = int(np.count_nonzero((got > 0.0) & (got < 1.0)))
    print(f"ramp {ramp_px} px: {partial} partial pixels, worst deviation {worst:.2f} sigma")
    assert ramp_px - 1 <= partial <= ramp_px + 2  # (the ramp plus the pixels its two ends cut)
    still, _ = MM.restated_image(cam, sc, opts, [(0.0, 0.0, 0.0)], pixels=pix)
    assert int(np.count_nonzero((still[row, :, 0] > 0.0) & (still[row, :, 0] < 1.0))) <= 1  # (without a travel: a sharp edge)
