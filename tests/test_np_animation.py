"""The numpy restatement of the animation (np_animation.py) pinned from outside, without a GPU: scalar evaluations with explicit
loops that share no code with it -- the spheres' time and centre, the motion channel, the inserted step of the accumulation --
and np_temporal.accumulate itself for everything behind v; the rule's exact properties; and the one quality property: with the
moving rule the history of a sphere that advances a few pixels a frame grows by one a frame, with the plain rule it does not."""
import functools

import numpy as np
import pytest

import np_animation as NA
import np_motion as NM
import np_pattern
import np_temporal as NT
import scenes
import temporal_cases as TC
from rbrt_amd import abi

f32 = np.float32
U = 2.0 ** -24  # float32's unit roundoff


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- scalar evaluations -----------------------------------------------------------------------------------------------------------
def test_the_spheres_time_and_centre_one_operation_at_a_time():
    rng = np.random.default_rng(1)
    sc = scenes.spheres_scene()
    ns = np_pattern.np_scene(sc)
    tv = rng.uniform(-2, 2, (len(sc.spheres), 3)).astype(f32)
    for phase in (-3.0, 0.0, 0.5, 7.0, 40.0, 1.0e-3, -99.75):
        for t in rng.random(5).astype(f32):
            moved = NA.scene_at(ns, tv, phase, t)
            s = f32(f32(phase) + f32(t))
            assert bits(NA.spheres_time(phase, t)) == bits(s)
            for i, (c, r, m) in enumerate(ns["spheres"]):
                for k in range(3):
                    want = f32(f32(c[k]) + f32(s * tv[i, k]))
                    assert bits(moved["spheres"][i][0][k]) == bits(want), (phase, t, i, k)
                assert moved["spheres"][i][1] == r
    # a phase of 0 leaves the draw's bits, so the scene is np_motion's
    for t in (f32(0.0), f32(0.37), np.nextafter(f32(1.0), f32(0.0))):
        a, b = NA.scene_at(ns, tv, 0.0, t), NM.scene_at(ns, tv, t)
        assert all(np.array_equal(bits(x[0]), bits(y[0])) for x, y in zip(a["spheres"], b["spheres"]))


def test_the_motion_channel_one_sample_at_a_time():
    rng = np.random.default_rng(2)
    sc = scenes.triangle_scene()  # spheres and BasicTriangles interleaved: ids follow the element order
    tv = rng.uniform(-1, 1, (len(sc.spheres), 3)).astype(f32)
    n_obj = len(sc.element_order) + 1  # (and an id behind the elements, as a mesh has)
    P, n = 40, 5
    obj = rng.integers(-1, n_obj, (P, n + 2))
    got = NA.motion_from_hits(sc, tv, obj, n)
    inv_n = f32(f32(1.0) / f32(n))
    for p in range(P):
        for k in range(3):
            acc = f32(0.0)
            for s in range(n):
                o = int(obj[p, s])
                add = f32(0.0)
                if 0 <= o < len(sc.element_order) and not sc.element_order[o] >> 31:
                    add = tv[sc.element_order[o], k]
                acc = f32(acc + add)
            assert bits(got[p, k]) == bits(f32(acc * inv_n)), (p, k)
    assert not NA.motion_from_hits(sc, None, obj, n).any()


def moving_case(pair, w, h, seed=0):
    """A frozen case of temporal_cases with a motion buffer: c times a travel that varies over the image, some of it zero."""
    c = TC.case(pair, w, h)
    rng = np.random.default_rng(100 + seed)
    m = rng.uniform(-1.5, 1.5, (h, w, 3)).astype(f32)
    m[rng.random((h, w)) < 0.3] = 0.0
    Mv = (c.c[..., None] * m).astype(f32)
    Mv.flags.writeable = False
    return c, Mv


@pytest.mark.parametrize("pair", ["static", "drift_0.2", "turn"])
def test_the_inserted_step_one_pixel_at_a_time(pair):
    w, h = 23, 13
    c, Mv = moving_case(pair, w, h)
    d = NT.centre_rays(c.cam)  # (pinned by test_np_temporal.py)
    for step in (0.0, 1.0, -2.5):
        v = NA.point_vectors(c.z, c.c, c.cam, c.cam_prev, Mv, step)
        with np.errstate(all="ignore"):
            for row in range(h):
                for col in range(w):
                    cp = f32(c.c[row, col])
                    for k in range(3):
                        if cp > 0:
                            zbar = f32(f32(c.z[row, col]) / cp)
                            P = f32(f32(c.cam.position[k]) + f32(zbar * d[row, col, k]))
                            m = f32(f32(Mv[row, col, k]) / cp)
                            P_last = f32(P - f32(f32(step) * m))
                            want = f32(P_last - f32(c.cam_prev.position[k]))
                        else:
                            want = d[row, col, k]
                        assert bits(v[row, col, k]) == bits(want), (step, row, col, k)


@pytest.mark.parametrize("pair", list(TC.PAIRS))
def test_everything_behind_v_is_np_temporal(pair):
    """accumulate_from_v on the plain rule's v is np_temporal.accumulate, bit for bit, for every frozen camera pair and option row:
    the moving rule differs from the pinned restatement in point_vectors alone."""
    c = TC.case(pair, 37, 21)
    for p in (NT.DEFAULTS, dict(max_history=4.0, depth=0.0, normal=0.0), dict(max_history=1000.0, depth=0.5, normal=2.0)):
        ea, eb, el, _, einfo = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, **p)
        v = NA.point_vectors(c.z, c.c, c.cam, c.cam_prev)
        oa, ob, ln, info = NA.accumulate_from_v(c.A, c.B, c.N, c.c, v, c.cam, c.cam_prev, c.hist, **p)
        assert np.array_equal(bits(oa), bits(ea)) and np.array_equal(bits(ob), bits(eb)) and np.array_equal(bits(ln), bits(el)), (pair, p)
        assert np.array_equal(info.accepted, einfo.accepted) and np.array_equal(info.valid, einfo.valid)


# ---- exact properties -------------------------------------------------------------------------------------------------------------
def test_phase_0_reproduces_np_motion_bit_for_bit():
    from oracle import pyoracle
    cam = scenes.camera(pyoracle, 10, 6)
    sc = scenes.spheres_scene()
    tv = np.array([(0.0, 0.0, 0.0), (0.9, 0.0, 0.0), (-0.4, 0.3, 0.5), (0.0, 0.6, -0.7)], f32)
    opts = abi.default_opts(spp=2, seed=7, max_depth=6)
    exp, exp8 = NM.restated_image(cam, sc, opts, tv, shutter=(0.3, -0.2, 0.1))
    for phase in (0.0, -0.0):
        got, got8 = NA.restated_image(cam, sc, opts, tv, phase, shutter=(0.3, -0.2, 0.1))
        assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8)
    other, _ = NA.restated_image(cam, sc, opts, tv, 0.5, shutter=(0.3, -0.2, 0.1))
    assert not np.array_equal(bits(other), bits(exp))  # (a phase does something here)


def test_a_static_scenes_motion_buffer_is_all_plus_zero():
    from oracle import pyoracle
    cam = scenes.camera(pyoracle, 12, 8)
    sc = scenes.spheres_scene()
    _, mv = NA.features(cam, sc, abi.default_opts(spp=1, seed=3), 3, None)
    assert mv.shape == (8, 12, 3) and not bits(mv).any()  # (+0: no sign bit either)
    # an all-zero motion draws, and its buffer is +0 as well
    feat, mv0 = NA.features(cam, sc, abi.default_opts(spp=1, seed=3), 3, np.zeros((4, 3), f32))
    assert not bits(mv0).any() and feat.coverage.any()


def test_a_pixel_inside_a_moving_sphere_holds_its_travel():
    """Travel (0.25, -0.5, 0.125), n = 4: every partial sum and the product with 1 / 4 are exact."""
    from oracle import pyoracle
    cam = scenes.camera(pyoracle, 12, 8)
    travel = (0.25, -0.5, 0.125)
    sc = abi.SceneData(spheres=[((0.0, 1.0, -7.0), 3.0, abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5)))])
    feat, mv = NA.features(cam, sc, abi.default_opts(spp=1, seed=3), 4, [travel], phase=0.5)
    inside = feat.coverage == 1
    assert inside.sum() >= 10 and (feat.coverage == 0).any()
    assert np.array_equal(bits(mv[inside]), bits(np.broadcast_to(np.array(travel, f32), mv[inside].shape)))
    assert not bits(mv[feat.coverage == 0]).any()


@pytest.mark.parametrize("pair", ["static", "turn"])
def test_without_a_motion_buffer_it_is_np_temporal(pair):
    c, Mv = moving_case(pair, 37, 21)
    ea, eb, el, eh, _ = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist)
    oa, ob, ln, nxt, _ = NA.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, Mv=None, phase_step=3.0)
    assert np.array_equal(bits(oa), bits(ea)) and np.array_equal(bits(ob), bits(eb)) and np.array_equal(bits(ln), bits(el))
    assert np.array_equal(bits(NT.pack(nxt)), bits(NT.pack(eh)))
    # the first frame has nothing to look up, with a buffer or without
    fa, fb, fl, _, _ = NA.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, None, None, Mv=Mv, phase_step=1.0)
    assert np.array_equal(bits(fa), bits(c.A)) and np.array_equal(bits(fb), bits(c.B)) and (fl == 1).all()
    # ... and a motion does something: with a step the lengths differ somewhere
    _, _, lm, _, _ = NA.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, Mv=Mv, phase_step=1.0)
    assert not np.array_equal(bits(lm), bits(el))


# ---- the quality property ---------------------------------------------------------------------------------------------------------
# An emissive sphere over a constant background under the test suite's camera, which stays. Radius 2.5 at 12 units is 8 pixels
# of a 48 x 32 image; it moves 0.25 units an exposure and two exposures a frame, 1.9 pixels. Four feature samples a pixel.
Q_W, Q_H, Q_FRAMES, Q_SAMPLES, Q_SEED = 48, 32, 6, 4, 3
Q_CENTRE, Q_RADIUS, Q_TRAVEL, Q_STEP = (-3.0, 1.0, -7.0), 2.5, (0.25, 0.0, 0.0), 2.0
Q_MIN_PIXELS = 50


def quality_scene():
    return abi.SceneData(spheres=[(Q_CENTRE, Q_RADIUS, abi.material(abi.MAT_EMISSIVE, (2.0, 1.5, 0.5)))])


def quality_opts(k, spp=2):
    return abi.default_opts(spp=spp, seed=Q_SEED + k, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.1, 0.2, 0.3))


def eligible(coverage, coverage_last, info):
    """The pixels the property speaks of: the 3 x 3 neighbourhood has coverage 1 in this frame (so not on the image's border), and
    the reprojected 2 x 2 taps (info.i, info.j of the moving rule) are inside the image with coverage 1 in the last frame."""
    h, w = coverage.shape
    full = coverage == 1
    out = np.zeros_like(full)
    out[1:-1, 1:-1] = True
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            out[1:-1, 1:-1] &= full[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    out &= info.projects
    for dj in (0, 1):
        for di in (0, 1):
            qy, qx = info.j + dj, info.i + di
            inside = (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            out &= inside & (coverage_last[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)] == 1)
    return out


def length_tolerance(k):
    """How far float32 lets the length of frame k (0-based) be from k + 1 when every accepted tap's own length is within the
    tolerance of frame k - 1 of k. hl = sl / ws: the four products bw * len' round once each (u), the three additions of sl and
    the three of ws (positive terms) once each (6u), the division once (u), hl + 1 once more (u): 9u relative a frame, which
    add up over the k frames behind. Exact equality is not the rule's to give: bw * 3 is not 3 * bw's sum in float32."""
    return 9.0 * U * k * (k + 1)


def check_quality(frames):
    """frames: per frame (N, z, c, Mv) of the same static camera `cam`; the halves play no part in the lengths. Both rules run
    over the stream; -> the number of eligible pixels in the last frame."""
    from oracle import pyoracle
    cam = scenes.camera(pyoracle, Q_W, Q_H)
    hist_m = hist_p = None
    cov_last = None
    counts = []
    for k, (N, z, c, Mv) in enumerate(frames):
        A = B = np.zeros((Q_H, Q_W, 3), f32)
        _, _, len_m, hist_m, info = NA.accumulate(A, B, N, z, c, cam, cam, hist_m, Mv=Mv, phase_step=Q_STEP)
        _, _, len_p, hist_p, _ = NT.accumulate(A, B, N, z, c, cam, cam, hist_p)
        if k:
            el = eligible(c, cov_last, info)
            counts.append(int(el.sum()))
            assert el.any(), k
            off = np.abs(len_m[el].astype(np.float64) - (k + 1))
            assert (off <= length_tolerance(k)).all(), (k, float(off.max()), int((off > length_tolerance(k)).sum()))
            shorter = len_p[el] < (k + 1) - length_tolerance(k)
            assert shorter.any(), k  # the plain rule looks where the sphere no longer is
            print(f"frame {k}: {counts[-1]} eligible pixels, all of length {k + 1} under the moving rule, {int(shorter.sum())} shorter under the plain one")
        cov_last = c
    assert counts[-1] >= Q_MIN_PIXELS, counts
    return counts[-1]


@functools.lru_cache(maxsize=None)
def quality_frames():
    """The restated feature buffers of the six frames, made once (and left unchanged)."""
    from oracle import pyoracle
    cam = scenes.camera(pyoracle, Q_W, Q_H)
    out = []
    for k in range(Q_FRAMES):
        feat, mv = NA.features(cam, quality_scene(), quality_opts(k), Q_SAMPLES, [Q_TRAVEL], phase=f32(k) * f32(Q_STEP))
        for a in (feat.normal, feat.depth, feat.coverage, mv):
            a.flags.writeable = False
        out.append((feat.normal, feat.depth, feat.coverage, mv))
    return tuple(out)


def test_the_history_follows_a_moving_sphere():
    """120 eligible pixels in the last frame (frames 1 to 5: 122, 116, 118, 117, 120), every one of history length k + 1 under the
    moving rule; under the plain rule 96 of the last frame's are shorter."""
    assert check_quality(quality_frames()) == 120
