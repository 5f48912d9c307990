"""np_compare.py, the restatement the GPU is held to, pinned three ways without a GPU: against a scalar evaluation of the rule
that shares no code with it (explicit loops, clamps and the 255-step tree, one pixel at a time), by the consequences the header
states, and against a float64 evaluation through scipy."""
from __future__ import annotations

import struct

import numpy as np
import pytest

import compare_cases as CC
import np_compare as NC

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


# ---- 1. a scalar evaluation ------------------------------------------------------------------------------------------------------
G = [f32(t) for t in ("0.00102838012", "0.00759875821", "0.0360007733", "0.109360687", "0.213005543", "0.266011715", "0.213005543", "0.109360687",
                      "0.0360007733", "0.00759875821", "0.00102838012")]
BIG = f32(3.4028235e38)


def s_fin(x):
    return bool(x <= BIG) and bool(x >= -BIG)


def s_tone(c):
    y = ((f32(0.2126) * c[0]) + (f32(0.7152) * c[1])) + (f32(0.0722) * c[2])
    p = y if (s_fin(y) and y > f32(0)) else f32(0)
    return p / (f32(1.0) + p)


def s_tree(v):
    v = list(v)
    assert len(v) == 256
    steps, s = 0, 1
    while s <= 128:
        for i in range(0, 256, 2 * s):
            v[i] = v[i] + v[i + s]
            steps += 1
        s *= 2
    assert steps == 255
    return v[0]


def s_ordered_sum(values, W, H):
    """values: {(y, x): float} of the pixels inside the image -> the rule's sum, as a Python float (an IEEE double)."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    tiles = []
    for j in range(ty * tx):
        y0, x0 = (j // tx) * 16, (j % tx) * 16
        tiles.append(s_tree([values.get((y0 + t // 16, x0 + t % 16), 0.0) for t in range(256)]))
    lanes = []
    for t in range(256):
        acc = 0.0
        for j in range(t, len(tiles), 256):
            acc = acc + tiles[j]
        lanes.append(acc)
    return s_tree(lanes)


def scalar_compare(X, R, eps):
    H, W, _ = X.shape
    eps = f32(eps)
    cl = lambda a, n: min(max(a, 0), n - 1)
    with np.errstate(all="ignore"):
        u = [[s_tone(X[y, x]) for x in range(W)] for y in range(H)]
        v = [[s_tone(R[y, x]) for x in range(W)] for y in range(H)]
        planes = [lambda y, x: u[y][x], lambda y, x: v[y][x], lambda y, x: u[y][x] * u[y][x], lambda y, x: v[y][x] * v[y][x], lambda y, x: u[y][x] * v[y][x]]

        def rows(m, y, x):
            acc = G[0] * m(y, cl(x - 5, W))
            for i in range(1, 11):
                acc = acc + (G[i] * m(y, cl(x + i - 5, W)))
            return acc

        def window(m, y, x):
            acc = G[0] * rows(m, cl(y - 5, H), x)
            for j in range(1, 11):
                acc = acc + (G[j] * rows(m, cl(y + j - 5, H), x))
            return acc

        se, ae, rel, ss = {}, {}, {}, {}
        rel_map, ssim_map = np.zeros((H, W), f32), np.zeros((H, W), f32)
        mx, usable, skipped = f32(0), 0, 0
        c1, c2, two = f32(0.0001), f32(0.0009), f32(2.0)
        for y in range(H):
            for x in range(W):
                mu, mv, vuu, vvv, vuv = (window(m, y, x) for m in planes)
                su, sv, suv = vuu - (mu * mu), vvv - (mv * mv), vuv - (mu * mv)
                s = (((two * (mu * mv)) + c1) * ((two * suv) + c2)) / ((((mu * mu) + (mv * mv)) + c1) * ((su + sv) + c2))
                ssim_map[y, x] = s
                ss[(y, x)] = float(s)
                if all(s_fin(c) for c in X[y, x]) and all(s_fin(c) for c in R[y, x]):
                    e = [X[y, x, c] - R[y, x, c] for c in range(3)]
                    r = R[y, x]
                    se[(y, x)] = float(((e[0] * e[0]) + (e[1] * e[1])) + (e[2] * e[2]))
                    ae[(y, x)] = float((abs(e[0]) + abs(e[1])) + abs(e[2]))
                    q = (((e[0] * e[0]) / ((r[0] * r[0]) + eps)) + ((e[1] * e[1]) / ((r[1] * r[1]) + eps))) + ((e[2] * e[2]) / ((r[2] * r[2]) + eps))
                    rel[(y, x)] = float(q)
                    rel_map[y, x] = q
                    mx = max(mx, max(max(abs(e[0]), abs(e[1])), abs(e[2])))
                    usable += 1
                else:
                    skipped += 1
        sums = [s_ordered_sum(d, W, H) for d in (se, ae, rel, ss)]
    return struct.pack("<4df2I5I", *sums, float(mx), usable, skipped, 0, 0, 0, 0, 0), rel_map, ssim_map


@pytest.mark.parametrize("w,h,kind,eps", [(1, 1, "mixed", 0.01), (3, 3, "mixed", 0.01), (1, 20, "mixed", 0.01), (19, 18, "mixed", 0.01), (19, 18, "overflow", 0.01),
                                        (19, 18, "clean", 1e-6), (3, 3, "clean", 100.0)])
def test_the_restatement_equals_a_scalar_evaluation(w, h, kind, eps):
    assert (w, h) in CC.SMALL
    c = CC.case(w, h, kind)
    result, rel_map, ssim_map = scalar_compare(c.x, c.r, eps)
    e = NC.compare(c.x, c.r, eps)
    assert e.result == result, (e.result.hex(), result.hex())
    assert same(e.rel_map, rel_map) and same(e.ssim_map, ssim_map)
    if (w, h, kind) == (19, 18, "mixed"):  # the case is more than one tile each way and has what is not finite in X and in R
        assert e.skipped >= 8 and e.usable > 300 and (~np.isfinite(c.x)).any() and (~np.isfinite(c.r)).any()


def test_the_tree_and_the_lanes_follow_the_stated_order():
    """Values whose sum depends on the order: the vectorised sum equals the scalar one at 1, 2, 289 and 513 tiles, and differs from
    numpy's own sum and from a running sum, so the order is observable."""
    rng = np.random.default_rng(3)
    for W, H in ((16, 16), (17, 16), (272, 260), (1, 8200)):
        vals = (rng.uniform(0, 1, (H, W)) * 10.0 ** rng.integers(-8, 8, (H, W))).astype(np.float64)
        got = NC.ordered_sum(vals)
        assert got == s_ordered_sum({(y, x): float(vals[y, x]) for y in range(H) for x in range(W)}, W, H), (W, H)
    running = 0.0
    for x in vals.ravel():
        running += float(x)
    assert got != running


# ---- 2. the consequences the header states -------------------------------------------------------------------------------------------
def test_an_image_against_itself_gives_exact_zeros_and_ones():
    for kind in ("clean", "mixed", "overflow"):
        for w, h in ((33, 47), (1, 40), (3, 3)):
            x = CC.case(w, h, kind).x
            e = NC.compare(x, x.copy())
            assert (e.sum_se, e.sum_ae, e.sum_rel, float(e.max_abs)) == (0.0, 0.0, 0.0, 0.0) and (e.rel_map == 0).all()
            assert (e.ssim_map == f32(1)).all() and e.sum_ssim == float(w * h), (kind, w, h)


def test_swapping_the_images_leaves_all_but_rel():
    for kind in ("clean", "mixed"):
        c = CC.case(33, 47, kind)
        a, b = NC.compare(c.x, c.r), NC.compare(c.r, c.x)
        assert same(a.se, b.se) and same(a.ae, b.ae) and same(a.mx, b.mx) and same(a.ssim_map, b.ssim_map)
        assert (a.sum_se, a.sum_ae, a.sum_ssim, a.max_abs, a.usable, a.skipped) == (b.sum_se, b.sum_ae, b.sum_ssim, b.max_abs, b.usable, b.skipped)
        assert not same(a.rel_map, b.rel_map) and a.sum_rel != b.sum_rel


def test_a_pixel_reaches_5_pixels_and_no_further():
    c = CC.case(49, 50, "clean")
    base = NC.compare(c.x, c.r).ssim_map
    for dy, dx in ((0, 1), (1, 0), (0, -1), (-1, 0)):
        for dist, reaches in ((5, True), (6, False)):
            x = c.x.copy()
            y0, x0 = 25 + dy * dist, 24 + dx * dist
            x[y0, x0] = (9.0, 9.0, 9.0)
            s = NC.compare(x, c.r).ssim_map
            assert (bits(s)[25, 24] != bits(base)[25, 24]) == reaches, (dy, dx, dist)
            changed = np.argwhere(bits(s) != bits(base))
            assert np.abs(changed - (y0, x0)).max() == 5  # the 11 x 11 window around the changed pixel, and nothing outside it
    # at the border the window is clamped: the corner pixel stands for everything beyond it
    x = c.x.copy()
    x[0, 0] = (9.0, 9.0, 9.0)
    s = NC.compare(x, c.r).ssim_map
    changed = np.argwhere(bits(s) != bits(base))
    assert changed.max() == 5 and bits(s)[5, 5] != bits(base)[5, 5]


def test_an_unusable_pixel_is_skipped_by_the_sums_and_black_in_the_ssim():
    c = CC.case(33, 47, "clean")
    base = NC.compare(c.x, c.r)
    for value, channel in ((np.nan, 0), (np.inf, 1), (-np.inf, 2)):
        for which in ("x", "r"):
            x, r = c.x.copy(), c.r.copy()
            (x if which == "x" else r)[20, 17, channel] = value
            e = NC.compare(x, r)
            assert (e.usable, e.skipped) == (base.usable - 1, 1) and e.rel_map[20, 17] == 0 and not np.signbit(e.rel_map[20, 17])
            for name in ("se", "ae"):
                kept = getattr(base, name).astype(np.float64)
                kept[20, 17] = 0.0
                assert getattr(e, f"sum_{name}") == NC.ordered_sum(kept), (name, which)
            # ... and in the SSIM it is a pixel of luminance 0
            black_x, black_r = x.copy(), r.copy()
            (black_x if which == "x" else black_r)[20, 17] = 0.0
            assert same(e.ssim_map, NC.compare(black_x, black_r).ssim_map), (value, which)
            assert not same(e.ssim_map, base.ssim_map) and e.sum_ssim != base.sum_ssim


# ---- 3. against a float64 evaluation ---------------------------------------------------------------------------------------------------
def float_images(W=64, H=48):
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    tone = 0.4 + 0.25 * np.sin(xs / 6.0) + 0.12 * np.cos(ys / 4.0)
    base = np.stack([tone * 0.9, tone, tone * 0.55], -1)
    step = np.where(xs < W / 2, 0.05, 50.0)[..., None] * np.ones(3)
    rng = np.random.default_rng(77)
    return {"noise of +-50 %": ((base * (1.0 + rng.uniform(-0.5, 0.5, base.shape))).astype(f32), base.astype(f32)),
            "smooth, 2 % noise": ((base * (1.0 + rng.normal(0.0, 0.02, base.shape))).astype(f32), base.astype(f32)),
            "HDR step 0.05 | 50": ((step * (1.0 + np.random.default_rng(1).uniform(-0.25, 0.25, step.shape))).astype(f32), step.astype(f32))}


def ssim_float64(X, R, taps, c1=1e-4, c2=9e-4):
    ndimage = pytest.importorskip("scipy.ndimage")
    X, R = X.astype(np.float64), R.astype(np.float64)

    def tone(img):
        y = 0.2126 * img[..., 0] + 0.7152 * img[..., 1] + 0.0722 * img[..., 2]
        y = np.where(np.isfinite(y) & (y > 0), y, 0.0)
        return y / (1.0 + y)

    g = np.asarray(taps, np.float64)
    blur = lambda m: ndimage.correlate1d(ndimage.correlate1d(m, g, axis=1, mode="nearest"), g, axis=0, mode="nearest")
    u, v = tone(X), tone(R)
    mu, mv = blur(u), blur(v)
    su, sv, suv = blur(u * u) - mu * mu, blur(v * v) - mv * mv, blur(u * v) - mu * mv
    return ((2.0 * mu * mv + c1) * (2.0 * suv + c2)) / ((mu * mu + mv * mv + c1) * (su + sv + c2))


MEASURED = {"noise of +-50 %": 3.3e-5, "smooth, 2 % noise": 6.7e-5, "HDR step 0.05 | 50": 4.3e-4}


def test_the_float32_ssim_is_the_float64_ssim_within_its_rounding():
    """The largest per-pixel difference between the restatement's float32 SSIM and the same formula in float64 through
    scipy.ndimage.correlate1d(mode="nearest"), measured on a CPU at 64 x 48: 3.24e-5 on noise of +-50 %, 6.69e-5 on the smooth
    image with 2 % noise, 4.28e-4 on the HDR step (MEASURED holds them rounded up). The step is the worst because on its bright
    side u is about 0.98 and the variances are differences of numbers near 0.96 whose roundings, some 1e-7 together, stand
    against C2 = 9e-4. Each image is allowed four times its measured value, for other libm and BLAS builds, and that allowance
    stays below 2e-3. A wrong tap and a wrong constant each move the SSIM by more than 1e-2 on every one of the images, so the
    allowance tells them apart: the step's noise of +-25 % is what makes its SSIM sensitive to them at all."""
    wrong_taps = NC.TAPS.copy()
    wrong_taps[4] = wrong_taps[3]  # 0.109 where 0.213 belongs
    for name, (X, R) in float_images().items():
        allowed = 4.0 * MEASURED[name]
        assert allowed < 2e-3, name
        s32, s64 = NC.ssim_map(X, R), ssim_float64(X, R, NC.TAPS)
        worst = float(np.abs(s32.astype(np.float64) - s64).max())
        print(f"{name}: float32 against float64 {worst:.3e}, allowed {allowed:.3e}")
        assert worst <= allowed, (name, worst)
        for what, s_wrong in (("tap", NC.ssim_map(X, R, taps=wrong_taps)), ("C2", NC.ssim_map(X, R, c2=f32(0.009)))):
            moved = float(np.abs(s_wrong.astype(np.float64) - s64).max())
            print(f"    a wrong {what} moves it by {moved:.3e}")
            assert moved > 1e-2 > allowed, (name, what, moved)
        # the float64 taps sum to 1 within the literals' rounding, and the mean SSIM agrees far better than a pixel's
        assert abs(float(NC.TAPS.astype(np.float64).sum()) - 1.0) < 1e-7
        assert abs(NC.compare(X, R).sum_ssim / s64.size - float(s64.mean())) < 1e-4
