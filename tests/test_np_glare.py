"""np_glare.py, the restatement the GPU is compared with, pinned to statements of the rule of include/rbrt_hip.h "Glare" that do
not depend on it: conservation of an impulse's light, a constant image, an image with nothing bright, symmetry, a direct double
loop over a small image, and the smallest sizes. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import np_glare as G

f32, u32 = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def impulse(h, w, y, x, value=(64.0, 32.0, 16.0)):
    img = np.zeros((h, w, 3), f32)
    img[y, x] = value
    return img


# ---- light is moved, not added: sum(E) = n * sum(B) for an impulse far from the edges ----------------------------------------
@pytest.mark.parametrize("levels,h,w,exact", [(1, 97, 131, True), (2, 97, 131, True), (3, 200, 181, False), (4, 200, 180, False)])
@pytest.mark.parametrize("where", ["centre", "odd", "mixed"])
def test_an_interior_impulse_keeps_its_light(levels, h, w, exact, where):
    y, x = {"centre": (h // 2, w // 2), "odd": (h // 2 | 1, w // 2 | 1), "mixed": (h // 2 & ~1, (w // 2 | 1) + 2)}[where]
    img = impulse(h, w, y, x)
    b = G.bright_pass(img, 0.0)
    assert np.array_equal(bits(b), bits(img))  # T = 0: k is exactly 1
    e = G.spread_light(b, levels, 1.0)
    n, _ = G.normalisation(0.5, levels, 1.0)
    assert float(n) == levels
    got, want = float(e.astype(np.float64).sum()), float(n) * float(b.astype(np.float64).sum())
    if exact:
        assert got == want
    else:
        assert abs(got - want) <= 1e-6 * want, (got, want)
    out, _ = G.glare(img, 0.0, 0.5, levels, 1.0)
    total = out.astype(np.float64).sum()
    assert abs(total - 112.0) <= 1e-6 * 112.0  # the image's own light, 64 + 32 + 16
    assert out[y, x, 0] < 64.0 and (out[y, x + 3] > 0).all()  # ... some of which has left the pixel for its surroundings


def test_normalisation():
    n, a = G.normalisation(0.1, 1, 0.5)
    assert n == 1 and a == f32(0.1)
    n, a = G.normalisation(1.0, 4, 0.5)
    assert n == f32(1.875) and a == f32(f32(1) / f32(1.875))
    n, a = G.normalisation(0.1, 8, 0.0)
    assert n == 1 and a == f32(0.1)


def test_a_constant_image_comes_back_bit_for_bit():
    x = np.tile(np.array([0.75, 3.0, 0.5], f32), (37, 53, 1))
    b = G.bright_pass(x, 0.0)
    assert np.array_equal(bits(b), bits(x))
    e = G.spread_light(b, 5, 1.0)
    assert np.array_equal(bits(e), bits(f32(5) * x))
    out, rgb = G.glare(x, 0.0, 0.5, 5, 1.0)
    assert np.array_equal(bits(out), bits(x)) and np.array_equal(rgb, G.quantise(x))


def test_nothing_bright_is_the_identity_and_a_defect_stays_in_its_pixel():
    rng = np.random.default_rng(5)
    x = rng.uniform(0.0, 0.4, (23, 31, 3)).astype(f32)  # luminance below T = 1 everywhere
    x[3, 4] = (np.nan, 0.1, 0.1)
    x[10, 20] = (np.inf, 0.1, 0.1)
    x[11, 2] = (-np.inf, 5.0, 5.0)
    x[0, 0] = (-0.0, -0.0, -0.0)
    x[7, 7] = (1e-42, 0.0, 0.0)
    x[8, 8] = (-3.0, -3.0, -3.0)
    assert not G.bright_mask(x, 1.0).any()
    out, rgb = G.glare(x, 1.0, 1.0, 8, 1.0)
    bad = ~np.isfinite(x)
    assert np.array_equal(np.isnan(out), np.isnan(x)) and np.array_equal(out[~np.isnan(x)], x[~np.isnan(x)])  # equal as floats
    assert np.array_equal(bits(out)[~bad & (bits(x) != 0x80000000)], bits(x)[~bad & (bits(x) != 0x80000000)])
    assert (bits(out[0, 0]) == 0).all()  # -0.0f becomes +0.0f
    assert np.array_equal(rgb, G.quantise(x))
    # the same defects next to bright pixels: every pixel but the defects' own is finite
    x2 = x.copy()
    x2[5:9, 12:18] = 50.0
    out2, _ = G.glare(x2, 1.0, 0.5, 5, 1.0)
    assert np.array_equal(~np.isfinite(out2), ~np.isfinite(x2)) and (out2[4, 11] > x2[4, 11]).all()


@pytest.mark.parametrize("levels", [1, 2, 3, 5])
def test_an_even_impulses_response_is_symmetric_about_it(levels):
    """An impulse whose coordinates stay even on every level the pyramid halves them at: (64, 96) -> ... -> (2, 3) on level 5.
    REDUCE and EXPAND are mirror symmetric about such a pixel as real-number maps, but a mirrored pixel adds the same terms in
    the opposite order ((a + 6b) + c against (c + 6b) + a). With dyadic inputs one or two levels are exact, so the mirror image
    has the same bits. Deeper, every term is non-negative, so a value's relative error is at most (1 + 2^-24)^k - 1 for the k
    roundings behind it: at most 18 in a REDUCE (two passes of 4 products, 4 sums and a scale), 8 in an EXPAND, 2 for
    D + s * E; k <= 5 * 28 = 140 at five levels, and two mirrored values differ by at most twice that: 280 * 2^-24 < 2e-5."""
    h, w, y, x = 129, 193, 64, 96
    img = impulse(h, w, y, x, (8.0, 4.0, 2.0))
    e = G.spread_light(G.bright_pass(img, 0.0), levels, 0.5)
    r = 60
    win = e[y - r:y + r + 1, x - r:x + r + 1]
    assert win.max() > 0 and (win >= 0).all()
    for mirrored in (win[::-1], win[:, ::-1]):
        if levels <= 2:
            assert np.array_equal(bits(win), bits(mirrored))
        else:
            assert (np.abs(win.astype(np.float64) - mirrored) <= 2e-5 * np.maximum(win, mirrored)).all()


# ---- a direct, unvectorised statement of the rule ----------------------------------------------------------------------------
def cl(k, n):
    return min(max(k, 0), n - 1)


def five(a, b, c, d, e):
    return f32(f32(f32(f32(f32(a + f32(f32(4) * b)) + f32(f32(6) * c)) + f32(f32(4) * d)) + e) * f32(0.0625))


def loop_reduce(F):
    h, w = len(F), len(F[0])
    h2, w2 = (h + 1) // 2, (w + 1) // 2
    r = [[five(*[F[y][cl(2 * x + d, w)] for d in (-2, -1, 0, 1, 2)]) for x in range(w2)] for y in range(h)]
    return [[five(*[r[cl(2 * y + d, h)][x] for d in (-2, -1, 0, 1, 2)]) for x in range(w2)] for y in range(h2)]


def along(get, x, n):
    k = x >> 1
    if x & 1:
        return f32(f32(get(k) + get(cl(k + 1, n))) * f32(0.5))
    return f32(f32(f32(get(cl(k - 1, n)) + f32(f32(6) * get(k))) + get(cl(k + 1, n))) * f32(0.125))


def loop_expand(Gm, h, w):
    h2, w2 = len(Gm), len(Gm[0])
    r = [[along(lambda k: Gm[y][k], x, w2) for x in range(w)] for y in range(h2)]
    return [[along(lambda k: r[k][x], y, h2) for x in range(w)] for y in range(h)]


def loop_glare(X, T, i, L, s):
    """One channel image at a time would not do (the luminance joins them): X is [y][x] of 3-vectors; the pyramid runs per channel."""
    h, w = len(X), len(X[0])
    T, i, s = f32(T), f32(i), f32(s)
    B = [[[f32(0)] * 3 for _ in range(w)] for _ in range(h)]
    for y in range(h):
        for x in range(w):
            r, g, b = X[y][x]
            Y = f32(f32(f32(f32(0.2126) * r) + f32(f32(0.7152) * g)) + f32(f32(0.0722) * b))
            u = int(np.array([Y], f32).view(u32)[0])
            if 0x00800000 <= u <= 0x7F7FFFFF and Y > T:
                k = f32(f32(Y - T) / Y)
                B[y][x] = [f32(r * k), f32(g * k), f32(b * k)]
    n, p = f32(1), f32(1)
    for _ in range(2, L + 1):
        p = f32(p * s)
        n = f32(n + p)
    a = f32(i * f32(f32(1) / n))
    out = [[[None] * 3 for _ in range(w)] for _ in range(h)]
    for c in range(3):
        D = [[[B[y][x][c] for x in range(w)] for y in range(h)]]
        for _ in range(L):
            D.append(loop_reduce(D[-1]))
        Gl = D[L]
        for l in range(L - 1, 0, -1):
            hh, ww = len(D[l]), len(D[l][0])
            E = loop_expand(Gl, hh, ww)
            Gl = [[f32(D[l][y][x] + f32(s * E[y][x])) for x in range(ww)] for y in range(hh)]
        E = loop_expand(Gl, h, w)
        for y in range(h):
            for x in range(w):
                out[y][x][c] = f32(f32(X[y][x][c] - f32(i * B[y][x][c])) + f32(a * E[y][x]))
    return np.array(out, f32)


@pytest.mark.parametrize("T,i,s", [(1.0, 0.1, 1.0), (0.0, 1.0, 0.5), (0.5, 0.3, 0.0)])
def test_a_direct_double_loop_gives_the_same_bits(T, i, s):
    rng = np.random.default_rng(11)
    x = (2.0 ** rng.uniform(-4, 6, (5, 8, 3))).astype(f32)
    x[2, 3] = 0.0
    x[4, 7] = (-1.0, 9.0, 0.5)
    with np.errstate(all="ignore"):
        want = loop_glare([[list(px) for px in row] for row in x], T, i, 3, s)
    got, _ = G.glare(x, T, i, 3, s)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("h,w", [(1, 1), (1, 7), (2, 2), (3, 1), (5, 8)])
def test_the_smallest_sizes_stay_finite(h, w):
    rng = np.random.default_rng(h * 10 + w)
    x = (2.0 ** rng.uniform(-3, 8, (h, w, 3))).astype(f32)
    assert G.sizes(w, h, 8)[-1] == (1, 1)
    for s in (0.0, 0.5, 1.0):
        out, rgb = G.glare(x, 1.0, 0.1, 8, s)
        assert out.shape == x.shape and np.isfinite(out).all() and rgb.shape == x.shape
