"""Pins the numpy restatement of the display transform (np_tonemap.py) to independent statements of the rule of
include/rbrt_hip.h "Display transform": the rank pick against a sorted array, the identity, the white point's meaning, the
ACES fit's shape, and what is left out of the histogram. No GPU."""
from __future__ import annotations

import numpy as np
import pytest

import np_tonemap as N

f32, u32 = np.float32, np.uint32


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def log_uniform_pixels(rng, n, lo=-20.0, hi=20.0):
    """n pixels of random chroma whose luminances are spread evenly over the exponents lo..hi."""
    chroma = rng.uniform(0.05, 1.0, (n, 3)).astype(f32)
    y = N.luminance(chroma)
    target = (2.0 ** rng.uniform(lo, hi, n)).astype(f32)
    return (chroma * (target / y)[:, None]).astype(f32)


@pytest.mark.parametrize("q", [0, 1, 500, 990, 999, 1000])
@pytest.mark.parametrize("n", [1, 2, 7, 1000, 4097])
def test_rank_pick_is_the_bin_of_the_kth_smallest_counted_luminance(n, q):
    rng = np.random.default_rng(n)
    x = log_uniform_pixels(rng, n)
    x[1::5] = 0  # not counted
    x[3::11] *= f32(-1)
    y = N.luminance(x)
    counted = np.sort(y[np.isfinite(y) & (y >= np.finfo(f32).tiny)])  # positive, normal, finite: said with values, not bits
    assert counted.size > 0
    k = ((counted.size - 1) * q) // 1000
    assert N.rank_bin(N.histogram(x), q) == int(bits(counted[k:k + 1])[0] >> 19)


def test_a_bin_is_a_sixteenth_of_an_octave_and_its_midpoint_lies_inside():
    for b in (16, 1000, 2032, 2047, 2048, 4079):
        lo = np.array([b << 19], u32).view(f32)[0]
        hi = np.array([(b + 1) << 19], u32).view(f32)[0]
        assert lo < N.bin_mid(b) < hi
    one = int(bits([1.0])[0]) >> 19
    assert int(bits([2.0])[0]) >> 19 == one + 16


@pytest.mark.parametrize("curve", [N.LINEAR])
def test_linear_with_exposure_one_is_the_identity_on_the_bits(curve):
    rng = np.random.default_rng(5)
    x = log_uniform_pixels(rng, 500)
    x[::9] *= f32(-1)
    x[::13] = 0
    x[7] = (np.inf, -np.inf, 1e-42)
    out, rgb8, ch = N.tonemap(x, curve, exposure=1.0, white=1.0)
    assert np.array_equal(bits(out), bits(x)) and ch.counted == 0 and not ch.hist.any()
    assert np.array_equal(rgb8, N.quantise(x))


def ulps(a, b):
    return abs(int(bits([a])[0]) - int(bits([b])[0]))


@pytest.mark.parametrize("w", [0.5, 1.0, 2.0, 3.7, 11.0, 1000.0, 1e-3])
def test_reinhard_maps_a_grey_of_luminance_w_to_luminance_one(w):
    w = f32(w)
    # the luminance of a grey v is v up to rounding: look for the grey whose luminance is w itself
    v = w
    for _ in range(64):
        y = N.luminance(np.array([v, v, v], f32))
        if y == w:
            break
        v = np.nextafter(v, f32(np.inf) if y < w else f32(0), dtype=f32)
    grey = np.array([[v, v, v]], f32)
    assert ulps(N.luminance(grey)[0], w) <= 1
    out = N.apply(grey, N.REINHARD, 1.0, w)
    assert ulps(N.luminance(out)[0], 1.0) <= 2, (N.luminance(out)[0], w)


def test_aces_is_monotone_and_never_nan():
    """The fit rises towards 2.51 / 2.43 like 1.0329 * (1 - 0.2308 / x'), x' = 0.6 x. Its float32 evaluation has eleven
    roundings of half an ulp each at most, so two results can be told apart only when the true values differ by more than
    5.5 ulp of 1.03 (6.6e-7). Neighbours of the grid below differ by about 0.238 * 0.00069 / x' in truth, which is more than
    that up to x' = 250: there the computed values must not decrease at all. Beyond, where the curve is flat to within the
    format, no value may lie more than 6 ulp below any earlier one."""
    grid = np.concatenate([np.linspace(0.0, 1.0, 20001), np.geomspace(1.0, 1e6, 20001)]).astype(f32)
    out = N.apply(np.repeat(grid[:, None], 3, 1), N.ACES, 1.0, 1.0)[:, 0]
    steep = grid <= 100.0
    assert steep.sum() > 26000 and (np.diff(out[steep]) >= 0).all() and out[0] >= 0
    ulp = np.spacing(f32(1.0329))
    assert (np.maximum.accumulate(out) - out <= 6 * ulp).all() and out[-1] <= f32(2.51) / f32(2.43) + 6 * ulp
    big = np.concatenate([np.geomspace(1e-30, 1e15, 50001), -np.geomspace(1e-30, 1e15, 50001), [0.0, 1e15, -1e15]]).astype(f32)
    for curve in (N.LINEAR, N.REINHARD, N.ACES):
        assert not np.isnan(N.apply(np.repeat(big[:, None], 3, 1), curve, 1.0, 1.0)).any(), curve


def test_uncounted_values_change_neither_m_nor_any_bin():
    rng = np.random.default_rng(9)
    x = log_uniform_pixels(rng, 300)
    tiny = np.finfo(f32).tiny
    extra = np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [1e-42, 1e-42, 1e-42], [tiny / 2, tiny / 2, tiny / 2], [-1, -1, -1], [-1e30, 0, 0],
                      [np.inf, 1, 1], [-np.inf, 1, 1], [np.nan, 1, 1], [np.inf, -np.inf, 0]], f32)
    assert N.counted_bins(extra).size == 0
    both = np.concatenate([extra, x, extra])
    assert np.array_equal(N.histogram(both), N.histogram(x))
    a, b = N.choose(both, exposure=0.0), N.choose(x, exposure=0.0)
    assert a.counted == b.counted == int(N.histogram(x).sum()) and a.exposure == b.exposure and a.white == b.white
    none = N.choose(extra, exposure=0.0)
    assert none.counted == 0 and none.exposure == 1 and none.white == 1 and none.l_key == 0 and none.l_white == 0
    # the edges of what is counted: the smallest normal and FLT_MAX are in, their neighbours out
    for u, inside in ((0x00800000, True), (0x007FFFFF, False), (0x7F7FFFFF, True), (0x7F800000, False)):
        y = np.array([u], u32).view(f32)
        got = ((y.view(u32) >= N.FIRST_COUNTED) & (y.view(u32) <= N.LAST_COUNTED))[0]
        assert got == inside == bool(np.isfinite(y[0]) and y[0] >= tiny)


def test_exposure_and_white_follow_the_rule():
    rng = np.random.default_rng(3)
    x = log_uniform_pixels(rng, 2000, -6, 6)
    ch = N.choose(x, exposure=0.0, key=0.18, key_permille=500, white=0.0, white_permille=990)
    h = ch.hist
    assert ch.l_key == N.bin_mid(N.rank_bin(h, 500)) and ch.l_white == N.bin_mid(N.rank_bin(h, 990))
    assert ch.exposure == f32(f32(0.18) / ch.l_key) and ch.white == f32(ch.exposure * ch.l_white)
    # the median luminance lands within a bin's width (2^(1/16)) of the key
    med = np.median(N.luminance(x)) * ch.exposure
    assert 0.18 / 1.05 < med < 0.18 * 1.05
    manual = N.choose(x, exposure=2.0, white=3.0)
    assert manual.exposure == 2 and manual.white == 3 and manual.counted == 0 and not manual.hist.any()
    half = N.choose(x, exposure=2.0, white=0.0)
    assert half.exposure == 2 and half.l_key == 0 and half.white == f32(f32(2.0) * half.l_white) and half.counted == 2000
