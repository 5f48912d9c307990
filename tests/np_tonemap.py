"""numpy float32 restatement of the display transform of include/rbrt_hip.h "Display transform": the luminance histogram on
the float's bits, the rank pick, the exposure e, the white point w, the three curves and the quantisation. Every operation
is a float32 numpy operation in the header's order (numpy fuses nothing; its / and sqrt are correctly rounded), every count
an integer, so the GPU's outputs are compared with these bit for bit (tests/test_tonemap_gpu.py). test_np_tonemap.py pins
this file to independent statements of the same rule."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

f32 = np.float32
u32 = np.uint32
LINEAR, REINHARD, ACES = 0, 1, 2
BINS = 4096
FIRST_COUNTED, LAST_COUNTED = 0x00800000, 0x7F7FFFFF  # the positive, normal, finite floats


def pixels(x) -> np.ndarray:
    """Any array of RGB pixels as float32 (n, 3)."""
    return np.ascontiguousarray(x, f32).reshape(-1, 3)


def luminance(c: np.ndarray) -> np.ndarray:
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * c[..., 0]) + (f32(0.7152) * c[..., 1])) + (f32(0.0722) * c[..., 2])


def counted_bins(x) -> np.ndarray:
    """The bins of the counted pixels of x, in pixel order."""
    u = np.ascontiguousarray(luminance(pixels(x)), f32).view(u32)
    return (u[(u >= FIRST_COUNTED) & (u <= LAST_COUNTED)] >> 19).astype(np.int64)


def histogram(x) -> np.ndarray:
    return np.bincount(counted_bins(x), minlength=BINS).astype(u32)


def rank_bin(hist: np.ndarray, q: int) -> int:
    """b_q: the smallest bin whose prefix sum is above k = ((M - 1) * q) / 1000. M must be > 0."""
    m = int(hist.astype(np.int64).sum())
    assert m > 0 and 0 <= q <= 1000
    k = ((m - 1) * int(q)) // 1000  # (Python integers: no width to overflow)
    return int(np.searchsorted(np.cumsum(hist.astype(np.int64)), k, side="right"))


def bin_mid(b: int) -> np.float32:
    """L_q of a bin: the float whose bits are (b << 19) | (1 << 18)."""
    return np.array([(int(b) << 19) | (1 << 18)], u32).view(f32)[0]


def choose(x, exposure=1.0, key=0.18, key_permille=500, white=0.0, white_permille=990) -> SimpleNamespace:
    """What a call chooses: exposure (e), white (w), l_key, l_white, counted (M), hist -- the workspace's histogram, all zero
    when nothing is automatic -- and pixels (n)."""
    exposure, key, white = f32(exposure), f32(key), f32(white)
    auto_e, auto_w = exposure == 0, white == 0
    hist = histogram(x) if (auto_e or auto_w) else np.zeros(BINS, u32)
    m = int(hist.astype(np.int64).sum())
    l_key = bin_mid(rank_bin(hist, key_permille)) if auto_e and m > 0 else f32(0)
    l_white = bin_mid(rank_bin(hist, white_permille)) if auto_w and m > 0 else f32(0)
    with np.errstate(all="ignore"):
        e = (f32(key / l_key) if m > 0 else f32(1)) if auto_e else exposure
        w = (f32(e * l_white) if m > 0 else f32(1)) if auto_w else white
    return SimpleNamespace(exposure=f32(e), white=f32(w), l_key=f32(l_key), l_white=f32(l_white), counted=m, hist=hist,
                           pixels=pixels(x).shape[0])


def apply(x, curve: int, e, w) -> np.ndarray:
    """The float output, in x's shape."""
    x = np.ascontiguousarray(x, f32)
    e, w = f32(e), f32(w)
    with np.errstate(all="ignore"):
        c = e * x
        if curve == LINEAR:
            return c
        if curve == REINHARD:
            y = luminance(c)
            pos = y > 0  # (false for NaN)
            s = np.ones_like(y)
            s[pos] = ((f32(1) + (y / (w * w))) / (f32(1) + y))[pos]
            return c * s[..., None]
        assert curve == ACES
        v = c * f32(0.6)
        return (v * ((f32(2.51) * v) + f32(0.03))) / ((v * ((f32(2.43) * v) + f32(0.59))) + f32(0.14))


def quantise(c) -> np.ndarray:
    """(sqrt(c) * 256) as u8: the cast saturates and maps NaN to 0 (lib.rs:116-122)."""
    with np.errstate(all="ignore"):
        v = np.sqrt(np.ascontiguousarray(c, f32)) * f32(256)
    out = np.zeros(v.shape, np.uint8)
    mid = (v > 0) & (v < 255)  # (false for NaN)
    out[mid] = v[mid].astype(np.uint8)  # truncation
    out[v >= 255] = 255
    return out


def tonemap(x, curve=LINEAR, **opts):
    """(float output, rgb8 output, what choose() returned) of one call."""
    ch = choose(x, **opts)
    out = apply(x, curve, ch.exposure, ch.white)
    return out, quantise(out), ch
