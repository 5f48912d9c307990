"""numpy float32 restatement of the glare stage of include/rbrt_hip.h "Glare": the bright pass, REDUCE, EXPAND, the collapse,
the normalisation and the output. Every operation is a float32 numpy operation in the header's order, with .astype(f32) behind
it (numpy fuses nothing; its / is correctly rounded), so the GPU's outputs are compared with these bit for bit
(tests/test_glare_gpu.py). test_np_glare.py pins this file to statements that do not depend on it."""
from __future__ import annotations

import numpy as np

from np_tonemap import luminance, quantise  # the display transform's luminance (the same three constants, the same order)

f32 = np.float32
u32 = np.uint32
MAX_LEVELS = 8
FIRST_COUNTED, LAST_COUNTED = 0x00800000, 0x7F7FFFFF  # the positive, normal, finite floats


def image(x) -> np.ndarray:
    x = np.ascontiguousarray(x, f32)
    assert x.ndim == 3 and x.shape[2] == 3 and x.shape[0] >= 1 and x.shape[1] >= 1
    return x


def bright_mask(x, threshold) -> np.ndarray:
    y = luminance(image(x)).astype(f32)
    u = np.ascontiguousarray(y).view(u32)
    with np.errstate(all="ignore"):
        return (u >= FIRST_COUNTED) & (u <= LAST_COUNTED) & (y > f32(threshold))


def bright_pass(x, threshold) -> np.ndarray:
    """B: X_c * ((Y - T) / Y) at the bright pixels, 0 elsewhere."""
    x = image(x)
    t = f32(threshold)
    m = bright_mask(x, t)
    y = luminance(x).astype(f32)
    b = np.zeros_like(x)
    with np.errstate(all="ignore"):
        k = ((y[m] - t).astype(f32) / y[m]).astype(f32)
        b[m] = (x[m] * k[:, None]).astype(f32)
    return b


def sizes(w: int, h: int, levels: int):
    """[(W_0, H_0), ..., (W_L, H_L)]"""
    out = [(int(w), int(h))]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def _cl(k, n):
    return np.minimum(np.maximum(k, 0), n - 1)


def _reduce_axis0(f: np.ndarray) -> np.ndarray:
    """1 4 6 4 1 over 16 along axis 0, edges replicated, every second sample."""
    n = f.shape[0]
    k = 2 * np.arange((n + 1) // 2)
    t = [f[_cl(k + d, n)] for d in (-2, -1, 0, 1, 2)]
    with np.errstate(all="ignore"):
        acc = (t[0] + (f32(4) * t[1]).astype(f32)).astype(f32)
        acc = (acc + (f32(6) * t[2]).astype(f32)).astype(f32)
        acc = (acc + (f32(4) * t[3]).astype(f32)).astype(f32)
        acc = (acc + t[4]).astype(f32)
        return (acc * f32(0.0625)).astype(f32)


def reduce(f: np.ndarray) -> np.ndarray:
    """REDUCE: (h, w, 3) -> ((h + 1) // 2, (w + 1) // 2, 3). Rows first (along x), then columns."""
    r = _reduce_axis0(f.transpose(1, 0, 2)).transpose(1, 0, 2)
    return np.ascontiguousarray(_reduce_axis0(r))


def _expand_axis0(g: np.ndarray, n: int) -> np.ndarray:
    m = g.shape[0]
    assert m == (n + 1) // 2
    x = np.arange(n)
    k = x >> 1
    lo, mid, hi = g[_cl(k - 1, m)], g[k], g[_cl(k + 1, m)]
    with np.errstate(all="ignore"):
        even = (((lo + (f32(6) * mid).astype(f32)).astype(f32) + hi).astype(f32) * f32(0.125)).astype(f32)
        odd = ((mid + hi).astype(f32) * f32(0.5)).astype(f32)
    return np.where(((x & 1) == 1).reshape((-1,) + (1,) * (g.ndim - 1)), odd, even).astype(f32)


def expand(g: np.ndarray, w: int, h: int) -> np.ndarray:
    """EXPAND: (h', w', 3) -> (h, w, 3). Rows first (along x), then columns."""
    r = _expand_axis0(g.transpose(1, 0, 2), w).transpose(1, 0, 2)
    return np.ascontiguousarray(_expand_axis0(r, h))


def normalisation(intensity, levels: int, spread):
    """(n, a)"""
    i, s = f32(intensity), f32(spread)
    n, p = f32(1), f32(1)
    for _ in range(2, levels + 1):
        p = f32(p * s)
        n = f32(n + p)
    inv = f32(f32(1) / n)
    return n, f32(i * inv)


def pyramid(b: np.ndarray, levels: int):
    """[D_0 = B, D_1, ..., D_L]"""
    d = [b]
    for _ in range(levels):
        d.append(reduce(d[-1]))
    return d


def spread_light(b: np.ndarray, levels: int, spread) -> np.ndarray:
    """E: the collapse of B's pyramid, at B's size."""
    assert 1 <= levels <= MAX_LEVELS
    s = f32(spread)
    d = pyramid(b, levels)
    g = d[levels]
    with np.errstate(all="ignore"):
        for l in range(levels - 1, 0, -1):
            h, w = d[l].shape[:2]
            g = (d[l] + (s * expand(g, w, h)).astype(f32)).astype(f32)
    h, w = b.shape[:2]
    return expand(g, w, h)


def glare(x, threshold=1.0, intensity=0.1, levels=5, spread=1.0):
    """(float output, rgb8 output) of one call."""
    x = image(x)
    i = f32(intensity)
    b = bright_pass(x, threshold)
    e = spread_light(b, levels, spread)
    _, a = normalisation(intensity, levels, spread)
    with np.errstate(all="ignore"):
        out = ((x - (i * b).astype(f32)).astype(f32) + (a * e).astype(f32)).astype(f32)
    return out, quantise(out)
