"""The guided denoiser restated in numpy (include/rbrt_hip.h "Guided denoising"), written from the rule and independently of
the C++: two half images, their mix and the four feature buffers in, the filtered image out.

Everything is float32, one operation at a time (numpy never fuses), with explicit loops over the levels and the 25 taps in the
rule's order; only the pixels of the image are handled side by side.
"""
from __future__ import annotations

import numpy as np

from np_adaptive import quantise

f32 = np.float32
EPS = f32(1e-7)
FLOOR = f32(0.01)
THIRD = f32(0.33333334)
H5 = (f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625))
NO_DEMODULATION = 1
DEFAULTS = dict(levels=5, colour=2.0, normal=0.35, depth=0.05, albedo=0.1, flags=0)


def _pairs(H, W, dy, dx):
    """Slices of the pixels p whose q = p + (dy, dx) is inside, and of those q; None when there are none."""
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))
    if ys.stop <= ys.start or xs.stop <= xs.start:
        return None
    return ys, xs, yq, xq


def constants(colour, normal, depth, albedo):
    """The rule's host-side values: (kc2, kz2, in, ia)."""
    kc, kn, kz, ka = f32(colour), f32(normal), f32(depth), f32(albedo)
    return kc * kc, kz * kz, f32(1) / (kn * kn), f32(1) / (ka * ka)


def prepare(A, B, wa, rho, cov, flags=0):
    """-> (m, u, I, V), float32 [H, W, 3] each."""
    H, W, _ = A.shape
    m = np.maximum(rho + (f32(1) - cov)[..., None], FLOOR)
    u = np.ones_like(m) if flags & NO_DEMODULATION else m
    a, b = A / u, B / u
    wa3 = f32(0.5) if wa is None else wa[..., None]
    I = (a * wa3) + (b * (f32(1) - wa3))
    e = a - b
    e = e * e
    total = np.zeros((H, W, 3), f32)
    count = np.zeros((H, W), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            pr = _pairs(H, W, dy, dx)
            if pr is None:
                continue
            ys, xs, yq, xq = pr
            total[ys, xs] = total[ys, xs] + e[yq, xq]
            count[ys, xs] += 1
    V = (total / count.astype(f32)[..., None]) * f32(0.25)
    assert m.dtype == f32 and u.dtype == f32 and I.dtype == f32 and V.dtype == f32
    return m, u, I, V


def tap_weight(N, z, m, I, V, pr, hh, kc2, kz2, inv_n, inv_a):
    """w of the rule for the pixels p of `pr` and their taps q: float32 [h, w]."""
    ys, xs, yq, xq = pr
    n = N[yq, xq] - N[ys, xs]
    Dn = (((n[..., 0] * n[..., 0]) + (n[..., 1] * n[..., 1])) + (n[..., 2] * n[..., 2])) * inv_n
    a = m[yq, xq] - m[ys, xs]
    Da = (((a[..., 0] * a[..., 0]) + (a[..., 1] * a[..., 1])) + (a[..., 2] * a[..., 2])) * inv_a
    dz = z[yq, xq] - z[ys, xs]
    Dz = (dz * dz) / (EPS + (kz2 * (z[ys, xs] * z[yq, xq])))
    g = I[yq, xq] - I[ys, xs]
    t = (g * g) / (EPS + (kc2 * (V[ys, xs] + V[yq, xq])))
    Dc = ((t[..., 0] + t[..., 1]) + t[..., 2]) * THIRD
    D = ((Dn + Dz) + Da) + Dc
    f = np.maximum(f32(0), f32(1) - f32(0.25) * np.maximum(D, f32(0)))
    w = hh * ((f * f) * (f * f))
    assert w.dtype == f32
    return w


def level(N, z, m, I, V, s, kc2, kz2, inv_n, inv_a):
    """One level at step s: -> (I', V')."""
    H, W, _ = I.shape
    num, nv, den = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    for j in range(-2, 3):
        for i in range(-2, 3):
            pr = _pairs(H, W, j * s, i * s)
            if pr is None:
                continue
            ys, xs, yq, xq = pr
            w = tap_weight(N, z, m, I, V, pr, H5[j + 2] * H5[i + 2], kc2, kz2, inv_n, inv_a)
            num[ys, xs] = num[ys, xs] + w[..., None] * I[yq, xq]
            nv[ys, xs] = nv[ys, xs] + (w * w)[..., None] * V[yq, xq]
            den[ys, xs] = den[ys, xs] + w
    I2 = num / den[..., None]
    V2 = nv / (den * den)[..., None]
    assert I2.dtype == f32 and V2.dtype == f32
    return I2, V2


def denoise(A, B, wa, rho, N, z, cov, levels=5, colour=2.0, normal=0.35, depth=0.05, albedo=0.1, flags=0):
    """-> (image float32 [H, W, 3], rgb8 uint8 [H, W, 3]). wa None: 0.5 everywhere."""
    A, B, rho, N = (np.ascontiguousarray(x) for x in (A, B, rho, N))
    z, cov = np.ascontiguousarray(z), np.ascontiguousarray(cov)
    for x in (A, B, rho, N):
        assert x.dtype == f32 and x.shape == A.shape and x.ndim == 3 and x.shape[2] == 3
    for x in (z, cov) + (() if wa is None else (wa,)):
        assert x.dtype == f32 and x.shape == A.shape[:2]
    assert 1 <= int(levels) <= 6 and flags in (0, NO_DEMODULATION)
    assert all(np.isfinite(k) and k > 0 for k in (colour, normal, depth, albedo))
    kc2, kz2, inv_n, inv_a = constants(colour, normal, depth, albedo)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        m, u, I, V = prepare(A, B, wa, rho, cov, flags)
        for l in range(int(levels)):
            I, V = level(N, z, m, I, V, 1 << l, kc2, kz2, inv_n, inv_a)
        out = I * u
    assert out.dtype == f32
    return out, quantise(out)
