"""The image comparison of include/rbrt_hip.h "Image comparison" in numpy: float32 per pixel, one rounding an operation, the
header's order; float64 sums in the header's order (the pairwise tree over a tile of 16 x 16, 256 lanes over the tiles, the
same tree again). Vectorised over the image; test_np_compare.py holds a scalar evaluation that shares no code with it."""
from __future__ import annotations

import math
import struct
from types import SimpleNamespace

import numpy as np

f32, f64 = np.float32, np.float64
MAXF = f32(3.4028235e38)
TILE_W = TILE_H = 16
LANES = 256
DEFAULTS = dict(epsilon=0.01)
_HALF = ("0.00102838012", "0.00759875821", "0.0360007733", "0.109360687", "0.213005543", "0.266011715")
TAPS = np.array([f32(t) for t in _HALF + _HALF[-2::-1]], f32)  # 11 weights, symmetric about the middle
C1, C2 = f32(0.0001), f32(0.0009)
RESULT_FORMAT = "<4df2I5I"  # rbrt_compare_result_t
assert len(TAPS) == 11 and struct.calcsize(RESULT_FORMAT) == 64


def fin(x):
    return (x <= MAXF) & (x >= -MAXF)


def luminance(img):
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * img[..., 0]) + (f32(0.7152) * img[..., 1])) + (f32(0.0722) * img[..., 2])


def pos(y):
    with np.errstate(all="ignore"):
        return np.where(fin(y) & (y > 0), y, f32(0)).astype(f32)


def tone(img):
    """T(Y(img)): float32 [H, W] in [0, 1)."""
    y = pos(luminance(img))
    return (y / (f32(1) + y)).astype(f32)


def window(m, taps=TAPS):
    """V_m of the rule: the rows' pass, then the columns', coordinates clamped, each sum from its first product on."""
    H, W = m.shape
    n = len(taps)
    for axis, size in ((1, W), (0, H)):
        acc = None
        for i in range(n):
            at = np.clip(np.arange(size) + i - n // 2, 0, size - 1)
            term = taps[i] * np.take(m, at, axis=axis)
            acc = term if acc is None else acc + term
        m = acc.astype(f32)
    return m


def ssim_map(X, R, taps=TAPS, c1=C1, c2=C2):
    u, v = tone(X), tone(R)
    mu, mv = window(u, taps), window(v, taps)
    su = window(u * u, taps) - (mu * mu)
    sv = window(v * v, taps) - (mv * mv)
    suv = window(u * v, taps) - (mu * mv)
    return ((((f32(2) * (mu * mv)) + c1) * ((f32(2) * suv) + c2)) / ((((mu * mu) + (mv * mv)) + c1) * ((su + sv) + c2))).astype(f32)


def tree(v):
    """The pairwise tree over the last axis of 256 float64 values -> v[..., 0]."""
    v = np.array(v, f64)
    assert v.shape[-1] == LANES
    s = 1
    while s < LANES:
        v[..., ::2 * s] = v[..., ::2 * s] + v[..., s::2 * s]
        s *= 2
    return v[..., 0]


def ordered_sum(values):
    """The rule's sum of one float64 value per pixel, [H, W]: tiles by the tree, the tiles by 256 lanes and the tree."""
    H, W = values.shape
    ty, tx = -(-H // TILE_H), -(-W // TILE_W)
    padded = np.zeros((ty * TILE_H, tx * TILE_W), f64)  # a pixel outside the image counts as +0.0
    padded[:H, :W] = values
    with np.errstate(all="ignore"):
        tiles = tree(padded.reshape(ty, TILE_H, tx, TILE_W).transpose(0, 2, 1, 3).reshape(ty * tx, LANES))  # row-major tile order
        lanes = np.zeros(LANES, f64)
        for j0 in range(0, len(tiles), LANES):
            part = tiles[j0:j0 + LANES]
            lanes[:len(part)] = lanes[:len(part)] + part
        return float(tree(lanes))


def compare(X, R, epsilon=0.01):
    """-> namespace(result: the 64 bytes of rbrt_compare_result_t; sum_se, sum_ae, sum_rel, sum_ssim, max_abs, usable, skipped;
    rel_map, ssim_map float32 [H, W]; se, ae, mx float32 [H, W]; ok bool [H, W])."""
    X, R = np.ascontiguousarray(X), np.ascontiguousarray(R)
    assert X.dtype == f32 and R.dtype == f32 and X.shape == R.shape and X.ndim == 3 and X.shape[2] == 3
    eps = f32(epsilon)
    assert np.isfinite(eps) and eps > 0
    ok = fin(X).all(-1) & fin(R).all(-1)
    with np.errstate(all="ignore"):
        e = (X - R).astype(f32)
        sq = (e * e).astype(f32)
        a = np.abs(e)
        se = ((sq[..., 0] + sq[..., 1]) + sq[..., 2]).astype(f32)
        ae = ((a[..., 0] + a[..., 1]) + a[..., 2]).astype(f32)
        q = (sq / ((R * R) + eps)).astype(f32)
        rel = ((q[..., 0] + q[..., 1]) + q[..., 2]).astype(f32)
        mx = np.maximum(np.maximum(a[..., 0], a[..., 1]), a[..., 2])
    zero = f32(0)
    se, ae, rel, mx = (np.where(ok, v, zero).astype(f32) for v in (se, ae, rel, mx))
    with np.errstate(all="ignore"):
        ssim = ssim_map(X, R)
    sums = [ordered_sum(v.astype(f64)) for v in (se, ae, rel, ssim)]
    max_abs = f32(mx.max())
    usable = int(ok.sum())
    skipped = ok.size - usable
    result = struct.pack(RESULT_FORMAT, *sums, float(max_abs), usable, skipped, 0, 0, 0, 0, 0)
    return SimpleNamespace(result=result, sum_se=sums[0], sum_ae=sums[1], sum_rel=sums[2], sum_ssim=sums[3], max_abs=max_abs, usable=usable,
                           skipped=skipped, rel_map=rel, ssim_map=ssim, se=se, ae=ae, mx=mx, ok=ok)


def summary(c, width, height, peak=1.0):
    """rbrt_compare_summary in Python floats (IEEE doubles): -> dict(mse, mae, relmse, psnr_db, ssim)."""
    nan = float("nan")
    if c.usable == 0:
        return dict(mse=nan, mae=nan, relmse=nan, psnr_db=nan, ssim=nan)
    n = 3.0 * float(c.usable)
    div = lambda a, b: a / b if b != 0.0 else (nan if a == 0.0 or a != a else math.copysign(math.inf, a))
    mse = c.sum_se / n
    ratio = div(peak * peak, mse)
    psnr = 10.0 * (math.log10(ratio) if 0.0 < ratio < math.inf else math.inf if ratio == math.inf else -math.inf if ratio == 0.0 else nan)
    return dict(mse=mse, mae=c.sum_ae / n, relmse=c.sum_rel / n, psnr_db=psnr, ssim=c.sum_ssim / (float(width) * float(height)))


def grey8(m, lo, hi):
    """The CLI's 8-bit maps: (m - lo) / (hi - lo) clipped to [0, 1], times 255, rounded to nearest (halves up); NaN is 0."""
    with np.errstate(all="ignore"):
        t = (m.astype(f32) - f32(lo)) / (f32(hi) - f32(lo))
        t = np.where(t > 0, np.minimum(t, f32(1)), f32(0)).astype(f32)
        return np.floor((t * f32(255)) + f32(0.5)).astype(np.uint8)
