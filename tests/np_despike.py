"""The spike removal of include/rbrt_hip.h "Spike removal" in numpy: float32 throughout, one rounding an operation, the
header's order. Vectorised over the image; test_np_despike.py holds a scalar evaluation that shares no code with it.

The k-th largest of a window comes from the same compare-exchange chain the kernel uses, applied to whole planes: only values
matter, so any correct selection gives the same bits (the scalar evaluation sorts instead)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

f32 = np.float32
MAXF = f32(3.4028235e38)
MAX_RADIUS, MAX_RANK = 2, 4
DEFAULTS = dict(radius=2, rank=2, threshold=4.0, floor=0.01)


def fin(x):
    return (x <= MAXF) & (x >= -MAXF)


def luminance(img):
    """Y of the rule: float32 [H, W]."""
    with np.errstate(all="ignore"):
        return ((f32(0.2126) * img[..., 0]) + (f32(0.7152) * img[..., 1])) + (f32(0.0722) * img[..., 2])


def pos(y):
    """x where it is finite and above 0, else +0."""
    with np.errstate(all="ignore"):
        return np.where(fin(y) & (y > 0), y, f32(0)).astype(f32)


def rank_value(y, radius, rank):
    """r of the rule for every pixel of the luminance plane y: float32 [H, W]."""
    H, W = y.shape
    R = int(radius)
    padded = np.zeros((H + 2 * R, W + 2 * R), f32)  # outside the image: +0, one more zero
    padded[R:R + H, R:R + W] = pos(y)
    top = [np.zeros((H, W), f32) for _ in range(rank)]
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            v = padded[R + dy:R + dy + H, R + dx:R + dx + W]
            for j in range(rank):
                hi, v = np.maximum(top[j], v), np.minimum(top[j], v)  # (finite, no -0: the order of the operands is immaterial)
                top[j] = hi
    return top[rank - 1]


def limit_half(X, O, radius, rank, threshold, floor):
    """One half: -> (X' float32 [H, W, 3], flagged bool [H, W], info)."""
    t, f = f32(threshold), f32(floor)
    y, yo = luminance(X), luminance(O)
    r = rank_value(y, radius, rank)
    base = np.maximum(r, pos(yo))
    with np.errstate(all="ignore"):
        lim = np.minimum((t * base) + f, MAXF).astype(f32)
        nonfinite = ~fin(y)
        above = ~nonfinite & (y > lim)
        s = (lim / np.where(above, y, f32(1))).astype(f32)
        scaled = (X * s[..., None]).astype(f32)
    out = X.copy()
    out[above] = scaled[above]
    out[nonfinite] = lim[nonfinite][:, None]
    with np.errstate(all="ignore"):
        by_rank = ~nonfinite & ~above & (y > ((t * pos(yo)) + f))  # kept by the window alone: the other half would not have
        by_other = ~nonfinite & ~above & (y > ((t * r) + f))       # kept by the other half alone
    return out, above | nonfinite, SimpleNamespace(y=y, r=r, lim=lim, above=above, nonfinite=nonfinite, kept_by_rank=by_rank, kept_by_other=by_other)


def despike(A, B, radius=2, rank=2, threshold=4.0, floor=0.01):
    """-> (A', B' float32 [H, W, 3], mask uint8 [H, W], (spikes_a, spikes_b), info: namespace(a, b))."""
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    assert A.dtype == f32 and B.dtype == f32 and A.shape == B.shape and A.ndim == 3 and A.shape[2] == 3
    assert 1 <= radius <= MAX_RADIUS and 1 <= rank <= MAX_RANK
    assert np.isfinite(threshold) and threshold >= 1 and np.isfinite(floor) and floor >= 0
    oa, fa, ia = limit_half(A, B, radius, rank, threshold, floor)
    ob, fb, ib = limit_half(B, A, radius, rank, threshold, floor)
    mask = (fa.astype(np.uint8) | (fb.astype(np.uint8) << 1)).astype(np.uint8)
    return oa, ob, mask, (int(fa.sum()), int(fb.sum())), SimpleNamespace(a=ia, b=ib)


def spike_map(mask):
    """The CLI's --spike-map: 0 none, 85 A, 170 B, 255 both."""
    return (mask.astype(np.uint8) * np.uint8(85)).astype(np.uint8)
