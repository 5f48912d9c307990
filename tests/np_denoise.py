"""The denoiser restated in numpy (include/rbrt_hip.h "Denoising"), written from the rule and
independently of the C++: two half images and their mix in, the filtered image out.

Everything is float32, one operation at a time (numpy never fuses), with explicit loops over the window's offsets and the
patch's columns and rows in the rule's order; only the pixels of the image are handled side by side.
"""
from __future__ import annotations

import numpy as np

from np_adaptive import TILE, quantise

f32 = np.float32
EPS = f32(1e-7)
DEFAULTS = dict(window_radius=5, patch_radius=3, strength=0.7)


def variance(A, B):
    """V: float32 [H, W, 3]."""
    H, W, _ = A.shape
    d = A - B
    d = d * d
    total = np.zeros((H, W, 3), f32)
    count = np.zeros((H, W), np.int64)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))        # p with p + o inside
            yq, xq = slice(max(0, dy), min(H, H + dy)), slice(max(0, dx), min(W, W + dx))          # those p + o
            total[ys, xs] = total[ys, xs] + d[yq, xq]
            count[ys, xs] += 1
    V = (total / count.astype(f32)[..., None]) * f32(0.5)
    assert V.dtype == f32
    return V


def _pairs(H, W, dy, dx):
    """Slices of the pixels p whose q = p + (dy, dx) is inside, and of those q. Empty when there are none."""
    ys, xs = slice(max(0, -dy), max(0, min(H, H - dy))), slice(max(0, -dx), max(0, min(W, W - dx)))
    yq, xq = slice(max(0, dy), max(0, min(H, H + dy))), slice(max(0, dx), max(0, min(W, W + dx)))
    return ys, xs, yq, xq


def _inside_count(n, P, d):
    """Per coordinate c in [0, n): how many j in -P..P have both c + j and c + j + d inside."""
    out = np.zeros(n, np.int64)
    for c in range(n):
        for j in range(-P, P + 1):
            if 0 <= c + j < n and 0 <= c + j + d < n:
                out[c] += 1
    return out


def patch_distance(G, V, dy, dx, P, k2):
    """D(p, o) for every pixel p: float32 [H, W] (the value at a p whose q is outside is never used)."""
    H, W, _ = G.shape
    # delta over the image and a border of P around it: 0 where p or q is outside
    delta = np.zeros((H + 2 * P, W + 2 * P), f32)
    ys, xs, yq, xq = _pairs(H, W, dy, dx)
    if ys.stop > ys.start and xs.stop > xs.start:
        gp, gq, vp, vq = G[ys, xs], G[yq, xq], V[ys, xs], V[yq, xq]
        g = gq - gp
        t = ((g * g) - (vp + np.minimum(vp, vq))) / (EPS + k2 * (vp + vq))
        assert t.dtype == f32
        delta[P + ys.start:P + ys.stop, P + xs.start:P + xs.stop] = (t[..., 0] + t[..., 1]) + t[..., 2]
    rows = np.zeros((H + 2 * P, W), f32)        # r of every row of the bordered area, for the patch centred at column x
    for i in range(2 * P + 1):                  # left to right
        rows = rows + delta[:, i:i + W]
    D = np.zeros((H, W), f32)
    for j in range(2 * P + 1):                  # top to bottom
        D = D + rows[j:j + H]
    n = f32(3) * np.outer(_inside_count(H, P, dy), _inside_count(W, P, dx)).astype(f32)   # (small integers: exact)
    with np.errstate(divide="ignore", invalid="ignore"):  # (n = 0 only where q is outside)
        D = D / n
    assert D.dtype == f32
    return D


def weight(D):
    t = np.maximum(f32(0), f32(1) - f32(0.25) * np.maximum(D, f32(0)))
    w = (t * t) * (t * t)
    assert w.dtype == f32
    return w


def nlm(F, G, V, R, P, k2):
    """filter(F, G): float32 [H, W, 3]."""
    H, W, _ = F.shape
    num, den = np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            ys, xs, yq, xq = _pairs(H, W, dy, dx)
            if not (ys.stop > ys.start and xs.stop > xs.start):
                continue
            w = weight(patch_distance(G, V, dy, dx, P, k2))[ys, xs]
            num[ys, xs] = num[ys, xs] + w[..., None] * F[yq, xq]
            den[ys, xs] = den[ys, xs] + w
    out = num / den[..., None]
    assert out.dtype == f32
    return out


def filtered_halves(A, B, window_radius=5, patch_radius=3, strength=0.7):
    """-> (Ah, Bh) = (filter(A, guide B), filter(B, guide A)), float32 [H, W, 3] each."""
    A, B = np.ascontiguousarray(A), np.ascontiguousarray(B)
    assert A.dtype == f32 and B.dtype == f32 and A.shape == B.shape and A.ndim == 3 and A.shape[2] == 3
    R, P = int(window_radius), int(patch_radius)
    assert 0 <= R <= 10 and 0 <= P <= 4 and np.isfinite(strength) and strength > 0
    k = f32(strength)
    k2 = k * k
    assert k2.dtype == f32
    with np.errstate(over="ignore", invalid="ignore"):
        V = variance(A, B)
        return nlm(A, B, V, R, P, k2), nlm(B, A, V, R, P, k2)


def denoise(A, B, wa=None, window_radius=5, patch_radius=3, strength=0.7):
    """-> (image float32 [H, W, 3], rgb8 uint8 [H, W, 3]). wa None: 0.5 everywhere."""
    Ah, Bh = filtered_halves(A, B, window_radius, patch_radius, strength)
    out = mix(Ah, Bh, wa)
    return out, quantise(out)


def mix(A, B, wa=None):
    """(A * wa) + (B * (1 - wa)): the output from the two filtered halves, and what R = 0 returns for the halves themselves."""
    assert A.dtype == f32 and B.dtype == f32 and (wa is None or (wa.dtype == f32 and wa.shape == A.shape[:2]))
    wa3 = f32(0.5) if wa is None else wa[..., None]
    out = (A * wa3) + (B * (f32(1) - wa3))
    assert out.dtype == f32
    return out


def halves_from_samples(samples, counts):
    """samples float32 [N, H, W, 3], counts [tiles_y, tiles_x] -> (S, S_even): every pixel's samples added in order up to
    its tile's count, S_even those with an even index."""
    samples = np.asarray(samples)
    assert samples.dtype == f32
    N, H, W, _ = samples.shape
    py, px = np.meshgrid(np.arange(H) // TILE, np.arange(W) // TILE, indexing="ij")
    n = np.asarray(counts)[py, px]
    assert n.max() <= N
    S, S_even = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    for s in range(N):
        m = n > s
        S[m] = S[m] + samples[s][m]
        if s % 2 == 0:
            S_even[m] = S_even[m] + samples[s][m]
    return S, S_even


def halves(S, S_even, counts):
    """The rule's "From a handle's sums": -> (A, B, wa)."""
    H, W, _ = S.shape
    assert S.dtype == f32 and S_even.dtype == f32
    py, px = np.meshgrid(np.arange(H) // TILE, np.arange(W) // TILE, indexing="ij")
    n = np.asarray(counts).astype(np.int64)[py, px]
    assert n.min() >= 2
    h = (n + 1) // 2
    g = n - h
    inv_h, inv_g, inv_n = f32(1) / h.astype(f32), f32(1) / g.astype(f32), f32(1) / n.astype(f32)
    A = S_even * inv_h[..., None]
    B = (S - S_even) * inv_g[..., None]
    wa = h.astype(f32) * inv_n
    assert A.dtype == f32 and B.dtype == f32 and wa.dtype == f32
    return A, B, wa
