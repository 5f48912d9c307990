"""Inputs for the guided upsampling's tests (test_np_upsample.py without a GPU, test_upsample_gpu.py with one): synthetic
full-size feature buffers and low-size half images, made once per size and factor and never changed.

The scene is an empty sky over a ground whose depth falls towards the horizon and whose albedo changes on a straight vertical
edge, with a sphere in front. The features are what rbrt_hip_render_features gives with 4 x 4 regular samples a pixel: the
horizon lies inside a pixel row and the sphere's rim crosses pixels, so those pixels are partly covered and hold the sums of
their samples. The albedo edge lies on an odd pixel column, so that full pixels are pure and low pixels straddle it for every
factor. The low halves are block means of albedo times a light that differs per object, with independent noise in each half."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import np_upsample as NU

f32 = np.float32
SUB = 4  # samples a pixel and direction
LIGHT = {"sky": (0.5, 0.7, 1.0), "ground": (0.6, 0.6, 0.6), "sphere": (0.95, 0.9, 0.8)}
ALBEDO = {"left": (0.8, 0.3, 0.2), "right": (0.2, 0.3, 0.8), "sphere": (0.7, 0.7, 0.2)}


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


def edge_column(W):
    """The first column of the ground's right albedo: odd, so a block of 2 or 4 columns never ends in front of it (W = 50: 23,
    which blocks of 3 straddle too)."""
    return (W * 9 // 20) | 1


@functools.lru_cache(maxsize=None)
def features(W, H):
    """-> namespace(rho, N [H, W, 3]; z, cov [H, W]; light [H, W, 3]: the per-pixel mean of its samples' light; obj [H, W]: the
    object of the pixel's first sample, 0 sky, 1 ground left, 2 ground right, 3 sphere)."""
    n = SUB
    ys = (np.arange(H * n, dtype=np.float64) + 0.5) / n   # sample positions in pixels
    xs = (np.arange(W * n, dtype=np.float64) + 0.5) / n
    Y, X = np.meshgrid(ys, xs, indexing="ij")
    horizon = 0.35 * H + 0.37
    edge = float(edge_column(W))
    cy, cx, rad = 0.55 * H + 0.2, 0.62 * W + 0.3, 0.23 * min(W, H) + 0.4
    obj = np.where(Y < horizon, 0, np.where(X < edge, 1, 2))
    d2 = (X - cx) ** 2 + (Y - cy) ** 2
    on = d2 < rad * rad
    obj = np.where(on, 3, obj)
    nz = np.sqrt(np.where(on, 1.0 - d2 / (rad * rad), 0.0))
    N = np.zeros((H * n, W * n, 3))
    N[obj == 1] = N[obj == 2] = (0.0, 1.0, 0.0)
    N[on] = np.stack([(X - cx) / rad, -(Y - cy) / rad, nz], -1)[on]
    depth = np.where(obj == 0, 0.0, 4.0 + 20.0 * (H - Y) / max(H - horizon, 1.0))   # the ground: far at the horizon
    depth = np.where(on, 6.0 - 1.5 * nz, depth)
    rho = np.zeros((H * n, W * n, 3))
    rho[obj == 1], rho[obj == 2], rho[obj == 3] = ALBEDO["left"], ALBEDO["right"], ALBEDO["sphere"]
    light = np.zeros((H * n, W * n, 3))
    light[obj == 0] = LIGHT["sky"]
    light[(obj == 1) | (obj == 2)] = LIGHT["ground"]
    light[on] = (np.asarray(LIGHT["sphere"]) * (0.3 + 0.7 * nz[..., None]))[on]
    hit = (obj != 0).astype(np.float64)

    def mean(x):
        return x.reshape(H, n, W, n, *x.shape[2:]).mean(axis=(1, 3)).astype(f32)

    out = SimpleNamespace(rho=mean(rho), N=mean(N), z=mean(depth), cov=mean(hit), light=mean(light), obj=obj[::n, ::n].copy())
    _freeze(out.rho, out.N, out.z, out.cov, out.light, out.obj)
    return out


@functools.lru_cache(maxsize=None)
def case(W, H, f, sigma=0.05):
    """-> namespace(W, H, f, w, h; a, b [h, w, 3], wa [h, w]; rho, N, z, cov: the features; truth [H, W, 3]: the noise-free full
    image; left, straddle [h, w]: the low pixels of ground rows whose block lies left of the albedo edge, or across it)."""
    F = features(W, H)
    w, h = NU.low_size(W, H, f)
    rng = np.random.default_rng(1000 * W + 10 * H + f)
    m = np.maximum(F.rho + (f32(1) - F.cov)[..., None], f32(0.01))
    truth = (m * F.light).astype(f32)
    low = NU._block_mean(truth, f, w, h)
    a = (low * (f32(1) + rng.normal(0.0, sigma, low.shape).astype(f32))).astype(f32)
    b = (low * (f32(1) + rng.normal(0.0, sigma, low.shape).astype(f32))).astype(f32)
    wa = rng.uniform(0.3, 0.7, (h, w)).astype(f32)
    edge = edge_column(W)
    c0, c1 = np.arange(w) * f, np.minimum(np.arange(w) * f + f, W) - 1
    left = np.broadcast_to((c1 < edge)[None, :], (h, w)).copy()
    straddle = np.broadcast_to(((c0 < edge) & (c1 >= edge))[None, :], (h, w)).copy()
    out = SimpleNamespace(W=W, H=H, f=f, w=w, h=h, a=a, b=b, wa=wa, rho=F.rho, N=F.N, z=F.z, cov=F.cov, truth=truth, obj=F.obj,
                          left=left, straddle=straddle, edge=edge)
    assert all(x.dtype == f32 and np.isfinite(x).all() for x in (a, b, wa, truth))
    _freeze(a, b, wa, truth, left, straddle)
    return out


def planted(c, info):
    """The NaN case: copies of c's low halves and mix with NaN and infinities in low pixels that no accepted tap reaches.
    -> (a, b, wa, bad [h, w]: the planted low pixels, listed [H, W]: the full pixels that may differ -- the fallback pixels
    whose q0 is planted). `info` is the restatement's for the clean case."""
    used = np.zeros((c.h, c.w), bool)
    for (qy, qx), wt in zip(info.taps, info.weights):
        used[qy[wt > 0], qx[wt > 0]] = True
    free = np.argwhere(~used)
    a, b, wa = c.a.copy(), c.b.copy(), c.wa.copy()
    bad = np.zeros((c.h, c.w), bool)
    values = (f32(np.nan), f32(np.inf), f32(-np.inf))
    for k, (y, x) in enumerate(free):
        a[y, x, k % 3] = values[k % 3]            # one channel of a, another of b, and the mix: three kinds a pixel
        b[y, x, (k + 1) % 3] = values[(k + 1) % 3]
        wa[y, x] = values[(k + 2) % 3]
        if k % 4 == 3:
            a[y, x], b[y, x] = values[k % 3], values[(k + 1) % 3]
        bad[y, x] = True
    listed = info.fallback & bad[info.q0]
    return a, b, wa, bad, listed


def rmse(x, y):
    return float(np.sqrt(np.mean((np.asarray(x, np.float64) - np.asarray(y, np.float64)) ** 2)))
