"""Inputs for the guided denoiser's tests (test_np_guided.py without a GPU, test_guided_gpu.py with one): synthetic half images
with their feature buffers, made once per size and never changed."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

f32 = np.float32


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


@functools.lru_cache(maxsize=None)
def synthetic(w, h):
    """(A, B, wa, rho, N, z, cov) for a w x h image.
    Features: the albedo is a gentle ramp (differences the albedo term lets through in part) times a checker of 5-pixel cells
    (steps it stops); the normal turns slowly and flips at the column 3w/5; the depth is a ramp with a step at the row h/2; the
    last column third of the first row third is background (coverage 0, depth 0, albedo 0, normal 0) with a half-covered rim.
    Colour: albedo times a shading ramp, with independent noise in each half; the top-left quarter has A == B; the bottom-right
    third holds values up to 1e6. Nothing is 0 in A and B."""
    rng = np.random.default_rng(7000 * w + h)
    y, x = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    checker = (((x // 5) + (y // 5)) % 2).astype(f32)
    rho = ((f32(0.35) + f32(0.004) * x + f32(0.003) * y)[..., None] * np.array([1.0, 0.9, 0.8], f32)
           + checker[..., None] * np.array([0.3, 0.25, 0.2], f32)).astype(f32)
    ang = f32(0.02) * x + f32(0.015) * y
    N = np.stack([np.sin(ang), np.cos(ang) * f32(0.8), np.full_like(ang, 0.6)], -1).astype(f32)
    N[:, (3 * w) // 5:, 0] *= f32(-1)
    z = (f32(5) + f32(0.02) * x + f32(0.01) * y).astype(f32)
    z[h // 2:] += f32(3)
    cov = np.ones((h, w), f32)
    if h >= 3 and w >= 3:
        bg = (slice(0, h // 3), slice(w - w // 3, w))
        cov[bg], z[bg], rho[bg], N[bg] = 0, 0, 0, 0
        rim = (slice(0, h // 3), w - w // 3)
        cov[rim], z[rim] = f32(0.5), f32(2.5)
    shade = (f32(0.3) + f32(0.6) * x / f32(w) + f32(0.2) * y / f32(h))[..., None]
    truth = (np.maximum(rho + (f32(1) - cov)[..., None], f32(0.01)) * shade).astype(f32)
    a = (truth * (f32(1) + rng.normal(0.0, 0.08, (h, w, 3)).astype(f32))).astype(f32)
    b = (truth * (f32(1) + rng.normal(0.0, 0.08, (h, w, 3)).astype(f32))).astype(f32)
    a, b = np.abs(a) + f32(1e-3), np.abs(b) + f32(1e-3)
    b[:(h + 1) // 2, :(w + 1) // 2] = a[:(h + 1) // 2, :(w + 1) // 2]
    if h >= 3 and w >= 3:
        big = (slice(h - h // 3, h), slice(w - w // 3, w))
        scale = (10.0 ** rng.uniform(3.0, 7.0, a[big].shape[:2])).astype(f32)[..., None]
        a[big], b[big] = np.minimum(a[big] * scale, f32(1e6)), np.minimum(b[big] * scale, f32(1e6))
    wa = rng.uniform(0.3, 0.7, (h, w)).astype(f32)
    out = (a, b, wa, rho, N, z, cov)
    for arr in out:
        assert arr.dtype == f32 and np.isfinite(arr).all()
    assert (a != 0).all() and (b != 0).all() and (z >= 0).all()
    _freeze(*out)
    return out


@functools.lru_cache(maxsize=None)
def prototype(w=96, h=64, spp_half=8, seed=11):
    """The scene the rule was prototyped on: a checker albedo, a shadow edge no feature knows about, a step in normal and depth,
    exponential noise with spp_half samples a half. -> namespace(truth, A, B, rho, N, z, cov), float32."""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    checker = (((x // 8) + (y // 8)) % 2).astype(f32)
    rho = (np.array([0.2, 0.25, 0.3], f32) + checker[..., None] * np.array([0.6, 0.5, 0.4], f32)).astype(f32)
    light = np.where(x + y // 2 < (2 * w) // 3, f32(1.0), f32(0.35)).astype(f32)         # the shadow edge
    right = x >= w // 2                                                                 # the geometry step
    N = np.where(right[..., None], np.array([0.6, 0.0, 0.8], f32), np.array([0.0, 0.0, 1.0], f32)).astype(f32)
    z = np.where(right, f32(9.0), f32(6.0)).astype(f32) + f32(0.01) * x.astype(f32)
    light = (light * np.where(right, f32(0.8), f32(1.0))).astype(f32)
    truth = (rho * light[..., None]).astype(f32)
    halves = []
    for _ in range(2):
        s = rng.exponential(1.0, (spp_half, h, w, 1)).astype(f32).mean(0, dtype=np.float64).astype(f32)
        halves.append((truth * s).astype(f32))
    c = SimpleNamespace(truth=truth, A=halves[0], B=halves[1], rho=rho, N=N, z=z.astype(f32), cov=np.ones((h, w), f32), checker=checker)
    _freeze(c.truth, c.A, c.B, c.rho, c.N, c.z, c.cov, c.checker)
    return c


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
