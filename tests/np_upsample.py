"""Guided upsampling restated in numpy (include/rbrt_hip.h "Guided upsampling"), written from the rule and independently of the
C++: low-size half images and the full-size feature buffers in, full-size half images out; and the low camera's rule.

Everything is float32, one operation at a time (numpy never fuses), with explicit loops over a block's rows and columns and over
the four taps in the rule's order; only the pixels of an image are handled side by side. max(x, y) is the C fmaxf (np.fmax): it
returns the other operand when one is a NaN.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from rbrt_amd import abi

f32 = np.float32
EPS = f32(1e-7)
FLOOR = f32(0.01)
MIN_DEN = f32(0.01)
NO_DEMODULATION = 1
MAX_FACTOR = 4
DEFAULTS = dict(factor=2, normal=0.5, depth=0.1, albedo=0.2, flags=0)
BILINEAR = dict(normal=1e15, depth=1e15, albedo=1e15, flags=NO_DEMODULATION)  # sigmas so large that every distance is 0: plain bilinear


def low_size(W, H, f):
    """(w, h) of the low image."""
    return (W + f - 1) // f, (H + f - 1) // f


def low_camera(cam, f):
    """The rule of rbrt_hip_upsample_camera: -> abi.Camera."""
    assert 1 <= f <= MAX_FACTOR
    W, H = int(cam.img_width_pix), int(cam.img_height_pix)
    w, h = low_size(W, H, f)
    low = type(cam).from_buffer_copy(cam)
    mm_hor, mm_vert = f32(cam.mm_per_pix_hor), f32(cam.mm_per_pix_vert)
    kx = (f32(f * (w // 2)) - f32(W // 2)) + (f32(0.5) * f32(f - 1))
    ky = (f32(f * (h // 2)) - f32(H // 2)) + (f32(0.5) * f32(f - 1))
    sx, sy = f32(0.001) * (kx * mm_hor), f32(0.001) * (ky * mm_vert)
    for k in range(3):
        low.img_center_point[k] = (f32(cam.img_center_point[k]) + (sx * f32(cam.right[k]))) - (sy * f32(cam.up[k]))
    low.mm_per_pix_hor, low.mm_per_pix_vert = f32(f) * mm_hor, f32(f) * mm_vert
    low.img_width_pix, low.img_height_pix = w, h
    return low


def constants(f, normal, depth, albedo):
    """The rule's host-side values: (in, ia, kz2, invf)."""
    kn, kz, ka = f32(normal), f32(depth), f32(albedo)
    return f32(1) / (kn * kn), f32(1) / (ka * ka), kz * kz, f32(1) / f32(f)


def _block_mean(x, f, w, h):
    """(sum over each low pixel's block, rows outer, columns inner, from 0) * (1 / count): x is [H, W] or [H, W, k]."""
    H, W = x.shape[:2]
    rows, cols = np.arange(h) * f, np.arange(w) * f
    total = np.zeros((h, w) + x.shape[2:], f32)
    for dy in range(f):
        for dx in range(f):
            ry, cx = rows + dy, cols + dx
            ok = (ry < H)[:, None] & (cx < W)[None, :]
            v = x[np.minimum(ry, H - 1)][:, np.minimum(cx, W - 1)]
            ok = ok.reshape(ok.shape + (1,) * (x.ndim - 2))
            total = np.where(ok, total + v, total)
    cnt = (np.minimum(rows + f, H) - rows)[:, None] * (np.minimum(cols + f, W) - cols)[None, :]
    inv = f32(1) / cnt.astype(f32)
    out = total * inv.reshape(inv.shape + (1,) * (x.ndim - 2))
    assert out.dtype == f32
    return out


def reduce(a, b, wa, rho, N, z, cov, f, flags=0):
    """The low records: -> namespace(a, b: a~, b~ [h, w, 3]; wa, z, c [h, w]; n, m [h, w, 3])."""
    H, W = z.shape
    w, h = low_size(W, H, f)
    assert a.shape == (h, w, 3) and b.shape == (h, w, 3)
    rho_l, n_l, z_l, c_l = (_block_mean(x, f, w, h) for x in (rho, N, z, cov))
    m_l = np.fmax(rho_l + (f32(1) - c_l)[..., None], FLOOR)
    u_l = np.ones_like(m_l) if flags & NO_DEMODULATION else m_l
    wa_l = np.full((h, w), 0.5, f32) if wa is None else wa
    return SimpleNamespace(a=a / u_l, b=b / u_l, wa=wa_l, z=z_l, c=c_l, n=n_l, m=m_l)


def pack(L):
    """The low records as the library packs its workspace: float32 [4, h, w, 4], planes {a~, wa}, {b~, z}, {N, c}, {m, 0}."""
    h, w = L.z.shape
    out = np.zeros((4, h, w, 4), f32)
    out[0, ..., :3], out[0, ..., 3] = L.a, L.wa
    out[1, ..., :3], out[1, ..., 3] = L.b, L.z
    out[2, ..., :3], out[2, ..., 3] = L.n, L.c
    out[3, ..., :3] = L.m
    return out


def gather(L, rho, N, z, cov, f, normal, depth, albedo, flags=0):
    """-> (A, B float32 [H, W, 3], wa float32 [H, W], info)."""
    H, W = z.shape
    h, w = L.z.shape
    inv_n, inv_a, kz2, invf = constants(f, normal, depth, albedo)
    m = np.fmax(rho + (f32(1) - cov)[..., None], FLOOR)
    u = np.ones_like(m) if flags & NO_DEMODULATION else m
    xl = ((np.arange(W, dtype=f32) + f32(0.5)) * invf) - f32(0.5)
    yl = ((np.arange(H, dtype=f32) + f32(0.5)) * invf) - f32(0.5)
    fi, fj = np.floor(xl), np.floor(yl)
    fx, fy = xl - fi, yl - fj
    gx, gy = f32(1) - fx, f32(1) - fy
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    den, nw = np.zeros((H, W), f32), np.zeros((H, W), f32)
    na, nb = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    count = np.zeros((H, W), np.int64)
    weights, taps, bilinear = [], [], []
    for dj, di, wy, wx in ((0, 0, gy, gx), (0, 1, gy, fx), (1, 0, fy, gx), (1, 1, fy, fx)):
        bw = wx[None, :] * wy[:, None]
        qy = np.broadcast_to(np.clip(j + dj, 0, h - 1)[:, None], (H, W))
        qx = np.broadcast_to(np.clip(i + di, 0, w - 1)[None, :], (H, W))
        n = L.n[qy, qx] - N
        Dn = (((n[..., 0] * n[..., 0]) + (n[..., 1] * n[..., 1])) + (n[..., 2] * n[..., 2])) * inv_n
        d = L.m[qy, qx] - m
        Da = (((d[..., 0] * d[..., 0]) + (d[..., 1] * d[..., 1])) + (d[..., 2] * d[..., 2])) * inv_a
        zq = L.z[qy, qx]
        dz = zq - z
        Dz = (dz * dz) / (EPS + (kz2 * (z * zq)))
        D = (Dn + Dz) + Da
        g = np.fmax(f32(0), f32(1) - f32(0.25) * np.fmax(D, f32(0)))
        wt = bw * ((g * g) * (g * g))
        assert wt.dtype == f32
        add = wt > 0
        den = np.where(add, den + wt, den)
        na = np.where(add[..., None], na + wt[..., None] * L.a[qy, qx], na)
        nb = np.where(add[..., None], nb + wt[..., None] * L.b[qy, qx], nb)
        nw = np.where(add, nw + wt * L.wa[qy, qx], nw)
        count += add
        weights.append(wt)
        taps.append((qy, qx))
        bilinear.append(bw)
    valid = den >= MIN_DEN
    q0y = np.broadcast_to((np.arange(H) // f)[:, None], (H, W))
    q0x = np.broadcast_to((np.arange(W) // f)[None, :], (H, W))
    A = np.where(valid[..., None], (na / den[..., None]) * u, L.a[q0y, q0x] * u)
    B = np.where(valid[..., None], (nb / den[..., None]) * u, L.b[q0y, q0x] * u)
    wo = np.where(valid, nw / den, L.wa[q0y, q0x])
    assert A.dtype == f32 and B.dtype == f32 and wo.dtype == f32
    info = SimpleNamespace(fallback=~valid, count=count, weights=weights, taps=taps, bilinear=bilinear, q0=(q0y, q0x), den=den)
    return A, B, wo, info


def upsample(a, b, wa, rho, N, z, cov, factor=2, normal=0.5, depth=0.1, albedo=0.2, flags=0):
    """-> (A, B float32 [H, W, 3], wa float32 [H, W], info). a, b: float32 [h, w, 3]; wa: float32 [h, w] or None (0.5 everywhere);
    rho, N: float32 [H, W, 3]; z, cov: float32 [H, W]."""
    a, b, rho, N, z, cov = (np.ascontiguousarray(x) for x in (a, b, rho, N, z, cov))
    f = int(factor)
    assert 1 <= f <= MAX_FACTOR and flags in (0, NO_DEMODULATION)
    assert all(np.isfinite(k) and k > 0 for k in (normal, depth, albedo))
    H, W = z.shape
    w, h = low_size(W, H, f)
    for x in (rho, N):
        assert x.dtype == f32 and x.shape == (H, W, 3)
    for x in (a, b):
        assert x.dtype == f32 and x.shape == (h, w, 3)
    assert z.dtype == f32 and cov.dtype == f32 and cov.shape == (H, W)
    assert wa is None or (wa.dtype == f32 and wa.shape == (h, w))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        L = reduce(a, b, wa, rho, N, z, cov, f, flags)
        A, B, wo, info = gather(L, rho, N, z, cov, f, normal, depth, albedo, flags)
    info.low = L
    return A, B, wo, info


def mix(A, B, wa):
    """The plain mix of two halves (what the denoiser's window radius 0 gives): (A * wa) + (B * (1 - wa))."""
    w3 = wa[..., None]
    return (A * w3) + (B * (f32(1) - w3))
