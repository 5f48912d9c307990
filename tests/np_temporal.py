"""The temporal accumulation of include/rbrt_hip.h ("Temporal accumulation") in vectorised numpy: float32 throughout, one
operation a statement, every sum in the rule's order, so that the GPU stage can be compared bit for bit
(tests/test_temporal_gpu.py). tests/test_np_temporal.py pins this file from outside with a scalar evaluation that shares no
code with it.

A camera is anything with rbrt_camera_t's fields (abi.Camera, a SimpleNamespace). A history is a History, or None for the
first frame."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

f32 = np.float32
DEFAULTS = dict(max_history=32.0, depth=0.05, normal=0.35)
VALID_WS = f32(0.01)


def History(a, b, length, n, z, c):
    """What a frame leaves to the next: A', B', len and the frame's N, z, c."""
    return SimpleNamespace(a=np.ascontiguousarray(a, f32), b=np.ascontiguousarray(b, f32), length=np.ascontiguousarray(length, f32),
                           n=np.ascontiguousarray(n, f32), z=np.ascontiguousarray(z, f32), c=np.ascontiguousarray(c, f32))


def pack(hist):
    """The library's layout of a history: three planes of float4 records {A', len}, {B', c}, {N, z}."""
    h, w = hist.length.shape
    out = np.empty((3, h, w, 4), f32)
    out[0, ..., :3], out[0, ..., 3] = hist.a, hist.length
    out[1, ..., :3], out[1, ..., 3] = hist.b, hist.c
    out[2, ..., :3], out[2, ..., 3] = hist.n, hist.z
    return out


def vec(x):
    return np.array([x[0], x[1], x[2]], f32)


def dot(a, b):
    """((a_x b_x) + (a_y b_y)) + a_z b_z on the last axis."""
    return ((a[..., 0] * b[..., 0]) + (a[..., 1] * b[..., 1])) + (a[..., 2] * b[..., 2])


def camera_constants(cam):
    """The rule's constants of K'."""
    r, u = vec(cam.right), vec(cam.up)
    n = np.array([(r[1] * u[2]) - (r[2] * u[1]), (r[2] * u[0]) - (r[0] * u[2]), (r[0] * u[1]) - (r[1] * u[0])], f32)
    w = vec(cam.img_center_point) - vec(cam.position)
    rr, uu, ru = dot(r, r), dot(u, u), dot(r, u)
    return SimpleNamespace(n=n, w=w, wn=dot(w, n), rr=rr, uu=uu, ru=ru, det=(rr * uu) - (ru * ru),
                           sx=f32(0.001) * f32(cam.mm_per_pix_hor), sy=f32(0.001) * f32(cam.mm_per_pix_vert), right=r, up=u,
                           position=vec(cam.position))


def centre_rays(cam):
    """d[H][W][3]: the render's own ray of every pixel with both jitter draws at 0.5."""
    w, h = int(cam.img_width_pix), int(cam.img_height_pix)
    hx, hy = f32(w // 2), f32(h // 2)
    cm = (np.arange(w, dtype=f32) - hx) * f32(cam.mm_per_pix_hor)
    rm = (np.arange(h, dtype=f32) - hy) * f32(cam.mm_per_pix_vert)
    sc = (f32(0.001) * cm)[None, :, None]
    sr = (f32(0.001) * rm)[:, None, None]
    T = (vec(cam.img_center_point) + (sc * vec(cam.right))) - (sr * vec(cam.up))
    e = T - vec(cam.position)
    return e / np.sqrt(dot(e, e))[..., None]


def accumulate(A, B, N, z, c, cam, cam_prev=None, hist=None, max_history=32.0, depth=0.05, normal=0.35):
    """One frame. -> (A', B', len, the next History, info); info holds the intermediates the tests ask about: surface, projects,
    xs, ys, i, j, accepted[4] (per tap, False outside the image), ws, valid."""
    A, B, N = (np.ascontiguousarray(x, f32) for x in (A, B, N))
    z, c = np.ascontiguousarray(z, f32), np.ascontiguousarray(c, f32)
    h, w = z.shape
    assert (w, h) == (int(cam.img_width_pix), int(cam.img_height_pix))
    if hist is None:
        length = np.ones((h, w), f32)
        return A.copy(), B.copy(), length, History(A, B, length, N, z, c), None
    M, kz, kn = f32(max_history), f32(depth), f32(normal)
    kn2 = kn * kn
    K = camera_constants(cam_prev)
    hx, hy = f32(w // 2), f32(h // 2)
    with np.errstate(all="ignore"):
        d = centre_rays(cam)
        surface = c > 0
        zbar = z / c
        P = vec(cam.position) + (zbar[..., None] * d)
        v = np.where(surface[..., None], P - K.position, d).astype(f32)
        t = K.wn / dot(v, K.n)
        Q = (t[..., None] * v) - K.w
        qr, qu = dot(Q, K.right), dot(Q, K.up)
        a = ((qr * K.uu) - (qu * K.ru)) / K.det
        b = ((qr * K.ru) - (qu * K.rr)) / K.det
        xs = (a / K.sx) + hx
        ys = (b / K.sy) + hy
        projects = (t > 0) & (t < f32(np.inf)) & (xs > f32(-1)) & (xs < f32(w)) & (ys > f32(-1)) & (ys < f32(h))
        xc, yc = np.where(projects, xs, f32(0)), np.where(projects, ys, f32(0))  # (the others take no tap: any index will do)
        fi, fj = np.floor(xc), np.floor(yc)
        i, j = fi.astype(np.int64), fj.astype(np.int64)
        fx, fy = xc - fi, yc - fj
        gx, gy = f32(1) - fx, f32(1) - fy
        ze = np.sqrt(dot(v, v))
        ztol = kz * ze
        ws, sl = np.zeros((h, w), f32), np.zeros((h, w), f32)
        sa, sb = np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32)
        accepted = np.zeros((4, h, w), bool)
        for k, (dj, di, bw) in enumerate(((0, 0, gx * gy), (0, 1, fx * gy), (1, 0, gx * fy), (1, 1, fx * fy))):
            qy, qx = j + dj, i + di
            inside = projects & (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
            qy, qx = np.where(inside, qy, 0), np.where(inside, qx, 0)
            cq = hist.c[qy, qx]
            zq = hist.z[qy, qx] / cq
            D = N - hist.n[qy, qx]
            ok_surface = (cq > 0) & (np.abs(zq - ze) <= ztol) & (dot(D, D) <= kn2)
            acc = inside & np.where(surface, ok_surface, cq == 0)
            accepted[k] = acc
            ws = np.where(acc, ws + bw, ws)
            sa = np.where(acc[..., None], sa + (bw[..., None] * hist.a[qy, qx]), sa)
            sb = np.where(acc[..., None], sb + (bw[..., None] * hist.b[qy, qx]), sb)
            sl = np.where(acc, sl + (bw * hist.length[qy, qx]), sl)
        valid = ws >= VALID_WS
        HA, HB, hl = sa / ws[..., None], sb / ws[..., None], sl / ws
        length = np.where(valid, np.minimum(hl + f32(1), M), f32(1)).astype(f32)
        alpha = (f32(1) / length)[..., None]
        oa = np.where(valid[..., None], HA + (alpha * (A - HA)), A).astype(f32)
        ob = np.where(valid[..., None], HB + (alpha * (B - HB)), B).astype(f32)
    info = SimpleNamespace(surface=surface, projects=projects, xs=xs, ys=ys, i=i, j=j, accepted=accepted, ws=ws, valid=valid)
    return oa, ob, length, History(oa, ob, length, N, z, c), info
