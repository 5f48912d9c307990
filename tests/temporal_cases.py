"""Inputs for the temporal accumulation's tests (test_np_temporal.py without a GPU, test_temporal_gpu.py with one): an analytic
scene seen from pairs of cameras, with noisy half images and a history, made once per pair and size and never changed.

The scene is a ground sphere and three spheres in front of it under an empty sky. Its normal, depth and coverage are those of
the centre rays (what rbrt_hip_render_features gives with one unjittered sample), except for one column of half-covered
pixels, whose surface pixels hold half the normal and depth at coverage 0.5 as a pixel with one hit in two samples would.
In the last frame one sphere stood elsewhere, so that even under the smallest camera motion some pixels have no history."""
from __future__ import annotations

import functools
from types import SimpleNamespace

import numpy as np

import np_temporal as NT
from rbrt_amd import abi

f32 = np.float32

SPHERES = (((0.0, -1000.0, -5.0), 1000.0), ((-5.0, 1.5, -9.0), 1.5), ((-2.5, 2.9, -15.0), 3.0), ((1.5, 1.25, -9.0), 1.5))
# ... and in the last frame, when the sphere in front stood one unit to the right: what it covered and uncovered has no history
SPHERES_BEFORE = SPHERES[:3] + (((2.5, 1.25, -9.0), 1.5),)
POSITION, LOOK, UP, FOCAL_MM = (0.0, 5.0, 4.0), (0.0, -0.1, -1.0), (0.0, 1.0, -0.4), 28.0
# the last frame's camera K' of each pair, as changes against this frame's K
PAIRS = {
    "static": {},
    "drift_0.002": dict(position=(-0.002, 5.0, 4.0)),
    "drift_0.2": dict(position=(-0.2, 5.0, 4.0)),
    # `up` neither of unit length nor perpendicular to the view, and `right` leaning towards it: all of the Gram solve's terms
    "turn": dict(position=(-0.15, 5.05, 4.1), look=(0.04, -0.12, -1.0), up=(0.15, 1.0, -0.3), skew=0.1),
    "away": dict(look=(0.0, 0.1, 1.0)),
    "aside": dict(position=(-400.0, 5.0, 4.0)),
}
MOVED = ("drift_0.002", "drift_0.2", "turn")


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.sqrt((v * v).sum())


def camera(w, h, position=POSITION, look=LOOK, up=UP, focal_mm=FOCAL_MM, skew=0.0):
    """The scene files' camera: `look` is a direction, right = unit(unit(look) x unit(up)), `up` stays as written, the image
    plane is 35 mm wide and focal_mm in front of the position. skew: right = unit(right + skew * up), which no scene file gives
    and the rule allows."""
    cam = abi.Camera()
    right = _unit(_unit(np.cross(_unit(look), _unit(up))) + skew * np.asarray(up, np.float64))
    centre = np.asarray(position, np.float64) + focal_mm / 1000.0 * _unit(look)
    for k in range(3):
        cam.position[k], cam.right[k], cam.up[k], cam.img_center_point[k] = position[k], right[k], up[k], centre[k]
    cam.mm_per_pix_hor = cam.mm_per_pix_vert = 35.0 / w
    cam.img_width_pix, cam.img_height_pix = w, h
    return cam


def features(cam, spheres=SPHERES):
    """(N, z, c) of the analytic scene along the centre rays of `cam`, float32."""
    w, h = cam.img_width_pix, cam.img_height_pix
    d = NT.centre_rays(cam).astype(np.float64)
    o = np.array(list(cam.position), np.float64)
    best = np.full((h, w), np.inf)
    N = np.zeros((h, w, 3))
    for centre, radius in spheres:
        oc = o - np.asarray(centre)
        bq = (d * oc).sum(-1)
        disc = bq * bq - ((oc * oc).sum() - radius * radius)
        t = -bq - np.sqrt(np.where(disc > 0, disc, np.nan))
        hit = (disc > 0) & (t > 1e-3) & (t < best)
        best = np.where(hit, t, best)
        n = (o + t[..., None] * d - np.asarray(centre)) / radius
        N = np.where(hit[..., None], n, N)
    c = np.isfinite(best).astype(f32)
    z = np.where(c > 0, best, 0.0).astype(f32)
    N = N.astype(f32)
    half = w // 3  # the half-covered column
    c[:, half] *= f32(0.5)
    z[:, half] *= f32(0.5)
    N[:, half] *= f32(0.5)
    return N, z, c


def truth(N, c):
    """A noise-free image of the scene: a shaded surface under a graded sky."""
    h, w = c.shape
    shade = np.clip(N @ np.array([0.3, 0.8, 0.5], f32), 0.05, None)[..., None] * np.array([0.8, 0.7, 0.6], f32)
    sky = (f32(0.4) + f32(0.5) * np.arange(h, dtype=f32) / f32(max(h, 1)))[:, None, None] * np.array([0.5, 0.7, 1.0], f32)
    return np.where(c[..., None] > 0, shade, np.broadcast_to(sky, (h, w, 3))).astype(f32)


def _freeze(*arrays):
    for a in arrays:
        a.flags.writeable = False


def noisy(img, rng, sigma=0.3):
    return (img * (f32(1) + rng.normal(0.0, sigma, img.shape).astype(f32))).astype(f32)


@functools.lru_cache(maxsize=None)
def case(pair, w, h):
    """-> namespace(cam, cam_prev, A, B, N, z, c, hist): this frame's halves and features under K, and a history whose features
    are the scene's under K', whose halves are noisy and whose lengths run from 1 to 40 (beyond the default M = 32). The
    bottom-right third of A, B and of the history's halves holds values up to 1e6."""
    rng = np.random.default_rng(9000 * w + 31 * h + sorted(PAIRS).index(pair))
    cam, cam_prev = camera(w, h), camera(w, h, **PAIRS[pair])
    N, z, c = features(cam)
    Np, zp, cp = features(cam_prev, SPHERES_BEFORE)
    A, B = noisy(truth(N, c), rng), noisy(truth(N, c), rng)
    HA, HB = noisy(truth(Np, cp), rng), noisy(truth(Np, cp), rng)
    if h >= 3 and w >= 3:
        big = (slice(h - h // 3, h), slice(w - w // 3, w))
        for img in (A, B, HA, HB):
            scale = (10.0 ** rng.uniform(3.0, 7.0, img[big].shape[:2])).astype(f32)[..., None]
            img[big] = np.clip(img[big] * scale, f32(-1e6), f32(1e6))
        A[h - 1, w - 1], HB[h - 1, w - 1] = f32(1e6), f32(1e6)
    length = rng.integers(1, 41, (h, w)).astype(f32)
    hist = NT.History(HA, HB, length, Np, zp, cp)
    out = SimpleNamespace(pair=pair, w=w, h=h, cam=cam, cam_prev=cam_prev, A=A, B=B, N=N, z=z, c=c, hist=hist)
    arrays = (A, B, N, z, c, hist.a, hist.b, hist.length, hist.n, hist.z, hist.c)
    assert all(a.dtype == f32 and np.isfinite(a).all() for a in arrays)
    _freeze(*arrays)
    return out


@functools.lru_cache(maxsize=None)
def frames(w, h, n, seed=5):
    """n frames of independent noise on the scene's noise-free image under the static camera.
    -> namespace(cam, N, z, c, truth, A[n], B[n])."""
    rng = np.random.default_rng(seed)
    cam = camera(w, h)
    N, z, c = features(cam)
    t = truth(N, c)
    A = np.stack([noisy(t, rng) for _ in range(n)])
    B = np.stack([noisy(t, rng) for _ in range(n)])
    _freeze(N, z, c, t, A, B)
    return SimpleNamespace(cam=cam, N=N, z=z, c=c, truth=t, A=A, B=B)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
