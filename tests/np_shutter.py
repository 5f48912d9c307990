"""The camera shutter (rbrt_hip_scene_set_shutter) restated in numpy float32, on top of np_lens.py and np_reference.py: the
camera ray of one sample, whole images, and every pixel's ray for given draws.

The contract (include/rbrt_hip.h "Camera shutter"): the origin o and the direction d of a sample are
made exactly as without a shutter -- jitter draws, lens draws with a lens, d = normalize(F - o) -- and then, in float32,
unfused:
    t   = the next draw of the sample's stream
    o_c = o_c + (t * travel_c)
d is not recomputed, a zero travel still draws, and the bounce draws follow."""
from __future__ import annotations

import numpy as np

import np_env
import np_lens
import np_pattern
import np_reference as R
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def travel_of(travel):
    return np.array([f32(v) for v in travel], f32)


def camera_ray_shutter(cam, lens, travel, row: int, col: int, rng: R.Rng):
    """(origin, direction) of the camera ray of the sample whose stream is `rng` on a handle with the shutter `travel`.
    cam: np_reference's dict; lens: None (the pinhole) or (lens_u, lens_v, focus_scale)."""
    o, d = R.camera_ray(cam, row, col, rng) if lens is None else np_lens.camera_ray_lens(cam, lens, row, col, rng)
    t = rng.next_f32()
    o = (o + (t * travel_of(travel)).astype(f32)).astype(f32)
    return o, d


def restated_image(cam, sc, opts, lens, travel, nodes=None, pixels=None):
    """(radiance, rgb8) of the whole image, every sample through camera_ray_shutter (travel None: no shutter, no draw) and
    np_pattern.colorize -- emitters, the constant background, smooth meshes and solid patterns on top of the reference's
    colorize -- or, with `nodes`, np_env.colorize. `pixels`: only these (row, col), the rest stays 0."""
    nc, ns = T.np_cam(cam), np_pattern.np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    lo, hi = f32(opts.min_dist), f32(opts.max_dist)
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            if travel is None:
                o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
            else:
                o, d = camera_ray_shutter(nc, lens, travel, row, col, rng)
            if nodes is not None:
                color = color + np_env.colorize(o, d, ns, nodes, opts.max_depth, rng, lo, hi)
            else:
                color = color + np_pattern.colorize(o, d, ns, bg, const, opts.max_depth, rng, lo, hi)
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


def primary_rays(cam, seed, n, lens, travel, pixels=None):
    """np_features.primary_rays on a handle with the shutter `travel`: float32 (P, n, 6)."""
    nc = T.np_cam(cam)
    W = cam.img_width_pix
    pix = [(r, c) for r in range(cam.img_height_pix) for c in range(W)] if pixels is None else list(pixels)
    rays = np.zeros((len(pix), n, 6), f32)
    for k, (row, col) in enumerate(pix):
        for s in range(n):
            o, d = camera_ray_shutter(nc, lens, travel, row, col, R.Rng(seed, row * W + col, s))
            rays[k, s, :3], rays[k, s, 3:] = o, d
    return rays


def shutter_rays(cam, lens, u0, u1, lx, ly, t, travel):
    """Every pixel's shutter ray for given jitter draws u0, u1 ((H, W) arrays), lens point (lx, ly) and shutter draw t (scalars
    or (H, W) arrays of values the draws can give), float32 operation for operation: (H*W, 6). cam: an abi.Camera; lens:
    None (the pinhole: lx, ly are not read) or (lens_u, lens_v, focus_scale)."""
    W, H = cam.img_width_pix, cam.img_height_pix
    if lens is None:  # (by hand: an all-zero lens would give pos + 1 (T - pos), which is not T - pos bit for bit)
        col = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
        row = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
        col_mm = (((col - f32(W // 2)) + u0).astype(f32) - f32(0.5)) * f32(cam.mm_per_pix_hor)
        row_mm = (((row - f32(H // 2)) + u1).astype(f32) - f32(0.5)) * f32(cam.mm_per_pix_vert)
        v = lambda a: np.array(list(a), f32)  # noqa: E731
        right, up, ctr, pos = v(cam.right), v(cam.up), v(cam.img_center_point), v(cam.position)
        target = ((ctr + (f32(0.001) * col_mm)[..., None] * right) - (f32(0.001) * row_mm)[..., None] * up).astype(f32)
        d = (target - pos).astype(f32)
        with np.errstate(all="ignore"):
            ln = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32))
            d = (d / ln[..., None]).astype(f32)
        rays = np.concatenate([np.broadcast_to(pos, d.shape), d], -1).reshape(-1, 6).astype(f32)
    else:
        rays = np_lens.lens_rays(cam, lens, u0, u1, lx, ly)
    t = np.broadcast_to(np.asarray(t, f32), (H, W)).reshape(-1, 1)
    rays = rays.copy()
    rays[:, :3] = (rays[:, :3] + (t * travel_of(travel)).astype(f32)).astype(f32)
    return rays
