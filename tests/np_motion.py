"""Moving spheres (rbrt_hip_scene_set_motion) restated in numpy float32, on top of np_shutter.py and np_pattern.py: the
scene a sample sees, whole images, and the primary rays with their draws.

The contract (include/rbrt_hip.h "Moving spheres"): a sample's ray is made exactly as without a motion;
if the handle has a shutter or a motion the next draw of the stream is t, ONE draw for both; with a shutter
o += t * travel; with a motion every sphere centre the sample's path reads is, in float32, unfused,
    c_i(t) = c_i + (t * travel_i)
for the camera ray and every bounce. Nothing else moves, and an all-zero motion still draws."""
from __future__ import annotations

import numpy as np

import np_env
import np_lens
import np_pattern
import np_reference as R
import np_shutter
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def travels_of(travels):
    return np.asarray(travels, f32).reshape(-1, 3)


def centre_at(c, travel, t):
    """c_i(t): a product and a sum per component, float32."""
    return (np.asarray(c, f32) + (f32(t) * np.asarray(travel, f32)).astype(f32)).astype(f32)


def scene_at(ns, travels, t):
    """A copy of np_pattern.np_scene's dict with every sphere where the draw t puts it."""
    out = dict(ns)
    out["spheres"] = [(centre_at(c, tv, t), r, m) for (c, r, m), tv in zip(ns["spheres"], travels_of(travels))]
    return out


def camera_ray_motion(cam, lens, shutter, row: int, col: int, rng: R.Rng):
    """(origin, direction, t) of the camera ray of the sample whose stream is `rng` on a handle with a motion and the shutter
    `shutter` (None: no shutter): the one draw, and the origin it moves when there is a shutter."""
    o, d = R.camera_ray(cam, row, col, rng) if lens is None else np_lens.camera_ray_lens(cam, lens, row, col, rng)
    t = rng.next_f32()
    if shutter is not None:
        o = (o + (t * np_shutter.travel_of(shutter)).astype(f32)).astype(f32)
    return o, d, t


def restated_image(cam, sc, opts, travels, lens=None, shutter=None, nodes=None, pixels=None):
    """(radiance, rgb8) of the whole image on a handle with the motion `travels` ((n_spheres, 3)), every sample through
    camera_ray_motion and np_pattern.colorize -- or, with `nodes`, np_env.colorize -- on scene_at(its own t). `pixels`: only
    these (row, col), the rest stays 0."""
    nc, ns = T.np_cam(cam), np_pattern.np_scene(sc)
    tv = travels_of(travels)
    assert len(tv) == len(ns["spheres"])
    assert not ns["patterns"] or nodes is None  # (np_env.colorize knows no pattern: np_whole.restated_image does both)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    lo, hi = f32(opts.min_dist), f32(opts.max_dist)
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            o, d, t = camera_ray_motion(nc, lens, shutter, row, col, rng)
            moved = scene_at(ns, tv, t)
            if nodes is not None:
                color = color + np_env.colorize(o, d, moved, nodes, opts.max_depth, rng, lo, hi)
            else:
                color = color + np_pattern.colorize(o, d, moved, bg, const, opts.max_depth, rng, lo, hi)
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


def primary_rays(cam, seed, n, lens=None, shutter=None, pixels=None):
    """np_features.primary_rays on a handle with a motion: (rays float32 (P, n, 6), t float32 (P, n)), the draw of every
    sample beside its ray (the feature buffers and the tile pass test sample s against scene_at(t[., s]))."""
    nc = T.np_cam(cam)
    W = cam.img_width_pix
    pix = [(r, c) for r in range(cam.img_height_pix) for c in range(W)] if pixels is None else list(pixels)
    rays, ts = np.zeros((len(pix), n, 6), f32), np.zeros((len(pix), n), f32)
    for k, (row, col) in enumerate(pix):
        for s in range(n):
            o, d, t = camera_ray_motion(nc, lens, shutter, row, col, R.Rng(seed, row * W + col, s))
            rays[k, s, :3], rays[k, s, 3:], ts[k, s] = o, d, t
    return rays, ts
