"""Every extension at once, restated in numpy float32: the thin lens camera (np_lens.camera_ray_lens) in front of
np_smooth.colorize (emitters, the constant background and the shading normal of smooth meshes, on top of the reference's
colorize). One function covers what the product adds to the reference; the CPU oracle's rbrt_oracle_render_ext must give
its image bit for bit (tests/test_oracle_extensions.py)."""
from __future__ import annotations

import numpy as np

import np_lens
import np_reference as R
import np_smooth
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def restated_image(cam, sc, opts, lens=None, pixels=None):
    """(radiance, rgb8) of the image for a scene of abi types: lens None (the pinhole) or (lens_u, lens_v, focus_scale);
    `pixels`: only these (row, col), the rest stays 0."""
    nc, ns = T.np_cam(cam), np_smooth.np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
            color = color + np_smooth.colorize(o, d, ns, bg, const, opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist))
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)
