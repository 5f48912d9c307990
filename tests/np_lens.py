"""The thin lens (RBRT_FLAG_THIN_LENS) restated in numpy float32, on top of np_reference.py: the host's derivation of the
lens from the YAML keys, the camera ray of one sample, the rays of a whole image for given draws, and whole images.

The contract (include/rbrt_hip.h rbrt_camera_lens_t): after the column and row jitter draws that
place the pinhole target T, in float32, unfused, in this order:
    repeat lx = 2 u - 1; ly = 2 u - 1 until lx lx + ly ly < 1
    o = position + ((lx u_c) + (ly v_c))   F = position + focus_scale (T - position)   d = normalize(F - o)
and the bounce draws follow."""
from __future__ import annotations

import numpy as np

import np_reference as R
import test_emissive as E
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def lens_from_yaml(right, look_at, focal_mm, aperture_mm, focus_distance):
    """Camera::set_lens (rbrt_amd/host/scene.cpp): (lens_u, lens_v, focus_scale), float32 step by step."""
    right = np.array(right, f32)
    r = f32(f32(aperture_mm) / f32(2000.0))
    lens_u = r * right
    lens_v = r * R.normalize(R.cross(right, R.normalize(np.array(look_at, f32))))
    focus_scale = f32(f32(focus_distance) / f32(f32(focal_mm) / f32(1000.0)))
    return lens_u, lens_v, focus_scale


def lens_for(cam, look_at, focal_mm, aperture_mm, focus_distance):
    """The lens tuple (lens_u, lens_v, focus_scale) of `cam` (an abi.Camera) for the render calls."""
    u, v, fs = lens_from_yaml(list(cam.right), look_at, focal_mm, aperture_mm, focus_distance)
    return tuple(float(x) for x in u), tuple(float(x) for x in v), float(fs)


def camera_target(cam, row: int, col: int, rng: R.Rng):
    """cam.rs:64-82 up to the point of the image plane (np_reference.camera_ray without the normalisation)."""
    col_off = f32(col) - f32(cam["W"] // 2)
    row_off = f32(row) - f32(cam["H"] // 2)
    col_mm = f32(f32(col_off + rng.next_f32()) - f32(0.5)) * cam["mm_per_pix_hor"]
    row_mm = f32(f32(row_off + rng.next_f32()) - f32(0.5)) * cam["mm_per_pix_vert"]
    return (cam["img_center_point"] + f32(f32(0.001) * col_mm) * cam["right"]) - f32(f32(0.001) * row_mm) * cam["up"]


def camera_ray_lens(cam, lens, row: int, col: int, rng: R.Rng):
    """(origin, direction) of the lens camera ray of the sample whose stream is `rng`. lens = (lens_u, lens_v, focus_scale)."""
    lens_u, lens_v, fs = np.array(lens[0], f32), np.array(lens[1], f32), f32(lens[2])
    target = camera_target(cam, row, col, rng)
    while True:
        lx = f32(R.F2 * rng.next_f32()) - R.F1
        ly = f32(R.F2 * rng.next_f32()) - R.F1
        if f32(f32(lx * lx) + f32(ly * ly)) < R.F1:
            break
    pos = cam["position"]
    o = pos + (lx * lens_u + ly * lens_v)
    focus = pos + fs * (target - pos)
    return o, R.normalize(focus - o)


def restated_image(cam, sc, opts, lens):
    """(radiance, rgb8) of the whole image, every sample through camera_ray_lens (lens=None: the pinhole camera) and the
    emissive-aware colorize of test_emissive (the reference's colorize for scenes without emitters)."""
    nc, ns = T.np_cam(cam), E.np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    rad = np.zeros((cam.img_height_pix, cam.img_width_pix, 3), f32)
    for row in range(cam.img_height_pix):
        for col in range(cam.img_width_pix):
            color = R.vec(0, 0, 0)
            for s in range(opts.spp):
                rng = R.Rng(opts.seed, row * nc["W"] + col, s)
                o, d = R.camera_ray(nc, row, col, rng) if lens is None else camera_ray_lens(nc, lens, row, col, rng)
                color = color + E.colorize_emissive(o, d, ns, bg, const, opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist))
            rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    rgb = np.vectorize(R.quantise, otypes=[np.uint8])(rad)
    return rad, rgb


def lens_rays(cam, lens, u0, u1, lx, ly):
    """Every pixel's lens ray for given jitter draws u0, u1 ((H, W) arrays) and lens point (lx, ly) (scalars or (H, W)
    arrays of values the draws can give), float32 operation for operation: (H*W, 6)."""
    W, H = cam.img_width_pix, cam.img_height_pix
    col = np.broadcast_to(np.arange(W, dtype=f32)[None, :], (H, W))
    row = np.broadcast_to(np.arange(H, dtype=f32)[:, None], (H, W))
    col_mm = (((col - f32(W // 2)) + u0).astype(f32) - f32(0.5)) * f32(cam.mm_per_pix_hor)
    row_mm = (((row - f32(H // 2)) + u1).astype(f32) - f32(0.5)) * f32(cam.mm_per_pix_vert)
    v = lambda a: np.array(list(a), f32)  # noqa: E731
    right, up, ctr, pos = v(cam.right), v(cam.up), v(cam.img_center_point), v(cam.position)
    target = ((ctr + (f32(0.001) * col_mm)[..., None] * right) - (f32(0.001) * row_mm)[..., None] * up).astype(f32)
    lu, lv, fs = np.array(lens[0], f32), np.array(lens[1], f32), f32(lens[2])
    lx = np.broadcast_to(np.asarray(lx, f32), (H, W))[..., None]
    ly = np.broadcast_to(np.asarray(ly, f32), (H, W))[..., None]
    o = (pos + ((lx * lu).astype(f32) + (ly * lv).astype(f32))).astype(f32)
    focus = (pos + (fs * (target - pos).astype(f32)).astype(f32)).astype(f32)
    d = (focus - o).astype(f32)
    with np.errstate(all="ignore"):
        ln = np.sqrt(((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).astype(f32) + d[..., 2] * d[..., 2]).astype(f32))
        d = (d / ln[..., None]).astype(f32)
    return np.concatenate([o, d], -1).reshape(-1, 6).astype(f32)
