"""Every per-sample feature at once, restated in numpy float32: the one restatement to extend when the next one lands.

It composes the pieces that are pinned one by one -- np_reference (the reference's hot path), test_emissive (emitters, the
constant background), np_lens (the thin lens), np_smooth (shading normals), np_pattern (solid checkers), np_env (the
environment), np_shutter / np_motion (the one draw t, the shifted origin, the moved spheres) and np_animation (the phase) --
in the order include/rbrt_hip.h gives them:

    the camera ray as without a shutter or a motion (jitter draws, lens draws, d = normalize(F - o))
    with a shutter OR a motion: t = the next draw, ONE for both; with a shutter o += t * travel
    with a motion: every sphere centre the path reads is c_i + ((phase + t) * travel_i); without one the phase has no effect
    colorize: an emitter returns its radiance; a lambertian hit attenuates with the colour of the cell its point lies in
    (np_pattern.hit_albedo at hit["point"] of the MOVED scene: the checker stays in world space); a ray that hits nothing
    returns the environment's lookup when the handle has one -- opts.bg and the constant-background flag are then ignored --
    and else the constant background or the gradient.

The device writes this arithmetic out in the trace kernel (megakernel.inl), the short-path stage (short_paths.inl) and the
feature kernel (features.inl), and the tile pass (kernels.hip primary_cull_kernel) bounds it: tests/test_whole_gpu.py holds
all four against this file. tests/test_np_whole.py pins this file: it reduces bit for bit to each single-feature restatement
and to the CPU oracle, and one path through everything is evaluated by hand."""
from __future__ import annotations

import numpy as np

import np_animation as NA
import np_env
import np_lens
import np_motion as NM
import np_pattern
import np_reference as R
import np_smooth as S
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def colorize(o, d, scene, bg, constant_bg, nodes, depth, rng, min_dist=f32(0.001), max_dist=f32(2000.0), trace=None, scatters=None):
    """np_pattern.colorize (the cell's colour on a lambertian hit) with np_env.colorize's miss branch when `nodes` is not None.
    trace: np_pattern.colorize's. scatters: a list that receives the object id of every hit scatter was called for (a path of
    at most one entry is one the short-path stage can finish)."""
    hit = S.scene_hit(scene, o, d, min_dist, max_dist)
    if hit is not None:
        kind, albedo, param = hit["mat"]
        if kind == abi.MAT_EMISSIVE:
            return albedo.copy()
        if depth > 0:
            mat = hit["mat"]
            second = 0
            if kind == abi.MAT_LAMBERTIAN:
                a = np_pattern.hit_albedo(scene.get("patterns"), hit["obj"], albedo, hit["point"])
                second = int(a is not albedo)
                mat = (kind, a, param)
            if scatters is not None:
                scatters.append(int(hit["obj"]))
            ok, att, no, nd = R.scatter(mat, d, hit, rng)
            if ok:
                if trace is not None and kind != abi.MAT_DIELECTRIC:
                    trace.append((int(hit["obj"]), second))
                return att * colorize(no, nd, scene, bg, constant_bg, nodes, depth - 1, rng, min_dist, max_dist, trace, scatters)
        return R.vec(0, 0, 0)
    if nodes is not None:
        return np_env.lookup1(nodes, d)
    if constant_bg:
        return bg.copy()
    t = f32(0.5) * f32(d[1] + R.F1)
    return t * R.vec(1, 1, 1) + f32(R.F1 - t) * bg


def _ray_without_draw(nc, lens, row, col, rng):
    """The camera ray of a handle with neither shutter nor motion: camera_ray_motion's ray, and no draw behind it."""
    return R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)


def restated_image(cam, sc, opts, *, lens=None, shutter=None, travels=None, phase=0.0, nodes=None, pixels=None, traces=None, scatters=None):
    """(radiance, rgb8) of the image of a handle with the shutter `shutter` ((dx, dy, dz) or None), the motion `travels`
    ((n_spheres, 3) or None) at the phase `phase` and the environment `nodes` ((N + 1, N + 1, 3) or None), rendered with
    `lens` (None or (lens_u, lens_v, focus_scale)). `pixels`: only these (row, col), the rest stays 0. traces: a dict that
    receives {(row, col, s): the sample's recorded bounces} (np_pattern.colorize's trace); scatters: likewise, colorize's."""
    nc, ns = T.np_cam(cam), np_pattern.np_scene(sc)
    tv = None if travels is None else NM.travels_of(travels)
    assert tv is None or len(tv) == len(ns["spheres"])
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    lo, hi = f32(opts.min_dist), f32(opts.max_dist)
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            if shutter is None and tv is None:
                o, d = _ray_without_draw(nc, lens, row, col, rng)
                seen = ns
            else:
                o, d, t = NM.camera_ray_motion(nc, lens, shutter, row, col, rng)
                seen = ns if tv is None else NM.scene_at(ns, tv, NA.spheres_time(phase, t))
            tr = [] if traces is not None else None
            sl = [] if scatters is not None else None
            color = color + colorize(o, d, seen, bg, const, nodes, opts.max_depth, rng, lo, hi, tr, sl)
            if traces is not None:
                traces[(row, col, s)] = tr
            if scatters is not None:
                scatters[(row, col, s)] = sl
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


def features(cam, sc, opts, n, *, lens=None, shutter=None, travels=None, phase=0.0, pixels=None):
    """(np_features.Features, motion (H, W, 3)) of rbrt_hip_render_features_motion on the same handle, over n samples: the
    albedo is the colour of each sample's cell at the hit point of the moved scene, the normal the one scatter would use (a
    smooth mesh's shading normal), the motion all +0 without a motion. np_animation.features carries all of it."""
    return NA.features(cam, sc, opts, n, travels, phase, lens=lens, shutter=shutter, pixels=pixels)
