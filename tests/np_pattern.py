"""Solid patterns (rbrt_hip.h rbrt_scene_patterns_t) restated in numpy float32, on top of np_smooth.py.

The rule (include/rbrt_hip.h, DESIGN.md "Solid patterns"): a lambertian object may carry a checker (albedo2, origin, size).
With inv = 1.0f / size, at the hit point p = o + t d that scatter uses, per component c, in float32, unfused:
    t_c = (p_c - origin_c) * inv
    u_c = min(max(t_c, -1e9f), 1e9f)      (fmax / fmin: a NaN counts as -1e9)
    k_c = int32(floor(u_c))
    odd = (k_x ^ k_y ^ k_z) & 1
and the hit attenuates the path with albedo2 in an odd cell, with the material's albedo in an even one. Everything else is
np_smooth's colorize. The oracle does not know the pattern: tests/test_np_pattern.py pins this file from sides that share
no code with it."""
from __future__ import annotations

import numpy as np

import np_features
import np_lens
import np_reference as R
import np_smooth as S
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32
LO, HI = f32(-1e9), f32(1e9)


# ---- the rule ----------------------------------------------------------------------------------------------------------
def cells(p, origin, size):
    """k of points p (..., 3): int32 (..., 3)."""
    p, origin = np.asarray(p, f32), np.asarray(origin, f32)
    with np.errstate(all="ignore"):
        inv = f32(f32(1.0) / f32(size))
        t = ((p - origin).astype(f32) * inv).astype(f32)
        u = np.fmin(np.fmax(t, LO), HI)
        return np.floor(u).astype(np.int32)


def odd(p, origin, size):
    """1 where p lies in an odd cell, else 0: int32 (...)."""
    k = cells(p, origin, size)
    return (k[..., 0] ^ k[..., 1] ^ k[..., 2]) & 1


def pattern_fields(pt):
    """(albedo2, origin, size) of an abi.Pattern, as float32."""
    return np.array(list(pt.albedo2), f32), np.array(list(pt.origin), f32), f32(pt.size)


def hit_albedo(patterns, obj, albedo, p):
    """The albedo a hit of object `obj` at p attenuates with; patterns: {object id: abi.Pattern}."""
    pt = patterns.get(int(obj)) if patterns else None
    if pt is None or pt.kind == abi.PATTERN_NONE:
        return albedo
    a2, origin, size = pattern_fields(pt)
    return a2 if int(odd(p, origin, size)) else albedo


# ---- colorize and the image -----------------------------------------------------------------------------------------------
def colorize(o, d, scene, bg, constant_bg, depth, rng, min_dist=f32(0.001), max_dist=f32(2000.0), trace=None):
    """np_smooth.colorize with the hit's albedo replaced at hit["point"]. trace: a list that receives, per recorded bounce
    (a scatter that succeeded and is no dielectric's), (object id, 1 if the second colour attenuated else 0)."""
    hit = S.scene_hit(scene, o, d, min_dist, max_dist)
    if hit is not None:
        kind, albedo, param = hit["mat"]
        if kind == abi.MAT_EMISSIVE:
            return albedo.copy()
        if depth > 0:
            mat = hit["mat"]
            second = 0
            if kind == abi.MAT_LAMBERTIAN:
                a = hit_albedo(scene.get("patterns"), hit["obj"], albedo, hit["point"])
                second = int(a is not albedo)
                mat = (kind, a, param)
            ok, att, no, nd = R.scatter(mat, d, hit, rng)
            if ok:
                if trace is not None and kind != abi.MAT_DIELECTRIC:
                    trace.append((int(hit["obj"]), second))
                return att * colorize(no, nd, scene, bg, constant_bg, depth - 1, rng, min_dist, max_dist, trace)
        return R.vec(0, 0, 0)
    if constant_bg:
        return bg.copy()
    t = f32(0.5) * f32(d[1] + R.F1)
    return t * R.vec(1, 1, 1) + f32(R.F1 - t) * bg


def np_scene(sc):
    """np_smooth.np_scene with the scene's patterns under 'patterns'."""
    ns = S.np_scene(sc)
    ns["patterns"] = dict(getattr(sc, "pattern_of", {}) or {})
    return ns


def restated_image(cam, sc, opts, pixels=None, traces=None, lens=None):
    """(radiance, rgb8) of the image by the restatement; `pixels`: only these (row, col), the rest stays 0. traces: a dict
    that receives {(row, col, s): the sample's recorded bounces} (colorize's trace). lens: (lens_u, lens_v, focus_scale) of a
    thin-lens render (np_lens.camera_ray_lens), None for the pinhole camera."""
    nc, ns = T.np_cam(cam), np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
            tr = [] if traces is not None else None
            color = color + colorize(o, d, ns, bg, const, opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist), tr)
            if traces is not None:
                traces[(row, col, s)] = tr
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


# ---- the hook and the feature buffers -------------------------------------------------------------------------------------
def surface_albedo(oracle, sc, rays, min_dist=0.001, max_dist=2000.0):
    """What rbrt_hip_debug_surface_albedo documents, from the oracle's Scene::hit: float32 (n, 3), NaN for a miss."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    t, obj, _, _ = oracle.trace_rays(sc, rays, min_dist, max_dist)
    table = np_features.object_albedos(sc)
    out = np.full((len(rays), 3), np.nan, f32)
    for i in range(len(rays)):
        if obj[i] < 0:
            continue
        p = (rays[i, :3] + f32(t[i]) * rays[i, 3:]).astype(f32)
        out[i] = hit_albedo(getattr(sc, "pattern_of", None), obj[i], table[obj[i]], p)
    return out


def feature_albedo(oracle, cam, sc, opts, n, pixels=None):
    """The albedo buffer and the object buffer of rbrt_hip_render_features with the cell's colour per sample: float32
    (H, W, 3), int32 (H, W). Also returns, per listed pixel, whether its samples saw both colours of a patterned object."""
    H, W = cam.img_height_pix, cam.img_width_pix
    pix = np_features.all_pixels(cam) if pixels is None else list(pixels)
    rays = np_features.primary_rays(cam, opts.seed, n, None, pix)
    a = surface_albedo(oracle, sc, rays.reshape(-1, 6), opts.min_dist, opts.max_dist).reshape(len(pix), n, 3)
    _, obj, _, _ = oracle.trace_rays(sc, np.ascontiguousarray(rays.reshape(-1, 6)), opts.min_dist, opts.max_dist)
    obj = obj.reshape(len(pix), n)
    a = np.where(obj[..., None] >= 0, a, f32(0.0)).astype(f32)
    acc = np.zeros((len(pix), 3), f32)
    for s in range(n):
        acc = acc + a[:, s]
    acc = acc * f32(f32(1.0) / f32(n))
    albedo, first = np.zeros((H, W, 3), f32), np.full((H, W), -1, np.int32)
    straddles = []
    for k, (r, c) in enumerate(pix):
        albedo[r, c], first[r, c] = acc[k], obj[k, 0]
        same_obj = np.all(obj[k] == obj[k, 0]) and obj[k, 0] in (getattr(sc, "pattern_of", None) or {})
        straddles.append(bool(same_obj and len({tuple(x) for x in a[k].tolist()}) > 1))
    return albedo, first, straddles
