"""Moving meshes (rbrt_hip_scene_set_mesh_motion) restated in numpy float32, on top of np_motion.py, np_animation.py,
np_pattern.py, np_env.py and np_smooth.py: the per-mesh origin, Scene::hit with it, colorize, whole images and the feature
buffers.

The contract (include/rbrt_hip.h "Moving meshes"): a handle with a shutter, a sphere motion or a mesh
motion makes the one draw t; the time is s = phase + t; a handle with a mesh motion and no sphere motion is one whose sphere
travels are all zero. Wherever a path tests mesh m it reads, in float32, unfused, a product and a difference per component,
    o_m = o - (s * w_m)
and everything mesh.rs does with the ray is done with (o_m, d): the box gate, the triangle scan, p_m = o_m + t d,
dist = length(o_m - p_m), the distance window, a smooth mesh's barycentrics. dist competes with the closest hit so far as it
always did (strict <, elements first, meshes in order), and the path continues from p = o + t d with its own o, which is
also where a solid checker is evaluated.

tests/test_np_mesh_motion.py pins this file with scalar evaluations that share no code with it."""
from __future__ import annotations

import numpy as np

import np_animation as NA
import np_env
import np_features
import np_motion as NM
import np_pattern
import np_reference as R
import np_smooth as S
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def origin_at(o, travel, s):
    """o_m: a product and a difference per component, float32."""
    return (np.asarray(o, f32) - (f32(s) * np.asarray(travel, f32)).astype(f32)).astype(f32)


def scene_hit(scene, o, d, min_dist, max_dist, mesh_travels, s):
    """np_smooth.scene_hit with the per-mesh origin: the elements as they are (np_reference.scene_hit of the scene without its
    meshes), then every mesh in order from its own origin, strict `<` on dist. The hit's point is o + t d with the world o."""
    best = R.scene_hit(dict(scene, meshes=[]), o, d, min_dist, max_dist)
    closest = np.finfo(f32).max if best is None else best["dist"]
    n_elem = S.n_elements(scene)
    for k, mesh in enumerate(scene["meshes"]):
        om = origin_at(o, mesh_travels[k], s)
        h = R.mesh_hit(mesh, om, d, min_dist, max_dist)
        if h is not None and h[2] < closest:
            closest = h[2]
            best = dict(point=R.point_at(o, d, h[3]), normal=S.shading_normal(mesh, h[4], om, d), dist=h[2], t=h[3], mat=mesh["mat"],
                        obj=n_elem + k, tri=h[4])
    return best


def colorize(o, d, scene, bg, constant_bg, nodes, depth, rng, mesh_travels, s, min_dist=f32(0.001), max_dist=f32(2000.0), scatters=None):
    """np_whole.colorize -- an emitter's radiance, the cell's colour on a lambertian hit, the environment for a miss when
    `nodes` is not None -- on this file's scene_hit. `scene`: the spheres already where s puts them (np_motion.scene_at).
    scatters: a list that receives the object id of every hit scatter was called for."""
    hit = scene_hit(scene, o, d, min_dist, max_dist, mesh_travels, s)
    if hit is not None:
        kind, albedo, param = hit["mat"]
        if kind == abi.MAT_EMISSIVE:
            return albedo.copy()
        if depth > 0:
            mat = hit["mat"]
            if kind == abi.MAT_LAMBERTIAN:
                mat = (kind, np_pattern.hit_albedo(scene.get("patterns"), hit["obj"], albedo, hit["point"]), param)
            if scatters is not None:
                scatters.append(int(hit["obj"]))
            ok, att, no, nd = R.scatter(mat, d, hit, rng)
            if ok:
                return att * colorize(no, nd, scene, bg, constant_bg, nodes, depth - 1, rng, mesh_travels, s, min_dist, max_dist, scatters)
        return R.vec(0, 0, 0)
    if nodes is not None:
        return np_env.lookup1(nodes, d)
    if constant_bg:
        return bg.copy()
    t = f32(0.5) * f32(d[1] + R.F1)
    return t * R.vec(1, 1, 1) + f32(R.F1 - t) * bg


def mesh_travels_of(travels):
    return np.asarray(travels, f32).reshape(-1, 3)


def restated_image(cam, sc, opts, mesh_travels, *, travels=None, phase=0.0, lens=None, shutter=None, nodes=None, pixels=None, scatters=None):
    """(radiance, rgb8) of the image of a handle with the mesh motion `mesh_travels` ((n_meshes, 3)), the sphere motion
    `travels` ((n_spheres, 3) or None: all zeros), the phase, the shutter ((dx, dy, dz) or None) and the environment `nodes`,
    rendered with `lens`. `pixels`: only these (row, col), the rest stays 0. scatters: a dict that receives
    {(row, col, s): colorize's scatters}."""
    nc, ns = T.np_cam(cam), np_pattern.np_scene(sc)
    mw = mesh_travels_of(mesh_travels)
    assert len(mw) == len(ns["meshes"])
    tv = np.zeros((len(ns["spheres"]), 3), f32) if travels is None else NM.travels_of(travels)
    assert len(tv) == len(ns["spheres"])
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    lo, hi = f32(opts.min_dist), f32(opts.max_dist)
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for k in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, k)
            o, d, t = NM.camera_ray_motion(nc, lens, shutter, row, col, rng)
            s = NA.spheres_time(phase, t)
            sl = [] if scatters is not None else None
            color = color + colorize(o, d, NM.scene_at(ns, tv, s), bg, const, nodes, opts.max_depth, rng, mw, s, lo, hi, sl)
            if scatters is not None:
                scatters[(row, col, k)] = sl
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


def np_hits(sc, rays, ss, travels, mesh_travels, lo, hi):
    """(obj, dist, g, points) of np_animation.primary_rays' rays, each against the scene at its own s: this file's scene_hit."""
    ns = np_pattern.np_scene(sc)
    mw = mesh_travels_of(mesh_travels)
    P, n = ss.shape
    obj, dist, g, pts = np.full((P, n), -1, np.int64), np.zeros((P, n), f32), np.zeros((P, n, 3), f32), np.zeros((P, n, 3), f32)
    for p in range(P):
        for k in range(n):
            hit = scene_hit(NM.scene_at(ns, travels, ss[p, k]), rays[p, k, :3], rays[p, k, 3:], f32(lo), f32(hi), mw, ss[p, k])
            if hit is not None:
                obj[p, k], dist[p, k], g[p, k], pts[p, k] = hit["obj"], hit["dist"], hit["normal"], hit["point"]
    return obj, dist, g, pts


def object_travels(sc, travels, mesh_travels):
    """np_animation.object_travels with the meshes' rows filled: [object id] -> what a hit of it adds to the motion sum."""
    out = NA.object_travels(sc, travels)
    n_elem = len(out) - 1 - len(sc.meshes)
    out[n_elem:n_elem + len(sc.meshes)] = mesh_travels_of(mesh_travels)
    return out


def features(cam, sc, opts, n, mesh_travels, travels=None, phase=0.0, lens=None, shutter=None, pixels=None):
    """(np_features.Features, motion (H, W, 3)) of rbrt_hip_render_features_motion on a handle with the mesh motion: depth is
    the rule's dist, the normal comes from (o_m, d), the albedo of a patterned object is its cell's colour at the world
    point, and a sample that hits mesh m adds w_m to the motion sum."""
    H, W = cam.img_height_pix, cam.img_width_pix
    pix = np_features.all_pixels(cam) if pixels is None else list(pixels)
    tv = np.zeros((len(sc.spheres), 3), f32) if travels is None else NM.travels_of(travels)
    rays, ss = NA.primary_rays(cam, opts.seed, n, phase, lens=lens, shutter=shutter, pixels=pix)
    obj, dist, g, pts = np_hits(sc, rays, ss, tv, mesh_travels, opts.min_dist, opts.max_dist)
    part = np_features.from_hits(sc, obj, dist, g, n)
    if getattr(sc, "pattern_of", None):
        part = part._replace(albedo=NA.cell_albedo(sc, obj, pts, n))
    feat = np_features.scatter_pixels(part, pix, H, W)
    table = object_travels(sc, travels, mesh_travels)
    m = np.where((obj >= 0)[..., None], table[np.where(obj >= 0, obj, 0)], f32(0.0)).astype(f32)
    sm = np.zeros((len(pix), 3), f32)
    for k in range(n):
        sm = sm + m[:, k]
    mv = np.zeros((H, W, 3), f32)
    mv[[p[0] for p in pix], [p[1] for p in pix]] = (sm * (f32(1.0) / f32(n))).astype(f32)
    return feat, mv
