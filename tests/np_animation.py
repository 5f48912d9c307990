"""Animation (include/rbrt_hip.h "Animation") restated in numpy float32 on top of np_motion.py, np_features.py and
np_temporal.py: the phase of a handle's motion, the motion buffer, and the accumulation that follows the spheres.

The contract. A sample's draw t is np_motion's, one draw shared with the shutter, which keeps the raw t. With the phase ph
every sphere centre the sample's path reads is, in float32, unfused,
    s = ph + t,    c_i(s) = c_i + (s * travel_i)
-- np_motion.scene_at at s. The motion buffer is, per pixel, the sum from 0 in sample order of travel_i for a sample that hits
sphere i (zeros for everything else), times 1.0f / float(n). The moving accumulation is np_temporal.accumulate with, for a
surface pixel, P_last = P - (phase_step * (Mv / c)) in P's place.

tests/test_np_animation.py pins this file with scalar evaluations that share no code with it."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import np_env
import np_features
import np_motion as NM
import np_pattern
import np_reference as R
import np_smooth
import np_temporal as NT
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32


def spheres_time(phase, t):
    """s = phase + t: one float32 addition (scalars or arrays of t)."""
    return (f32(phase) + np.asarray(t, f32)).astype(f32)


def scene_at(ns, travels, phase, t):
    """np_motion.scene_at where the phase and the draw put the spheres."""
    return NM.scene_at(ns, travels, spheres_time(phase, t))


def restated_image(cam, sc, opts, travels, phase, lens=None, shutter=None, nodes=None, pixels=None):
    """np_motion.restated_image on a handle whose motion has the phase `phase`: the same rays, the same draw (the shutter moves
    the origin by the raw t), every sample's path on scene_at(phase, its own t)."""
    nc, ns = T.np_cam(cam), np_pattern.np_scene(sc)
    tv = NM.travels_of(travels)
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
            o, d, t = NM.camera_ray_motion(nc, lens, shutter, row, col, rng)
            moved = scene_at(ns, tv, phase, t)
            if nodes is not None:
                color = color + np_env.colorize(o, d, moved, nodes, opts.max_depth, rng, lo, hi)
            else:
                color = color + np_pattern.colorize(o, d, moved, bg, const, opts.max_depth, rng, lo, hi)
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


def primary_rays(cam, seed, n, phase, lens=None, shutter=None, pixels=None):
    """np_motion.primary_rays with the spheres' time of every sample in the draw's place: (rays (P, n, 6), s (P, n))."""
    rays, ts = NM.primary_rays(cam, seed, n, lens=lens, shutter=shutter, pixels=pixels)
    return rays, spheres_time(phase, ts)


def np_hits(sc, rays, ss, travels, lo, hi, points=False):
    """(obj, dist, g) of primary_rays' rays, each against the scene at its own s: np_smooth.scene_hit (np_reference's, with the
    shading normal of a smooth mesh, the normal scatter would use). points: also the hit points p = o + t d, (P, n, 3)."""
    ns = np_pattern.np_scene(sc)
    P, n = ss.shape
    obj, dist, g, pts = np.full((P, n), -1, np.int64), np.zeros((P, n), f32), np.zeros((P, n, 3), f32), np.zeros((P, n, 3), f32)
    for p in range(P):
        for s in range(n):
            hit = np_smooth.scene_hit(NM.scene_at(ns, travels, ss[p, s]), rays[p, s, :3], rays[p, s, 3:], f32(lo), f32(hi))
            if hit is not None:
                obj[p, s], dist[p, s], g[p, s], pts[p, s] = hit["obj"], hit["dist"], hit["normal"], hit["point"]
    return (obj, dist, g, pts) if points else (obj, dist, g)


def cell_albedo(sc, obj, pts, n):
    """The albedo channel over the first n samples with the cell's colour of a patterned object (np_pattern.hit_albedo at the
    hit point; include/rbrt_hip.h "Solid patterns": sample by sample): obj (P, >= n), pts (P, >= n, 3) -> float32 (P, 3), sums
    from 0 in sample order times inv_n, as np_features.from_hits makes them from the table alone."""
    table = np.vstack([np_features.object_albedos(sc), np.zeros((1, 3), f32)])
    patterns = getattr(sc, "pattern_of", None)
    sm = np.zeros((obj.shape[0], 3), f32)
    for s in range(n):
        a = np.zeros((obj.shape[0], 3), f32)
        for p in range(obj.shape[0]):
            if obj[p, s] >= 0:
                a[p] = np_pattern.hit_albedo(patterns, obj[p, s], table[obj[p, s]], pts[p, s])
        sm = sm + a
    return (sm * (f32(1.0) / f32(n))).astype(f32)


def object_travels(sc, travels):
    """[object id] -> what a hit of that object adds to the motion sum: float32 (n_objects + 1, 3). travels None (a handle
    without a motion): zeros. Ids follow np_features.object_albedos; BasicTriangles and meshes add zeros."""
    order = sc.element_order if sc.element_order is not None else (list(range(len(sc.spheres))) + [0x80000000 | i for i in range(len(sc.triangles))])
    out = np.zeros((len(order) + len(sc.meshes) + 1, 3), f32)
    if travels is not None:
        tv = NM.travels_of(travels)
        for k, e in enumerate(order):
            if not e >> 31:
                out[k] = tv[e]
    return out


def motion_from_hits(sc, travels, obj, n):
    """The motion channel over the first n samples: obj (P, >= n) -> float32 (P, 3), sums from 0 in sample order times inv_n."""
    obj = obj[:, :n]
    table = object_travels(sc, travels)
    m = np.where((obj >= 0)[..., None], table[np.where(obj >= 0, obj, 0)], f32(0.0)).astype(f32)
    sm = np.zeros((obj.shape[0], 3), f32)
    for s in range(n):
        sm = sm + m[:, s]
    return (sm * (f32(1.0) / f32(n))).astype(f32)


def features(cam, sc, opts, n, travels, phase=0.0, lens=None, shutter=None, pixels=None):
    """(np_features.Features, motion (H, W, 3)) of a handle with the motion `travels` at `phase`; travels None: a handle without
    a motion (np_features' own rays and no draw -- or, with a shutter, the shutter's rays and its draw; the spheres stay where
    they are whatever the phase), whose motion buffer is all +0. The albedo of a patterned object is its cell's colour."""
    H, W = cam.img_height_pix, cam.img_width_pix
    pix = np_features.all_pixels(cam) if pixels is None else list(pixels)
    if travels is None:
        if shutter is None:
            rays = np_features.primary_rays(cam, opts.seed, n, lens, pix)
        else:
            rays, _ = NM.primary_rays(cam, opts.seed, n, lens=lens, shutter=shutter, pixels=pix)
        ss, tv = np.zeros(rays.shape[:2], f32), np.zeros((len(sc.spheres), 3), f32)
    else:
        rays, ss = primary_rays(cam, opts.seed, n, phase, lens=lens, shutter=shutter, pixels=pix)
        tv = travels
    obj, dist, g, pts = np_hits(sc, rays, ss, tv, opts.min_dist, opts.max_dist, points=True)
    part = np_features.from_hits(sc, obj, dist, g, n)
    if getattr(sc, "pattern_of", None):
        part = part._replace(albedo=cell_albedo(sc, obj, pts, n))
    feat = np_features.scatter_pixels(part, pix, H, W)
    mv = np.zeros((H, W, 3), f32)
    mv[[p[0] for p in pix], [p[1] for p in pix]] = motion_from_hits(sc, travels, obj, n)
    return feat, mv


# ---- the accumulation -------------------------------------------------------------------------------------------------------------
def point_vectors(z, c, cam, cam_prev, Mv=None, phase_step=0.0):
    """v[H][W][3] of the rule: P - position' for a surface pixel -- with Mv, P_last - position', P_last = P - (phase_step * m),
    m = Mv / c per component -- and the centre ray d for a background pixel."""
    z, c = np.ascontiguousarray(z, f32), np.ascontiguousarray(c, f32)
    with np.errstate(all="ignore"):
        d = NT.centre_rays(cam)
        zbar = z / c
        P = NT.vec(cam.position) + (zbar[..., None] * d)
        if Mv is not None:
            m = np.ascontiguousarray(Mv, f32) / c[..., None]
            P = P - (f32(phase_step) * m)
        return np.where((c > 0)[..., None], P - NT.vec(cam_prev.position), d).astype(f32)


def accumulate_from_v(A, B, N, c, v, cam, cam_prev, hist, max_history=32.0, depth=0.05, normal=0.35):
    """Everything of np_temporal.accumulate behind v, statement for statement: the projection, the taps, the sums, the mix."""
    A, B, N, c = (np.ascontiguousarray(x, f32) for x in (A, B, N, c))
    h, w = c.shape
    M, kz, kn = f32(max_history), f32(depth), f32(normal)
    kn2 = kn * kn
    K = NT.camera_constants(cam_prev)
    hx, hy = f32(w // 2), f32(h // 2)
    dot = NT.dot
    with np.errstate(all="ignore"):
        surface = c > 0
        t = K.wn / dot(v, K.n)
        Q = (t[..., None] * v) - K.w
        qr, qu = dot(Q, K.right), dot(Q, K.up)
        a = ((qr * K.uu) - (qu * K.ru)) / K.det
        b = ((qr * K.ru) - (qu * K.rr)) / K.det
        xs = (a / K.sx) + hx
        ys = (b / K.sy) + hy
        projects = (t > 0) & (t < f32(np.inf)) & (xs > f32(-1)) & (xs < f32(w)) & (ys > f32(-1)) & (ys < f32(h))
        xc, yc = np.where(projects, xs, f32(0)), np.where(projects, ys, f32(0))
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
        valid = ws >= NT.VALID_WS
        HA, HB, hl = sa / ws[..., None], sb / ws[..., None], sl / ws
        length = np.where(valid, np.minimum(hl + f32(1), M), f32(1)).astype(f32)
        alpha = (f32(1) / length)[..., None]
        oa = np.where(valid[..., None], HA + (alpha * (A - HA)), A).astype(f32)
        ob = np.where(valid[..., None], HB + (alpha * (B - HB)), B).astype(f32)
    info = SimpleNamespace(surface=surface, projects=projects, xs=xs, ys=ys, i=i, j=j, accepted=accepted, ws=ws, valid=valid)
    return oa, ob, length, info


def accumulate(A, B, N, z, c, cam, cam_prev=None, hist=None, Mv=None, phase_step=0.0, max_history=32.0, depth=0.05, normal=0.35):
    """rbrt_hip_temporal_accumulate_moving: np_temporal.accumulate's signature and result with the motion buffer Mv of this
    frame and the phase step. Mv None, or no history: np_temporal.accumulate itself."""
    if Mv is None or hist is None:
        return NT.accumulate(A, B, N, z, c, cam, cam_prev, hist, max_history=max_history, depth=depth, normal=normal)
    v = point_vectors(z, c, cam, cam_prev, Mv, phase_step)
    oa, ob, length, info = accumulate_from_v(A, B, N, c, v, cam, cam_prev, hist, max_history, depth, normal)
    return oa, ob, length, NT.History(oa, ob, length, N, z, c), info
