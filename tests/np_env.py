"""Environment lighting (rbrt_hip.h rbrt_environment_t) restated in numpy, on top of np_smooth.py / np_lens.py.

The lookup (include/rbrt_hip.h "Environment lighting"), float32, unfused, in this order, for the direction d of
the ray that hit nothing, as traced:
    s = (|dx| + |dy|) + |dz|;  p = d / s
    py >= 0: (u, v) = (px, pz);  else u = (1 - |pz|) * (px >= 0 ? 1 : -1), v = (1 - |px|) * (pz >= 0 ? 1 : -1)
    x = ((u * 0.5) + 0.5) * N;  i = x >= 0 ? min(uint(floor(x)), N - 1) : 0;  fx = x - i;   (y, j, fy likewise from v)
    top = E[j][i] + fx * (E[j][i+1] - E[j][i]);  bot likewise from row j + 1;  L = top + fy * (bot - top)
It takes the place of the background in np_smooth's colorize; everything else (the lens, smooth meshes, emitters) is theirs.

Also here: the host's conversion of a latitude/longitude image into nodes, in float64 (rbrt_amd/host/environment.cpp), and
seeded maps for the tests."""
from __future__ import annotations

import math

import numpy as np

import np_lens
import np_reference as R
import np_smooth as S
import test_np_reference as T

f32 = np.float32


# ---- the lookup --------------------------------------------------------------------------------------------------------
def cell(dirs, n):
    """(i, j, fx, fy) of directions (M, 3), float32 operation for operation."""
    d = np.ascontiguousarray(dirs, f32).reshape(-1, 3)
    with np.errstate(all="ignore"):
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        s = (np.abs(dx) + np.abs(dy)).astype(f32) + np.abs(dz)
        px, py, pz = (dx / s).astype(f32), (dy / s).astype(f32), (dz / s).astype(f32)
        one, mone = f32(1.0), f32(-1.0)
        ul = (one - np.abs(pz)).astype(f32) * np.where(px >= 0, one, mone).astype(f32)
        vl = (one - np.abs(px)).astype(f32) * np.where(pz >= 0, one, mone).astype(f32)
        upper = py >= 0
        u, v = np.where(upper, px, ul).astype(f32), np.where(upper, pz, vl).astype(f32)
        fn = f32(n)
        x = ((u * f32(0.5)).astype(f32) + f32(0.5)).astype(f32) * fn
        y = ((v * f32(0.5)).astype(f32) + f32(0.5)).astype(f32) * fn

        def index(t):
            fl = np.floor(t)
            k = np.where(t >= 0, np.minimum(np.where(t >= 0, fl, 0.0), float(n - 1)), 0.0)  # (a NaN compares false: 0)
            return k.astype(np.int64)

        i, j = index(x), index(y)
        fx, fy = (x - i.astype(f32)).astype(f32), (y - j.astype(f32)).astype(f32)
    return i, j, fx, fy


def lookup(nodes, dirs):
    """The radiance of the map `nodes` (N + 1, N + 1, 3) for directions (M, 3): float32 (M, 3)."""
    E = np.ascontiguousarray(nodes, f32)
    n = E.shape[0] - 1
    i, j, fx, fy = cell(dirs, n)
    fx, fy = fx[:, None], fy[:, None]
    with np.errstate(all="ignore"):
        a, b, c, e = E[j, i], E[j, i + 1], E[j + 1, i], E[j + 1, i + 1]
        top = (a + (fx * (b - a).astype(f32)).astype(f32)).astype(f32)
        bot = (c + (fx * (e - c).astype(f32)).astype(f32)).astype(f32)
        return (top + (fy * (bot - top).astype(f32)).astype(f32)).astype(f32)


def lookup1(nodes, d):
    return lookup(nodes, np.asarray(d, f32)[None, :])[0]


# ---- images ------------------------------------------------------------------------------------------------------------
def colorize(o, d, scene, nodes, depth, rng, min_dist=f32(0.001), max_dist=f32(2000.0)):
    """np_smooth.colorize with the miss branch replaced by the lookup."""
    hit = S.scene_hit(scene, o, d, min_dist, max_dist)
    if hit is not None:
        kind, albedo, _ = hit["mat"]
        if kind == S.abi.MAT_EMISSIVE:
            return albedo.copy()
        if depth > 0:
            ok, att, no, nd = R.scatter(hit["mat"], d, hit, rng)
            if ok:
                return att * colorize(no, nd, scene, nodes, depth - 1, rng, min_dist, max_dist)
        return R.vec(0, 0, 0)
    return lookup1(nodes, d)


def restated_image(cam, sc, opts, nodes, lens=None, pixels=None):
    """(radiance, rgb8) of the image under the environment `nodes`; lens: None or (lens_u, lens_v, focus_scale); `pixels`:
    only these (row, col), the rest stays 0."""
    nc, ns = T.np_cam(cam), S.np_scene(sc)
    H, W = cam.img_height_pix, cam.img_width_pix
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
            color = color + colorize(o, d, ns, nodes, opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist))
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


# ---- the host's conversion, float64 --------------------------------------------------------------------------------------
def node_directions(n):
    """Unit directions (n + 1, n + 1, 3) of the nodes, float64: (u, v) = ((2i - N) / N, (2j - N) / N) unfolded."""
    k = (2.0 * np.arange(n + 1, dtype=np.float64) - float(n)) / float(n)
    u, v = np.meshgrid(k, k)  # u along columns (i), v along rows (j)
    py = (1.0 - np.abs(u)) - np.abs(v)
    lower = ~(py >= 0.0)
    px = np.where(lower, (1.0 - np.abs(v)) * np.where(u >= 0.0, 1.0, -1.0), u) + 0.0
    pz = np.where(lower, (1.0 - np.abs(u)) * np.where(v >= 0.0, 1.0, -1.0), v) + 0.0
    ln = np.sqrt((px * px + py * py) + pz * pz)
    return np.stack([px / ln, py / ln, pz / ln], -1)


def nodes_from_latlong(img, n, rotation_deg=0.0, intensity=1.0):
    """The nodes (n + 1, n + 1, 3) float32 of a latitude/longitude image (H, W, 3; top row = +y, middle column = -z)."""
    img = np.asarray(img, np.float64)
    hs, ws = img.shape[0], img.shape[1]
    d = node_directions(n)
    phi = np.arctan2(d[..., 0], -d[..., 2]) - rotation_deg * math.pi / 180.0
    t = 0.5 + phi / (2.0 * math.pi)
    u_ll = t - np.floor(t)
    v_ll = np.arccos(np.clip(d[..., 1], -1.0, 1.0)) / math.pi
    sx, sy = u_ll * ws - 0.5, v_ll * hs - 0.5
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = (sx - x0f)[..., None], (sy - y0f)[..., None]
    x0 = np.mod(x0f.astype(np.int64), ws)
    x1 = np.mod(x0 + 1, ws)
    y0 = np.clip(y0f.astype(np.int64), 0, hs - 1)
    y1 = np.clip(y0f.astype(np.int64) + 1, 0, hs - 1)
    top = img[y0, x0] + fx * (img[y0, x1] - img[y0, x0])
    bot = img[y1, x0] + fx * (img[y1, x1] - img[y1, x0])
    return np.maximum((top + fy * (bot - top)) * intensity, 0.0).astype(f32)


# ---- maps for the tests ----------------------------------------------------------------------------------------------------
def noise_map(n, seed):
    """White noise in [0, 8]: a wrong index or a swapped axis shows in one pixel. (The identified boundary nodes differ: the
    lookup does not care.)"""
    return np.random.default_rng(seed).uniform(0.0, 8.0, (n + 1, n + 1, 3)).astype(f32)


def smooth_map(n, seed):
    """A smooth map in [0, 8]: a few seeded lobes on the sphere, sampled at the nodes' directions (continuous over the fold)."""
    rng = np.random.default_rng(seed)
    d = node_directions(n)
    out = np.full((n + 1, n + 1, 3), 0.25)
    for _ in range(5):
        c = rng.normal(size=3)
        c /= np.linalg.norm(c)
        out = out + rng.uniform(0.2, 1.5, 3) * np.exp(rng.uniform(1.0, 6.0) * (d @ c - 1.0))[..., None]
    return np.clip(out, 0.0, 8.0).astype(f32)


def write_pfm(path, img, little=True):
    """A colour PFM of img (H, W, 3), top row first in `img`, bottom row first in the file."""
    img = np.ascontiguousarray(img, f32)
    h, w, _ = img.shape
    with open(path, "wb") as f:
        f.write(f"PF\n{w} {h}\n{'-1.0' if little else '1.0'}\n".encode())
        f.write(img[::-1].astype("<f4" if little else ">f4").tobytes())
