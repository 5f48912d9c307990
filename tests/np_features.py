"""The feature buffers (include/rbrt_hip.h "Feature buffers") restated in numpy float32.

The rule: for pixel (row, col) and sample s in 0..n-1 the primary ray is the render's own -- the stream keyed
(seed, row * W + col, s) draws the column jitter, then the row jitter, then (with a lens) the lens draws -- and its closest
hit is Scene::hit in the window [min_dist, max_dist]. Per sample
    a ray that hits nothing:  albedo (0, 0, 0), normal (0, 0, 0), depth 0, coverage 0
    a hit of object k:        albedo = the material's albedo ((1, 1, 1) for a dielectric; an emitter's radiance),
                              normal = normalize(g), g the normal the scatter pass would use (three divisions by the length),
                              depth = dist_from_ray_orig, coverage 1
and every channel is a sum from 0 in sample order, times 1.0f / float(n). object = the object id of sample 0, or -1.

The rays come from np_reference.Rng with np_reference.camera_ray or np_lens.camera_ray_lens; the hits from the CPU oracle
(trace_rays and shading_normals, one batch each); the table and the sums are numpy float32. tests/test_np_features.py pins it
from two sides that share no code with it: the oracle's render of an emitters-only scene, and the pure-numpy Scene::hit."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import np_lens
import np_reference as R
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32
Features = namedtuple("Features", "albedo normal depth coverage object")


def all_pixels(cam):
    return [(r, c) for r in range(cam.img_height_pix) for c in range(cam.img_width_pix)]


def primary_rays(cam, seed, n, lens=None, pixels=None):
    """The primary rays of samples 0..n-1 of every pixel (or of `pixels`, a list of (row, col)): float32 (P, n, 6). A sample's
    stream does not depend on n: the rays of a smaller n are the first of a larger one's."""
    nc = T.np_cam(cam)
    W = cam.img_width_pix
    pix = all_pixels(cam) if pixels is None else list(pixels)
    rays = np.zeros((len(pix), n, 6), f32)
    for k, (row, col) in enumerate(pix):
        for s in range(n):
            rng = R.Rng(seed, row * W + col, s)
            o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
            rays[k, s, :3], rays[k, s, 3:] = o, d
    return rays


def object_albedos(sc):
    """[object id] -> what a hit of that object adds to the albedo sum: float32 (n_objects, 3). Ids follow Scene::elements
    (element_order; without one the spheres, then the BasicTriangles), the meshes behind them."""
    order = sc.element_order if sc.element_order is not None else (list(range(len(sc.spheres))) + [0x80000000 | i for i in range(len(sc.triangles))])
    mats = [sc.triangles[e & 0x7FFFFFFF][1] if e >> 31 else sc.spheres[e][2] for e in order] + [md.struct.mat for md in sc.meshes]
    out = np.zeros((len(mats), 3), f32)
    for k, m in enumerate(mats):
        out[k] = (1.0, 1.0, 1.0) if m.kind == abi.MAT_DIELECTRIC else tuple(m.albedo)
    return out


def hits(oracle, sc, rays, min_dist, max_dist):
    """(obj, dist, g) of a batch of rays (…, 6): the oracle's Scene::hit and scatter normal, shaped like the batch."""
    flat = np.ascontiguousarray(rays, f32).reshape(-1, 6)
    _, obj, _, dist = oracle.trace_rays(sc, flat, min_dist, max_dist)
    g = oracle.shading_normals(sc, flat, min_dist, max_dist)
    lead = rays.shape[:-1]
    return obj.reshape(lead), dist.reshape(lead), g.reshape(lead + (3,))


def from_hits(sc, obj, dist, g, n):
    """The table and the sums over the first n samples: obj, dist (P, >= n), g (P, >= n, 3) -> five arrays of P pixels."""
    obj, dist, g = obj[:, :n], dist[:, :n], g[:, :n]
    hit = obj >= 0
    table = np.vstack([object_albedos(sc), np.zeros((1, 3), f32)])  # (a row behind the objects: an empty scene has a table, too)
    a = np.where(hit[..., None], table[np.where(hit, obj, 0)], f32(0.0)).astype(f32)
    with np.errstate(all="ignore"):
        ln = np.sqrt(((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]).astype(f32) + g[..., 2] * g[..., 2]).astype(f32))
        nrm = np.where(hit[..., None], (g / ln[..., None]).astype(f32), f32(0.0)).astype(f32)  # no guard: a zero g gives NaN
    z = np.where(hit, dist, f32(0.0)).astype(f32)
    c = np.where(hit, f32(1.0), f32(0.0)).astype(f32)
    P = obj.shape[0]
    sa, sn, sz, sc_ = np.zeros((P, 3), f32), np.zeros((P, 3), f32), np.zeros(P, f32), np.zeros(P, f32)
    with np.errstate(all="ignore"):
        for s in range(n):  # sums from 0, in sample order
            sa, sn, sz, sc_ = sa + a[:, s], sn + nrm[:, s], sz + z[:, s], sc_ + c[:, s]
        inv_n = f32(1.0) / f32(n)
        return Features(sa * inv_n, sn * inv_n, sz * inv_n, sc_ * inv_n, obj[:, 0].astype(np.int32))


def features(oracle, cam, sc, opts, n, lens=None, pixels=None, rays=None):
    """The five buffers of the image: albedo, normal float32 (H, W, 3), depth, coverage float32 (H, W), object int32 (H, W).
    `pixels`: only these (row, col); the rest stays 0 (object: -1). `rays`: primary_rays(...) of at least n samples for the
    same camera, seed, lens and pixels, when the caller has them already."""
    H, W = cam.img_height_pix, cam.img_width_pix
    pix = all_pixels(cam) if pixels is None else list(pixels)
    if rays is None:
        rays = primary_rays(cam, opts.seed, n, lens, pix)
    obj, dist, g = hits(oracle, sc, rays[:, :n], opts.min_dist, opts.max_dist)
    part = from_hits(sc, obj, dist, g, n)
    return scatter_pixels(part, pix, H, W)


def emitter_scene(oracle):
    """A scene made only of emitters -- two spheres, a BasicTriangle in front of them in the element order and a small mesh --
    for the identity: rendered with the constant background 0 at spp = n, its radiance is its albedo buffer bit for bit."""
    import scenes
    EM = abi.MAT_EMISSIVE
    spheres = [((-2.5, 2.9, -15.0), 3.0, abi.material(EM, (2.0, 1.5, 0.5))), ((1.5, 1.25, -9.0), 1.5, abi.material(EM, (0.3, 4.0, 1.0)))]
    tris = [(((-1.5, 0.3, -5.5), (1.0, 0.4, -6.0), (-0.2, 2.6, -6.5)), abi.material(EM, (5.0, 0.2, 0.1)))]
    mesh = scenes.standin_mesh(oracle, 203, 45.0, (5.0, -1.8, -12.5), (0.0, 0.0, 0.0), abi.material(EM, (0.7, 0.8, 9.0)))
    return abi.SceneData(spheres=spheres, meshes=[mesh], triangles=tris, element_order=[0, scenes.T | 0, 1])


def emitter_opts(n, seed=3, **kw):
    return abi.default_opts(spp=n, seed=seed, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0), **kw)


def scatter_pixels(part, pix, H, W):
    """Per-pixel arrays of the listed pixels -> whole images."""
    out = Features(np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32), np.zeros((H, W), f32),
                   np.full((H, W), -1, np.int32))
    rows, cols = np.array([p[0] for p in pix], int), np.array([p[1] for p in pix], int)
    for dst, src in zip(out, part):
        dst[rows, cols] = src
    return out
