"""Geometry and rays aimed where the BVH's culling pad (kernels.hip make_cull / child_key) is tight:
shared by the CPU walk of test_bvh_host.py and the GPU tests of test_cull_families.py.

Rays are aimed at the corners, edge points and face points of the decoded tree's node boxes and at the triangles' vertices
and edge points; some graze (one direction component about 1e-6 of the others); origins sit about 1.5 eps, R, 60 R and
1e4 R from the point aimed at (R: the mesh's bounding radius); direction lengths are 0.2, 1 and 3."""
from __future__ import annotations

import numpy as np

from rbrt_amd import abi, standin

EPS = 0.001  # the reference's minimum hit distance (Scene::hit's t_min)
NO_CHILD = -2 ** 31


def far_mesh(oracle, offset):
    """Small triangles (a 1500-triangle stand-in, about 3.5 across) translated far from the origin, where the pad's |o|inf term
    dominates."""
    return oracle.mesh_prep(standin.triangles(1500, "rough"), 15.0, (0.0, 0.0, 0.0), offset,
                            abi.material(abi.MAT_LAMBERTIAN, (0.6, 0.5, 0.4)))


def slivers(oracle, eps=EPS):
    """Long thin triangles a few eps wide, in every orientation: Moller-Trumbore's |a| is barely above eps for many rays."""
    rng = np.random.default_rng(21)
    n = 1200
    p = rng.uniform(-2, 2, (n, 3))
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    w = rng.normal(size=(n, 3))
    w -= (w * u).sum(1, keepdims=True) * u
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    length = rng.uniform(0.5, 3.0, (n, 1))
    width = eps * rng.uniform(1.2, 4.0, (n, 1))
    tris = np.stack([p, p + u * length, p + u * length * 0.5 + w * width], 1)
    return oracle.mesh_prep(tris.astype(np.float32), mat=abi.material(abi.MAT_METAL, (0.8, 0.8, 0.9), 0.1))


def integer_grid(oracle):
    """Axis-aligned unit squares on integer planes (z = 0, -2, -4 and x = 3), with coplanar duplicates and overlapping
    copies of some of them placed thousands of indices away: equal t in different leaves, which the (t, index) rule has
    to resolve the way the scan does."""
    quads = []
    for z in (0, -2, -4):
        for i in range(-8, 8):
            for j in range(-8, 8):
                quads.append([[i, j, z], [i + 1, j, z], [i + 1, j + 1, z]])
                quads.append([[i, j, z], [i + 1, j + 1, z], [i, j + 1, z]])
    for i in range(-8, 8):
        for j in range(-4, 0):
            quads.append([[3, i, j], [3, i + 1, j], [3, i + 1, j + 1]])
    base = np.array(quads, np.float32)
    rng = np.random.default_rng(22)
    pick = rng.choice(len(base), 300, replace=False)
    dup = base[pick]                                   # the same triangle again
    over = base[pick[:150]].copy()
    over[:, :, :2] += np.float32(0.5)                  # overlapping, same plane: exact t ties inside the overlap
    tris = np.concatenate([base, rng.permutation(np.concatenate([dup, over]))])
    return oracle.mesh_prep(tris, mat=abi.material(abi.MAT_LAMBERTIAN, (0.3, 0.7, 0.3)))


def families(oracle):
    """name -> (MeshData, lab environment for the host builder)."""
    out = {f"far{o[0]:+.0e}": (far_mesh(oracle, o), {}) for o in ((1e3, -40.0, 2.0), (-3e4, 1e4, -2e4), (1e5, 1e5, -1e5))}
    out["slivers"] = (slivers(oracle), {})
    out["grid"] = (integer_grid(oracle), {})
    out["rough_spatial"] = (oracle.mesh_prep(standin.triangles(2500, "rough"), 4.0, (0.0, 0.0, 0.0), (0.5, -0.25, -6.0),
                                             abi.material(abi.MAT_DIELECTRIC, (0, 0, 0), 1.5)), {"RBRT_BVH_SPATIAL": "0.6"})
    return out


def rough_mesh(oracle, scale):
    """The 1500-triangle rough stand-in, about 0.23 * scale across, centred near (0.3, -0.2, 0.1) * scale."""
    return oracle.mesh_prep(standin.triangles(1500, "rough"), scale, (0.0, 0.0, 0.0), (0.3 * scale, -0.2 * scale, 0.1 * scale),
                            abi.material(abi.MAT_LAMBERTIAN, (0.6, 0.5, 0.4)))


def radius(md):
    return float(np.linalg.norm((md.bbox_hi - md.bbox_lo).astype(np.float64)) / 2)


def sweep(oracle):
    """name -> (MeshData, lab environment for the host builder, min_dist, max_dist, direction lengths): the culling pad over
    the window the reference itself admits. triangle.rs:146 accepts a hit only if |a| >= min_dist (a = e1 . (d x e2): about
    twice the triangle's area times |d| times a cosine) and min_dist < t < 1 / min_dist, and triangle.rs:398 starts the scan
    at t = 1e6; so for triangle size L, direction length D and hit distance rho a row has L^2 D >~ min_dist and
    min_dist D < rho < min(D / min_dist, 1e6 D). Outside of that the scan finds nothing and there is nothing to compare.
    Mesh sizes from 3e-7 to 3e6, min_dist from 1e-17 to 1e-2, direction lengths from 1e-4 to 1e4. max_dist is 1e5 bounding
    radii (no ray of rays() starts further than 1e4 radii from its target: it plays no part) except in the row named for it,
    where it is the bounding radius itself: the origins one radius from their targets have their hits right at the cut."""
    unit = (0.2, 1.0, 3.0)
    rows = {}

    def add(name, md, min_dist, lengths=unit, env=None, max_dist=None):
        rows[name] = (md, env or {}, min_dist, max_dist if max_dist is not None else 1e5 * radius(md), lengths)

    add("s15_e1e-3", rough_mesh(oracle, 15.0), 1e-3)
    add("s15_e1e-6", rough_mesh(oracle, 15.0), 1e-6)
    add("s15_e1e-3_short_long", rough_mesh(oracle, 15.0), 1e-3, (1e-4, 1e4))
    add("s15_e1e-3_long", rough_mesh(oracle, 15.0), 1e-3, (30.0, 1000.0))
    add("s15_e1e-3_maxdist", rough_mesh(oracle, 15.0), 1e-3, max_dist=radius(rough_mesh(oracle, 15.0)))
    add("s0.6_e1e-5", rough_mesh(oracle, 0.6), 1e-5)   # (0.6: no power of two times another row's scale)
    add("s1.5e-3_e1e-11", rough_mesh(oracle, 1.5e-3), 1e-11)
    add("s1.5e-3_e1e-7_short_long", rough_mesh(oracle, 1.5e-3), 1e-7, (1e-4, 1e4))
    add("s1.5e-6_e1e-17", rough_mesh(oracle, 1.5e-6), 1e-17)
    add("s1.5e4_e1e-6", rough_mesh(oracle, 1.5e4), 1e-6)
    add("s1.5e7_e1e-9", rough_mesh(oracle, 1.5e7), 1e-9)
    add("s1.5e7_e1e-9_short_long", rough_mesh(oracle, 1.5e7), 1e-9, (1e-3, 1e3))
    add("far+1e+03_small", oracle.mesh_prep(standin.triangles(1500, "rough"), 0.043, (0.0, 0.0, 0.0), (1e3, -40.0, 2.0),
                                            abi.material(abi.MAT_LAMBERTIAN, (0.6, 0.5, 0.4))), 1e-9)
    add("slivers_e1e-6", slivers(oracle, 1e-6), 1e-6)
    add("slivers_e1e-2", slivers(oracle, 1e-2), 1e-2)
    add("grid_e2^-20", integer_grid(oracle), 2.0 ** -20)
    return rows


SWEEP = ["s15_e1e-3", "s15_e1e-6", "s15_e1e-3_short_long", "s15_e1e-3_long", "s15_e1e-3_maxdist", "s0.6_e1e-5", "s1.5e-3_e1e-11",
         "s1.5e-3_e1e-7_short_long", "s1.5e-6_e1e-17", "s1.5e4_e1e-6", "s1.5e7_e1e-9", "s1.5e7_e1e-9_short_long", "far+1e+03_small",
         "slivers_e1e-6", "slivers_e1e-2", "grid_e2^-20"]


def targets(md, N, T, rng, n):
    """n points where culling is tight: node box corners / edge and face points of the tree, triangle vertices and edge points."""
    child = N[:, 24:28].view(np.int32)
    lo = np.stack([N[:, 0:4], N[:, 4:8], N[:, 8:12]], -1)[child != NO_CHILD]      # (boxes, 3)
    hi = np.stack([N[:, 12:16], N[:, 16:20], N[:, 20:24]], -1)[child != NO_CHILD]
    b = rng.integers(0, len(lo), n)
    sel = rng.integers(0, 3, (n, 3))                   # per axis: the low face, the high face, or a point in between
    f = np.where(sel == 0, 0.0, np.where(sel == 1, 1.0, rng.random((n, 3))))
    box_pts = lo[b] + f * (hi[b] - lo[b])
    real = T[:, 9].view(np.uint32) != 0xFFFFFFFF
    R = T[real]
    t = rng.integers(0, len(R), n)
    w = rng.integers(0, 4, n)
    s = rng.random(n)
    u = np.where(w == 0, 0.0, np.where(w == 1, s, np.where(w == 2, 0.0, 1.0 - s)))[:, None]
    v = np.where(w == 0, 0.0, np.where(w == 1, 0.0, np.where(w == 2, s, s)))[:, None]
    tri_pts = R[t, 0:3] + u * R[t, 3:6] + v * R[t, 6:9]    # vertex v0, edges v0-v1, v0-v2, v1-v2
    return np.where(rng.random((n, 1)) < 0.5, box_pts, tri_pts).astype(np.float64)


def rays(md, N, T, n, seed=0, eps=EPS, lengths=(0.2, 1.0, 3.0)):
    """n rays (float32 (n, 6)) aimed at targets(): origin distances 1.5 eps, R, 60 R, 1e4 R; a third of them grazing;
    direction lengths drawn from `lengths`."""
    rng = np.random.default_rng(seed)
    p = targets(md, N, T, rng, n)
    R = float(np.linalg.norm((md.bbox_hi - md.bbox_lo).astype(np.float64)) / 2)
    d = rng.normal(size=(n, 3))
    graze = rng.random(n) < 1 / 3
    axis = rng.integers(0, 3, n)
    d[graze, axis[graze]] *= 1e-6                      # nearly parallel to a box face
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    dist = rng.choice([1.5 * eps, R, 60 * R, 1e4 * R], n)
    o = p - d * dist[:, None]
    d = d * rng.choice(list(lengths), n)[:, None]
    return np.concatenate([o, d], 1).astype(np.float32)
