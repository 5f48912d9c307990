"""Smooth shading of meshes (rbrt_hip.h rbrt_scene_shading_t) restated in numpy float32, on top of np_reference.py.

The contract (include/rbrt_hip.h): when the closest hit of a ray (o, d) is entry i of a mesh with
corner normals n0, n1, n2, scatter uses, in float32, unfused, in this order,
    h = d x e2;  a = e1 . h;  f = 1 / a;  s = o - v0;  u = f (s . h);  q = s x e1;  v = f (d . q)
    w = (1 - u) - v;  m_c = ((w n0_c) + (u n1_c)) + (v n2_c);  n_s = normalize(m)
and the stored face normal when n_s is not finite (m of length 0 included). u and v are triangle_scan's.
Everything else is test_emissive's colorize (the reference's, plus emitters and the constant background).

Also here: the meshes the tests use (a tessellated sphere with its exact normals, the stand-in with computed or
file-style normals) and the host's area-weighted vertex normals (rbrt_amd/host/scene.cpp smooth_model_normals)."""
from __future__ import annotations

import numpy as np

import np_reference as R
import test_emissive as E
import test_np_reference as T
from rbrt_amd import abi, standin

f32 = np.float32
NF = abi.NORMAL_FIELDS


# ---- the shading normal ----------------------------------------------------------------------------------------------
def barycentrics(mesh, i, o, d):
    """(u, v) of entry i for the ray (o, d): triangle_scan's expressions for that one entry."""
    g = {k: mesh[k][i:i + 1] for k in ("v0x", "v0y", "v0z", "e1x", "e1y", "e1z", "e2x", "e2y", "e2z")}
    with np.errstate(all="ignore"):
        hx, hy, hz = R._cross_soa(d[0], d[1], d[2], g["e2x"], g["e2y"], g["e2z"])
        a = R._dot_soa(g["e1x"], g["e1y"], g["e1z"], hx, hy, hz)
        f = R.F1 / a
        sx, sy, sz = o[0] - g["v0x"], o[1] - g["v0y"], o[2] - g["v0z"]
        u = f * R._dot_soa(sx, sy, sz, hx, hy, hz)
        qx, qy, qz = R._cross_soa(sx, sy, sz, g["e1x"], g["e1y"], g["e1z"])
        v = f * R._dot_soa(d[0], d[1], d[2], qx, qy, qz)
    return f32(u[0]), f32(v[0])


def shading_normal(mesh, i, o, d):
    """The normal scatter uses at a hit of entry i of `mesh` (an np_reference mesh dict; 'normals' = its corner normals)."""
    face = R.vec(mesh["nx"][i], mesh["ny"][i], mesh["nz"][i])
    nrm = mesh.get("normals")
    if nrm is None:
        return face
    u, v = barycentrics(mesh, i, o, d)
    with np.errstate(all="ignore"):
        w = f32(f32(R.F1 - u) - v)
        m = np.array([f32(f32(f32(w * nrm[f"n0{c}"][i]) + f32(u * nrm[f"n1{c}"][i])) + f32(v * nrm[f"n2{c}"][i])) for c in "xyz"], f32)
        n = R.normalize(m)
    return n if np.all(np.isfinite(n)) else face


def scene_hit(scene, o, d, min_dist, max_dist):
    """np_reference.scene_hit with the shading normal of a smooth mesh's hit."""
    hit = R.scene_hit(scene, o, d, min_dist, max_dist)
    if hit is not None and hit["tri"] >= 0:
        hit["normal"] = shading_normal(scene["meshes"][hit["obj"] - n_elements(scene)], hit["tri"], o, d)
    return hit


def n_elements(scene):
    return len(scene["spheres"]) + len(scene.get("triangles", []))


def colorize(o, d, scene, bg, constant_bg, depth, rng, min_dist=f32(0.001), max_dist=f32(2000.0)):
    """test_emissive.colorize_emissive with the shading normal in place of a smooth mesh's face normal."""
    hit = scene_hit(scene, o, d, min_dist, max_dist)
    if hit is not None:
        kind, albedo, _ = hit["mat"]
        if kind == abi.MAT_EMISSIVE:
            return albedo.copy()
        if depth > 0:
            ok, att, no, nd = R.scatter(hit["mat"], d, hit, rng)
            if ok:
                return att * colorize(no, nd, scene, bg, constant_bg, depth - 1, rng, min_dist, max_dist)
        return R.vec(0, 0, 0)
    if constant_bg:
        return bg.copy()
    t = f32(0.5) * f32(d[1] + R.F1)
    return t * R.vec(1, 1, 1) + f32(R.F1 - t) * bg


def np_scene(sc):
    """test_emissive.np_scene with every smooth mesh's corner normals under 'normals'."""
    ns = E.np_scene(sc)
    for m, md in zip(ns["meshes"], sc.meshes):
        if md.normals is not None:
            m["normals"] = md.normals
    return ns


def restated_image(cam, sc, opts, pixels=None):
    """(radiance, rgb8) of the image by the restatement; `pixels`: only these (row, col), the rest stays 0."""
    nc, ns = T.np_cam(cam), np_scene(sc)
    bg = np.array(list(opts.bg), f32)
    const = bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND)
    H, W = cam.img_height_pix, cam.img_width_pix
    rad = np.zeros((H, W, 3), f32)
    for row, col in (pixels if pixels is not None else ((r, c) for r in range(H) for c in range(W))):
        color = R.vec(0, 0, 0)
        for s in range(opts.spp):
            rng = R.Rng(opts.seed, row * W + col, s)
            o, d = R.camera_ray(nc, row, col, rng)
            color = color + colorize(o, d, ns, bg, const, opts.max_depth, rng, f32(opts.min_dist), f32(opts.max_dist))
        rad[row, col] = color * f32(R.F1 / f32(opts.spp))
    return rad, np.vectorize(R.quantise, otypes=[np.uint8])(rad)


# ---- meshes ------------------------------------------------------------------------------------------------------------
def corner_arrays(cn, n_total):
    """(N, 3, 3) corner normals of the N real triangles -> the nine SoA arrays, padding entries copying entry 0's."""
    cn = np.asarray(cn, f32)
    full = np.concatenate([cn, np.repeat(cn[:1], n_total - len(cn), 0)]) if n_total > len(cn) else cn
    return {f"n{k}{c}": np.ascontiguousarray(full[:, k, j]) for k in range(3) for j, c in enumerate("xyz")}


def with_normals(md, cn):
    """MeshData md with the corner normals cn ((N, 3, 3) for its N real triangles)."""
    return md.with_normals(corner_arrays(cn, md.n_total))


def area_weighted(tris, faces):
    """The host's computed normals (scene.cpp smooth_model_normals) of one model: tris (N, 3, 3) float32 transformed
    triangles, faces (N, 3) their position indices. Per position index the float32 sum, in face order and corners 0, 1, 2,
    of cross(e1, e2); normalised; a sum that does not normalise to a finite vector gives the face normal, a non-finite face
    normal (0, 0, 0)."""
    tris = np.asarray(tris, f32)
    acc = {}
    crosses = []
    for t, fc in zip(tris, faces):
        c = R.cross(t[1] - t[0], t[2] - t[0])
        crosses.append(c)
        for k in range(3):
            acc[int(fc[k])] = acc.get(int(fc[k]), R.vec(0, 0, 0)) + c
    out = np.zeros((len(tris), 3, 3), f32)
    with np.errstate(all="ignore"):
        for i, (t, fc) in enumerate(zip(tris, faces)):
            face = R.normalize(crosses[i])
            for k in range(3):
                n = R.normalize(acc[int(fc[k])])
                out[i, k] = n if np.all(np.isfinite(n)) else (face if np.all(np.isfinite(face)) else 0.0)
    return out


def sphere_mesh(oracle, center, radius, n, mat):
    """A tessellated sphere (standin's cube-sphere, 12 n^2 triangles, outward) and its exact normals: (flat MeshData,
    smooth MeshData)."""
    dirs, faces = standin._cube_sphere(n)
    c = np.asarray(center, np.float64)
    tris = (c + radius * dirs[faces]).astype(f32)
    flat = oracle.mesh_prep(tris, 1.0, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), mat)
    return flat, with_normals(flat, dirs[faces].astype(f32))


def standin_smooth(oracle, n_triangles, scale, translation, mat, style):
    """The stand-in mesh (rotation 0) with corner normals: style 'computed' = area_weighted over its transformed triangles,
    'file' = unnormalised radial vectors from the model's centre, scaled (the kind of values a .obj's vn may hold)."""
    verts, faces = standin.make_mesh(n_triangles)
    md = oracle.mesh_prep(verts[faces], scale, (0.0, 0.0, 0.0), translation, mat)
    if style == "computed":
        # the transformed triangles, as mesh_prep made them: v0, v0 + e1 is not v1 in float, so take the positions again
        tv = (verts[faces] * f32(scale)).astype(f32) + np.asarray(translation, f32)
        cn = area_weighted(tv.astype(f32), faces)
    else:
        cn = (3.0 * (verts[faces] - standin._CENTER)).astype(f32)
    return with_normals(md, cn)
