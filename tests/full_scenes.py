"""Scenes that use every extension at once (emitters, the constant background, the thin lens, smooth and flat meshes,
BasicTriangles in element order, distance windows), for the oracle-against-restatement tests on CPU and the HIP-against-
oracle tests on the GPU: a fuzzer, scenes at the object limit, and one fixed scene with everything.

Corner normals are drawn where kernels go wrong: all-zero corners (the fallback to the face normal), anti-face and non-unit
normals, and magnitudes that put |m|^2 on both sides of normalize's short-path gate (2^-80 and 2^52), at and around
2^-100 (m.m underflows) and up to 2^64 (m.m overflows: three divisions by an infinite length give a finite zero vector,
which the contract keeps)."""
from __future__ import annotations

import numpy as np

import np_lens
import np_smooth
import scenes
from rbrt_amd import abi

f32 = np.float32
L_, M_, D_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
T = scenes.T
# exponents e of a corner normal scaled by 2^e: |m|^2 ~ 2^(2e) straddles 2^-80 (e = -40) and 2^52 (e = 26); -100 and
# below underflow m.m, 64 overflows it
GATE_EXPONENTS = (-110, -100, -99, -64, -41, -40, -39, -20, 0, 25, 26, 27, 40, 60, 63, 64)


def mat(rng, kinds=(L_, M_, D_, EM)):
    """A material of a random kind among `kinds`; an emitter's L from 0 to large."""
    k = int(kinds[int(rng.integers(len(kinds)))])
    if k == EM:
        scale = float(rng.choice([0.0, 1.0, 8.0, 200.0]))
        return abi.material(EM, tuple(float(x) for x in rng.uniform(0.0, 1.0, 3) * scale))
    if k == M_:
        return abi.material(M_, tuple(rng.uniform(0.05, 0.95, 3)), float(rng.uniform(0.0, 0.6)))
    if k == D_:
        return abi.material(D_, (0.0, 0.0, 0.0), float(rng.uniform(0.3, 2.2)))
    return abi.material(L_, tuple(rng.uniform(0.05, 0.95, 3)))


def decorate(cn, rng, p=0.35):
    """Corner normals cn (N, 3, 3) with a fraction p of the entries changed: all-zero corners, the anti-face direction,
    non-unit lengths, one corner zero, and all three corners scaled by 2^e for e in GATE_EXPONENTS."""
    cn = np.array(cn, np.float64)
    for i in np.nonzero(rng.random(len(cn)) < p)[0]:
        what = int(rng.integers(5))
        if what == 0:
            cn[i] = 0.0
        elif what == 1:
            cn[i] = -cn[i]
        elif what == 2:
            cn[i] *= rng.uniform(0.01, 50.0, (3, 1))
        elif what == 3:
            cn[i, int(rng.integers(3))] = 0.0
        else:
            cn[i] *= 2.0 ** float(rng.choice(GATE_EXPONENTS))
    with np.errstate(over="ignore"):
        return cn.astype(f32)


def face_corner_normals(md, rng, noise=0.3):
    """Corner normals for an arbitrary mesh: its face normals, perturbed per corner (N real entries)."""
    n = md.n_real
    face = np.stack([md.arrays["nx"][:n], md.arrays["ny"][:n], md.arrays["nz"][:n]], 1).astype(np.float64)
    return face[:, None, :] + rng.normal(size=(n, 3, 3)) * noise


def smooth_standin(oracle, rng, n, scale, translation, m, style):
    """The stand-in (rotation 0) with 'computed' (the host's area-weighted) or 'file' normals, decorated."""
    md = np_smooth.standin_smooth(oracle, n, scale, translation, m, style)
    cn = np.stack([np.stack([md.normals[f"n{k}{c}"][:md.n_real] for c in "xyz"], 1) for k in range(3)], 1)
    return np_smooth.with_normals(md, decorate(cn, rng))


def lens_of(cam, look_at, focal_mm, r, focus_scale):
    """The host's lens (np_lens.lens_for) of radius r scene units, focused at focus_scale times the image plane."""
    return np_lens.lens_for(cam, look_at, focal_mm, 2000.0 * r, focus_scale * focal_mm / 1000.0)


def fuzz_case(oracle, seed, tiny=False):
    """One random scene with every feature: dict(cam, lens, sc, opts, builder, what)."""
    rng = np.random.default_rng(70000 + seed)
    spheres = [((0.0, -1000.0, -5.0), 1000.0, mat(rng))] if rng.random() < 0.7 else []
    for _ in range(int(rng.integers(0, 4 if tiny else 9))):
        spheres.append((tuple(rng.uniform(-6, 6, 3) + np.array([0, 2, -10])), float(rng.uniform(0.3, 2.5)), mat(rng)))
    meshes = []
    for _ in range(int(rng.integers(0, 3 if tiny else 4))):
        n = int(rng.integers(1, 60 if tiny else 700))
        style = int(rng.integers(4))  # 0 flat soup, 1 smooth soup, 2 stand-in computed normals, 3 stand-in file normals
        if style < 2:
            tri = scenes.random_soup(rng, n, extent=float(rng.uniform(0.5, 3.0)), size=float(rng.uniform(0.05, 1.0)))
            md = oracle.mesh_prep(tri, float(rng.uniform(0.5, 2.0)), tuple(rng.uniform(-1, 1, 3)),
                                  tuple(rng.uniform(-3, 3, 3) + np.array([0, 1.5, -9])), mat(rng))
            if style == 1:
                md = np_smooth.with_normals(md, decorate(face_corner_normals(md, rng), rng))
        else:
            md = smooth_standin(oracle, rng, n + 20, float(rng.uniform(15, 60)), tuple(rng.uniform(-4, 4, 3) + np.array([0, 0, -10])),
                                mat(rng), "computed" if style == 2 else "file")
        meshes.append(md)
    tris, order = [], None
    for _ in range(int(rng.integers(0, 7))):
        c = rng.uniform(-5, 5, 3) + np.array([0, 2, -9])
        tris.append((tuple(map(tuple, c + rng.uniform(-3, 3, (3, 3)))), mat(rng)))
    if tris:
        order = [i for i in range(len(spheres))] + [T | i for i in range(len(tris))]
        rng.shuffle(order)
    sc = abi.SceneData(spheres=spheres, meshes=meshes, triangles=tris, element_order=order)
    w, h = (int(rng.integers(6, 13)), int(rng.integers(5, 10))) if tiny else (int(rng.integers(20, 90)), int(rng.integers(16, 70)))
    pos = rng.uniform(-2, 2, 3) + np.array([0, 4, 4])
    look = (rng.uniform(-4, 4, 3) + np.array([0, 1.5, -10])) - pos
    look = tuple(look / np.linalg.norm(look))
    up = tuple(np.array([0.0, 1.0, 0.0]) + rng.uniform(-0.5, 0.5, 3))
    focal = float(np.exp(rng.uniform(np.log(12.0), np.log(120.0))))
    cam = scenes.camera(oracle, w, h, position=tuple(pos), look_at=look, up=up, focal_mm=focal)
    lens = None
    if rng.random() < 0.6:  # apertures from 0 to past the focus distance (where the tile pass can cull nothing)
        fs = float(np.exp(rng.uniform(np.log(0.05), np.log(2000.0))))
        D = fs * focal / 1000.0
        r = 0.0 if rng.random() < 0.1 else float(np.exp(rng.uniform(np.log(1e-4), np.log(3.0 * D))))
        lens = lens_of(cam, look, focal, r, fs)
    kw = {}
    if rng.random() < 0.5:
        kw["flags"] = abi.FLAG_CONSTANT_BACKGROUND
        kw["bg"] = tuple(float(x) for x in rng.choice([0.0, 0.3, 2.5]) * rng.uniform(0.0, 1.0, 3)) if rng.random() < 0.7 else (0.0, 0.0, 0.0)
    elif rng.random() < 0.5:
        kw["bg"] = tuple(float(x) for x in rng.uniform(0.0, 3.0, 3))
    if rng.random() < 0.3:
        kw["min_dist"] = float(np.exp(rng.uniform(np.log(0.001), np.log(2.0))))
        kw["max_dist"] = float(rng.uniform(5.0, 30.0))
    depth = int(rng.choice([0, 1, 3] if tiny else [0, 1, 3, 50]))
    spp = int(rng.integers(1, 3 if tiny else 6))
    opts = abi.default_opts(spp=spp, seed=seed, max_depth=depth, **kw)
    what = (f"fuzz {seed}: {len(spheres)} spheres, {len(tris)} triangles, meshes {[(m.n_real, m.normals is not None) for m in meshes]}, "
            f"{w}x{h}x{spp}, depth {depth}, lens {lens is not None}, flags {opts.flags}")
    return dict(cam=cam, lens=lens, sc=sc, opts=opts, builder="device" if seed % 2 else None, what=what)


# ---- the object limit -------------------------------------------------------------------------------------------------------
N_MAX = 255  # kMaxObjects: spheres + BasicTriangles + meshes


def sphere_grid(rng, n, with_ground=True):
    """n spheres: the ground and a grid of small ones on it in front of the example camera, every eighth an emitter."""
    out = [((0.0, -1000.0, -5.0), 1000.0, abi.material(L_, (0.5, 0.5, 0.5)))] if with_ground else []
    k = 0
    while len(out) < n:
        i, j = k % 17, k // 17
        r = 0.28
        c = (-8.0 + i * 1.0 + 0.3 * (j % 2), r + 0.02 * (k % 3), -4.5 - j * 1.1)
        m = abi.material(EM, (2.0, 1.5, 1.0)) if k % 8 == 5 else mat(rng, (L_, M_, D_))
        out.append((c, r, m))
        k += 1
    return out


def limit_scene(oracle, mix):
    """Exactly N_MAX objects. 'spheres': 255 spheres, the last an emitter. 'smooth_last': 254 spheres and a smooth mesh
    (id 254). 'mixed': 200 BasicTriangles, 40 spheres and 15 meshes, some smooth, the last (id 254) an emissive mesh, an
    emitter among the last elements."""
    rng = np.random.default_rng({"spheres": 1, "smooth_last": 2, "mixed": 3}[mix])
    if mix == "spheres":
        sph = sphere_grid(rng, N_MAX)
        sph[-1] = (sph[-1][0], sph[-1][1], abi.material(EM, (6.0, 5.0, 4.0)))
        return abi.SceneData(spheres=sph)
    if mix == "smooth_last":
        sph = sphere_grid(rng, N_MAX - 1)
        md = smooth_standin(oracle, rng, 300, 30.0, (1.0, -0.5, -9.0), abi.material(M_, (0.9, 0.8, 0.7), 0.05), "computed")
        return abi.SceneData(spheres=sph, meshes=[md])
    sph = sphere_grid(rng, 40)
    tris = []
    for k in range(200):
        c = np.array([rng.uniform(-9, 9), rng.uniform(0.1, 4.0), rng.uniform(-22, -5)])
        m = abi.material(EM, (3.0, 3.0, 3.0)) if k in (197, 198) else mat(rng, (L_, M_, D_))
        tris.append((tuple(map(tuple, c + rng.uniform(-0.6, 0.6, (3, 3)))), m))
    order = [i for i in range(len(sph))] + [T | i for i in range(len(tris))]
    rng.shuffle(order)
    order = [e for e in order if e != (T | 198)] + [T | 198]  # an emitter is the last element (id 239)
    meshes = []
    for k in range(15):
        tr = (-7.0 + k, 0.6 + 0.3 * (k % 3), -8.0 - 1.5 * (k % 5))
        if k == 14:
            m = abi.material(EM, (4.0, 2.0, 1.0))
        else:
            m = mat(rng, (L_, M_, D_))
        if k % 3 == 1 or k == 14:
            meshes.append(smooth_standin(oracle, rng, 40 + 7 * k, 6.0, tr, m, "computed" if k % 2 else "file"))
        else:
            meshes.append(scenes.standin_mesh(oracle, 40 + 7 * k, 6.0, tr, (0.0, 0.3 * k, 0.0), m))
    return abi.SceneData(spheres=sph, meshes=meshes, triangles=tris, element_order=order)


# ---- one scene with everything -----------------------------------------------------------------------------------------------
def all_features_scene(oracle):
    """The example spheres and an emissive one; BasicTriangles (one emissive) interleaved with them; a smooth tessellated
    sphere, a smooth stand-in with decorated area-weighted normals, a smooth emissive stand-in and a flat stand-in of 1203
    entries (enough for the device builder)."""
    rng = np.random.default_rng(5)
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(EM, (3.0, 2.5, 1.5)))]
    tris = list(scenes.TRIANGLES) + [(((-4.0, 0.3, -6.0), (-1.5, 0.4, -6.5), (-2.7, 2.6, -7.0)), abi.material(EM, (1.5, 3.0, 2.5)))]
    order = [0, T | 0, 1, T | 4, T | 2, 2, T | 1, 4, 3, T | 3]
    _, ball = np_smooth.sphere_mesh(oracle, (3.2, 1.2, -8.0), 1.2, 3, abi.material(D_, (0.0, 0.0, 0.0), 1.5))
    blob = smooth_standin(oracle, rng, 301, 30.0, (-1.0, -1.3, -6.5), abi.material(M_, (0.8, 0.8, 0.75), 0.05), "computed")
    lamp = smooth_standin(oracle, rng, 61, 20.0, (5.0, -0.8, -11.0), abi.material(EM, (2.0, 2.0, 4.0)), "file")
    flat = scenes.standin_mesh(oracle, 1203, 35.0, (0.0, -1.0, -14.0), (0.0, 0.0, 0.0), abi.material(L_, (0.3, 0.6, 0.3)))
    return abi.SceneData(spheres=sph, meshes=[ball, blob, lamp, flat], triangles=tris, element_order=order)


def all_features_camera(oracle, w, h):
    """The example camera and a lens of 20 mm focused at 9 units."""
    cam = scenes.camera(oracle, w, h)
    return cam, np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 20.0, 9.0)


def all_features_opts(spp, seed, **kw):
    """A constant black background, and a distance window that leaves the whole scene in view."""
    return abi.default_opts(spp=spp, seed=seed, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0), min_dist=0.002,
                            max_dist=60.0, **kw)


# ---- rays at the meshes ------------------------------------------------------------------------------------------------------
def mesh_rays(sc, rng, per_mesh=400):
    """Rays from outside at random points of every mesh's real entries (corners and edges included), some grazing."""
    rays = []
    for md in sc.meshes:
        a = md.arrays
        for j in range(per_mesh):
            i = int(rng.integers(0, md.n_real))
            v0 = np.array([a["v0x"][i], a["v0y"][i], a["v0z"][i]], np.float64)
            e1 = np.array([a["e1x"][i], a["e1y"][i], a["e1z"][i]], np.float64)
            e2 = np.array([a["e2x"][i], a["e2y"][i], a["e2z"][i]], np.float64)
            b = rng.dirichlet((1.0, 1.0, 1.0)) if j % 5 else np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0]][j % 4], float)
            p = v0 + b[1] * e1 + b[2] * e2
            nf = np.cross(e1, e2)
            nf /= np.linalg.norm(nf) + 1e-30
            side = 1.0 if rng.random() < 0.8 else -1.0
            dirn = side * nf + 0.8 * rng.normal(size=3)
            dirn /= np.linalg.norm(dirn) + 1e-30
            o = p + rng.uniform(0.5, 6.0) * dirn
            rays.append(np.concatenate([o, -dirn]))
    return np.array(rays, f32).reshape(-1, 6)


def same_bits(a, b):
    """Bit for bit, a NaN anywhere in one only where the other has one too."""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(np.where(nan, 0, a).view(np.uint32),
                                                                         np.where(nan, 0, b).view(np.uint32)))

