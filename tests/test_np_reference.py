"""The C++ oracle against an independent numpy-float32 restatement written from the Rust text (tests/np_reference.py).

The reference's own unit tests pin only vec3 ops, the packet dot/cross, the triangle normal, two sphere hits,
reflect, refract and the AABB extents (tests/test_oracle_kats.py). Everything else on the hot path -- the bbox gate
(T1), the packet Moller-Trumbore kernel and its arg-min (T4, T5), the mesh hit record (T6), the camera ray (C1),
Scene::hit (S0), the sphere quirks (S1), the three scatter functions (M1-M5), the integrator and the per-pixel mean
(I1, I2), the quantisation (I3) -- is pinned HERE: two restatements that share no code (C++ with AVX intrinsics and a
recursive integrator there, numpy arrays over all triangles here) must agree bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import gate_boxes
import np_reference as R
import scenes
from rbrt_amd import abi

f32 = np.float32
GOLD = __import__("pathlib").Path(__file__).resolve().parent / "golden"


def np_mat(m):
    return (int(m.kind), np.array(list(m.albedo), f32), f32(m.param))


def np_mesh(md):
    d = {k: md.arrays[k] for k in md.arrays}
    d.update(is_padding=md.is_padding, bbox_lo=np.float32(md.bbox_lo), bbox_hi=np.float32(md.bbox_hi), mat=np_mat(md.struct.mat))
    return d


def np_scene(sc):
    return dict(spheres=[(np.array(c, f32), f32(r), np_mat(m)) for c, r, m in sc.spheres], meshes=[np_mesh(m) for m in sc.meshes])


def np_cam(cam):
    return dict(position=np.array(list(cam.position), f32), right=np.array(list(cam.right), f32),
                up=np.array(list(cam.up), f32), img_center_point=np.array(list(cam.img_center_point), f32),
                mm_per_pix_hor=f32(cam.mm_per_pix_hor), mm_per_pix_vert=f32(cam.mm_per_pix_vert),
                W=int(cam.img_width_pix), H=int(cam.img_height_pix))


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def test_scene_hit_on_the_committed_ray_records(oracle):
    """S0 + S1 + T1 + T4 + T5 + T6: the 600 committed single-ray records (example scene + 3001-triangle stand-in;
    N % 8 = 1: the truncated-tail quirk is in play) through the numpy Scene::hit."""
    g = np.load(GOLD / "rays_example3001.npz")
    sc = np_scene(scenes.example_scene(oracle, 3001))
    n_mesh = 0
    for k, ray in enumerate(g["rays"]):
        h = R.scene_hit(sc, ray[:3].copy(), ray[3:].copy(), f32(0.001), f32(2000.0))
        if h is None:
            assert g["obj"][k] == -1, k
            continue
        assert h["obj"] == g["obj"][k] and h["tri"] == g["tri"][k], k
        assert bits(h["t"]) == bits(g["t"][k]) and bits(h["dist"]) == bits(g["dist"][k]), k
        n_mesh += h["obj"] >= 4
    assert n_mesh > 100


def test_packet_kernel_per_triangle_results(oracle):
    """T4 lane by lane: the per-triangle t (or -1000) array of triangle.rs:257-258, and T5's arg-min."""
    rng = np.random.default_rng(3)
    md = oracle.mesh_prep(scenes.random_soup(rng, 779, extent=2.0, size=0.8))  # N % 8 = 3
    mesh = np_mesh(md)
    n = (md.n_total // 8) * 8
    hits = 0
    for _ in range(150):
        o = rng.uniform(-4, 4, 3).astype(f32)
        d = (rng.uniform(-1, 1, 3) * rng.uniform(0.2, 3)).astype(f32)
        ray = np.concatenate([o, d]).astype(f32)
        params = np.zeros(n, f32)
        t, idx = C.c_float(), C.c_int32()
        ok = oracle.lib().rbrt_oracle_kat_mesh_intersect(C.byref(md.struct), oracle._p(ray), 0.001, C.byref(t), C.byref(idx),
                                                         oracle._p(params))
        res, np_params = R.triangle_scan(mesh, o, d, 0.001)
        assert np.array_equal(bits(params), bits(np_params))
        assert bool(ok) == (res is not None)
        if res is not None:
            assert bits(res[0]) == bits(t.value) and res[1] == idx.value
            hits += 1
    assert hits > 30


def test_bbox_gate(oracle):
    """T1 incl. zero, negative-zero, inf and NaN direction components (f32::min/max ignore NaN)."""
    rng = np.random.default_rng(5)
    lo, hi = np.array([-1, -2, -3], f32), np.array([2, 1, 0.5], f32)
    rays = [np.concatenate([rng.uniform(-6, 6, 3), rng.uniform(-1, 1, 3)]).astype(f32) for _ in range(3000)]
    specials = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-38, 1.0, -1.0]
    for a in specials:
        for b in specials:
            for o in ([0, 0, 0], [5, 0, 0], [0, -5, 0.2], [-1, 1, 0.5], [2, 1, 0.5]):
                rays.append(np.array([*o, a, b, 1.0], f32))
                rays.append(np.array([*o, 0.3, a, b], f32))
    n_true = 0
    for ray in rays:
        got = R.bbox_hit(lo, hi, ray[:3], ray[3:])
        exp = bool(oracle.lib().rbrt_oracle_kat_bbox_hit(oracle._p(lo), oracle._p(hi), oracle._p(ray)))
        assert got == exp, ray
        n_true += got
    assert 200 < n_true < len(rays) - 200


def test_camera_rays(oracle):
    """C1: integer halving, draw order (column jitter first), raw `up`."""
    for (w, h) in ((400, 300), (1024, 768), (33, 17)):
        cam = scenes.camera(oracle, w, h)
        nc = np_cam(cam)
        rng = np.random.default_rng(w)
        for _ in range(60):
            row, col, s, seed = int(rng.integers(h)), int(rng.integers(w)), int(rng.integers(4096)), int(rng.integers(1 << 40))
            out = np.zeros(6, f32)
            oracle.lib().rbrt_oracle_kat_camera_ray(C.byref(cam), row, col, seed, s, oracle._p(out))
            o, d = R.camera_ray(nc, row, col, R.Rng(seed, row * w + col, s))
            assert np.array_equal(bits(out[:3]), bits(o)) and np.array_equal(bits(out[3:]), bits(d))


def test_sphere_quirks(oracle):
    """S1: quirk A (near root slightly positive but below min_dist: None WITHOUT trying the far root), quirk B
    (tangent with negative t is not rejected by the sign test), unnormalised normal; random rays besides."""
    rng = np.random.default_rng(9)
    cases = []
    for _ in range(400):
        c = rng.uniform(-3, 3, 3).astype(f32)
        r = f32(rng.uniform(0.2, 2.5))
        o = rng.uniform(-5, 5, 3).astype(f32)
        d = (rng.uniform(-1, 1, 3) * rng.uniform(0.2, 2)).astype(f32)
        if rng.random() < 0.6:  # aimed at (or just past the rim of) the sphere, from outside or inside
            d = ((c + rng.uniform(-1.1, 1.1, 3) * r - o) * rng.uniform(0.05, 1.5)).astype(f32)
        cases.append((c, r, o, d))
    c, r = np.array([0, 0, -10], f32), f32(1.0)
    for tiny in (1e-4, 5e-4, 9e-4, 1.1e-3, 2e-3):  # ray leaving the surface from just inside: near root in (0, min_dist)
        cases.append((c, r, np.array([0, 0, -9 - tiny], f32), np.array([0, 0, 1], f32)))
        cases.append((c, r, np.array([0, 0, -9 + tiny], f32), np.array([0, 0, -1], f32)))
    cases.append((c, r, np.array([1, 0, 0], f32), np.array([0, 0, 1], f32)))   # tangent line, sphere behind: sol == 0, t < 0
    cases.append((c, r, np.array([1, 0, 0], f32), np.array([0, 0, -1], f32)))  # tangent line, sphere ahead
    cases.append((np.array([0, -1000, -5], f32), f32(1000.0), np.array([0, 5, 4], f32), np.array([0.1, -0.5, -0.8], f32)))
    n_hit = 0
    for c, r, o, d in cases:
        sph = abi.Sphere((C.c_float * 3)(*c), float(r), abi.material(0))
        pt, nm, dist = np.zeros(3, f32), np.zeros(3, f32), C.c_float()
        ray = np.concatenate([o, d]).astype(f32)
        ok = oracle.lib().rbrt_oracle_kat_sphere(C.byref(sph), oracle._p(ray), 0.001, 2000.0, oracle._p(pt), oracle._p(nm), C.byref(dist))
        h = R.sphere_hit(c, r, o, d, f32(0.001), f32(2000.0))
        assert bool(ok) == (h is not None), (c, r, o, d)
        if h is not None:
            assert np.array_equal(bits(h[0]), bits(pt)) and np.array_equal(bits(h[1]), bits(nm)) and bits(h[2]) == bits(dist.value)
            n_hit += 1
    assert n_hit > 150


@pytest.mark.parametrize("kind,param", [(0, 0.0), (1, 0.005), (1, 0.6), (2, 1.8), (2, 0.2)])
def test_scatter_events(oracle, kind, param):
    """M1-M5: a few hundred scatter events per material with an explicit random stream: same bool, attenuation,
    new ray, bit for bit (incl. the draw order and count: a wrong count would desynchronise the next event)."""
    rng = np.random.default_rng(kind * 10 + int(param * 100))
    mat = abi.material(kind, (0.7, 0.3, 0.2), param)
    n_false = 0
    for k in range(300):
        d = (rng.uniform(-1, 1, 3) * rng.uniform(0.3, 2)).astype(f32)
        n = (rng.uniform(-1, 1, 3) * rng.uniform(0.3, 1000)).astype(f32)  # sphere normals are unnormalised
        p = rng.uniform(-10, 10, 3).astype(f32)
        o = rng.uniform(-10, 10, 3).astype(f32)
        seed, pixel, sample = int(rng.integers(1 << 40)), int(rng.integers(1 << 20)), int(rng.integers(4096))
        att, out = np.zeros(3, f32), np.zeros(6, f32)
        ray = np.concatenate([o, d]).astype(f32)
        ok = oracle.lib().rbrt_oracle_kat_scatter(C.byref(mat), oracle._p(ray), oracle._p(p), oracle._p(n), seed, pixel, sample,
                                                  oracle._p(att), oracle._p(out))
        r = R.Rng(seed, pixel, sample)
        got_ok, got_att, no, nd = R.scatter(np_mat(mat), d, dict(point=p, normal=n), r)
        assert bool(ok) == got_ok, k
        assert np.array_equal(bits(att), bits(got_att)), k
        assert np.array_equal(bits(out[:3]), bits(no)) and np.array_equal(bits(out[3:]), bits(nd)), k
        n_false += not got_ok
    if kind == 1:
        assert n_false > 20  # metal.rs:25 really returns false sometimes


@pytest.mark.parametrize("which", ["example2003", "header2004"])
def test_whole_pixels_end_to_end(oracle, which):
    """I1 + I2 (+ everything below them): whole pixels -- camera ray, recursion to depth 50 with the right-to-left
    attenuation product, per-pixel sequential sum, * (1/spp) -- through numpy vs the oracle's render, bit for bit,
    on windows that cover the mesh, the glass and metal spheres and the ground; ray counts equal too."""
    if which == "example2003":
        sc = scenes.example_scene(oracle, 2003)
        windows = [(96, 104, 40, 46), (40, 46, 60, 64), (70, 76, 62, 66)]  # mesh / metal sphere / glass sphere + ground
    else:
        sc = scenes.header_scene(oracle, 2004)
        windows = [(88, 94, 44, 50), (60, 66, 70, 74)]
    W, H, spp, seed = 160, 120, 3, 11
    cam = scenes.camera(oracle, W, H)
    nc, ns = np_cam(cam), np_scene(sc)
    for (c0, c1, r0, r1) in windows:
        exp, _, rays = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=seed), window=(c0, c1, r0, r1), want_rgb8=True)
        counter = [0]
        for row in range(r0, r1):
            for col in range(c0, c1):
                got = R.pixel(nc, ns, row, col, spp, seed, counter=counter)
                assert np.array_equal(bits(got), bits(exp[row, col])), (which, row, col, got, exp[row, col])
        assert counter[0] == rays


def test_quantise(oracle):
    vals = np.concatenate([np.random.default_rng(1).uniform(0, 1.2, 500), [0.0, 1.0, 0.99609375, 0.9921875, 4.0, -1.0, np.nan, np.inf]]).astype(f32)
    for c in vals:
        assert oracle.lib().rbrt_oracle_kat_quantise(float(c)) == R.quantise(c), c


@pytest.mark.parametrize("box", list(gate_boxes.GATE_BOXES))
def test_gate_inputs_split_each_box(oracle, box):
    """A condition on the inputs of test_gpu_parity.test_division_free_mesh_gate_decides_like_the_ieee_form, with the numpy
    form alone: the rays of every box are neither all accepted nor all rejected (the inverted box of a mesh without
    triangles accepts every ray but those from an infinite origin), and the two boxes made for the gate's cut-offs have
    their quotients on both sides of them."""
    lo, hi, scales = gate_boxes.gate_box(oracle, box)
    rays, _, _ = gate_boxes.gate_rays(box, lo, hi, scales)
    rate = R.bbox_gate(lo, hi, rays).mean()
    print(f"{box}: lo {lo} hi {hi}, {len(rays)} rays, accept rate {rate:.4f}")
    assert 0.0 < rate < 1.0
    if box == "config2":
        assert 0.2 < rate < 0.9  # (what the one-box test asked of it)
    with np.errstate(all="ignore"):
        q = np.abs(np.concatenate([(lo - rays[:400_000, :3]) / rays[:400_000, 3:], (hi - rays[:400_000, :3]) / rays[:400_000, 3:]], 1)).max(1)
    if box == "quotients_near_1e30":   # the largest quotient of a ray, within two decades of the cut-off on both sides
        assert ((q > 1e28) & (q < 1e30)).mean() > 0.1 and ((q > 1e30) & (q < 1e32)).mean() > 0.1
    if box == "quotients_near_1e-30":
        assert ((q > 1e-32) & (q < 1e-30)).mean() > 0.1 and ((q > 1e-30) & (q < 1e-28)).mean() > 0.1
