"""Solid patterns on the GPU (pytest -m gpu), bit for bit on the float radiance: the test hook and whole images against
the numpy restatement (np_pattern.py), long records whose second entries pass through the gseq words, the limit of the
record byte, the anchors to the oracle (which does not know the pattern), every entry point, the feature buffers and the
CLI. References are computed once a module and shared."""
import ctypes as C
import functools
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_features
import np_lens
import np_pattern as NP
import np_smooth
import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
SHIPPED = ROOT / "scenes" / "checker" / "checker_ground.yaml"
f32 = np.float32
L, M, D, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
A1, A2 = (0.02, 0.2, 0.1), (0.8, 0.8, 0.7)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _from_oracle():
    from oracle import pyoracle
    pyoracle.lib()
    return pyoracle


# ---- scenes --------------------------------------------------------------------------------------------------------------
def sphere_scene(pattern="default", ground=A1):
    """A checkered ground sphere and a lambertian, a metal, a glass and an emissive sphere."""
    if pattern == "default":
        pattern = abi.checker(A2, 2.0, (0.0, -1.0, 0.0))
    spheres = [((0.0, -1000.0, -5.0), 1000.0, abi.material(L, ground)),
               ((-5.0, 1.5, -9.0), 1.5, abi.material(L, (0.1, 0.1, 0.9))),
               ((-2.5, 2.9, -15.0), 3.0, abi.material(M, (0.8, 0.8, 0.8), 0.005)),
               ((1.5, 1.25, -9.0), 1.5, abi.material(D, (0, 0, 0), 1.8)),
               ((4.0, 0.6, -8.0), 0.6, abi.material(EM, (0.5, 3.0, 3.0)))]
    return abi.SceneData(spheres=spheres, patterns=None if pattern is None else {0: pattern})


HOOK_ORIGIN, HOOK_SIZE = (0.11, -0.07, 0.23), 0.3
TRI_Z = -6.0


def hook_scene(oracle):
    """Every kind of object with a pattern -- a sphere, a BasicTriangle, a flat and a smooth mesh, and a sphere whose cells
    are so small that two of its coordinates clamp -- and a lambertian without one, a metal, a glass and an emitter."""
    ck = abi.checker(A2, HOOK_SIZE, HOOK_ORIGIN)
    spheres = [((-3.0, -1.0, -8.0), 1.5, abi.material(L, A1)),                 # 0 patterned
               ((3.5, 2.5, -9.0), 1.0, abi.material(L, (0.3, 0.4, 0.5), 7.0)),  # 1 plain lambertian (its param is ignored)
               ((3.5, -2.5, -9.0), 1.0, abi.material(M, (0.9, 0.8, 0.7), 0.3)),  # 2
               ((0.0, 3.5, -9.0), 1.0, abi.material(D, (0, 0, 0), 1.5)),         # 3
               ((0.0, -3.5, -9.0), 1.0, abi.material(EM, (4.0, 3.0, 2.0))),      # 4
               ((-3.5, 3.0, -9.0), 1.0, abi.material(L, (0.6, 0.1, 0.1)))]       # 5 patterned, clamping
    tri = [(((-1.5, -1.5, TRI_Z), (1.5, -1.5, TRI_Z), (0.0, 1.5, TRI_Z)), abi.material(L, (0.25, 0.5, 0.75)))]  # 6 patterned
    flat = scenes.standin_mesh(oracle, 203, 20.0, (5.0, -0.5, -12.0), (0.0, 0.0, 0.0), abi.material(L, (0.4, 0.4, 0.1)))  # 7
    smooth = np_smooth.standin_smooth(oracle, 203, 20.0, (-7.0, -0.5, -12.0), abi.material(L, (0.1, 0.4, 0.4)), "computed")  # 8
    pats = {0: ck, 5: abi.checker((0.0, 0.9, 0.0), 1e-7, (300.0, -250.0, -9.0)), 6: ck,
            7: abi.checker((0.9, 0.1, 0.9), HOOK_SIZE, HOOK_ORIGIN), 8: abi.checker((0.9, 0.9, 0.1), HOOK_SIZE, HOOK_ORIGIN)}
    return abi.SceneData(spheres=spheres, triangles=tri, meshes=[flat, smooth], patterns=pats)


def hook_rays(rng):
    """Rays from two origins at: points of the triangle's plane in, on and one ulp either side of cell faces in x and y
    (negative coordinates included); every object, at random."""
    faces_x = (f32(HOOK_ORIGIN[0]) + (np.arange(-5, 5) * f32(HOOK_SIZE)).astype(f32)).astype(f32)
    faces_y = (f32(HOOK_ORIGIN[1]) + (np.arange(-4, 4) * f32(HOOK_SIZE)).astype(f32)).astype(f32)
    targets = []
    for x in faces_x:
        for xx in (x, np.nextafter(x, f32(9)), np.nextafter(x, f32(-9))):
            for y in (-0.9, -0.3331, 0.2, faces_y[3]):
                targets.append((xx, y, TRI_Z))
    for y in faces_y:
        for yy in (y, np.nextafter(y, f32(9)), np.nextafter(y, f32(-9))):
            for x in (-0.4, 0.05, 0.31):
                targets.append((x, yy, TRI_Z))
    targets = np.array(targets, f32)
    centres = np.array([(-3.0, -1.0, -8.0), (3.5, 2.5, -9.0), (3.5, -2.5, -9.0), (0.0, 3.5, -9.0), (0.0, -3.5, -9.0), (-3.5, 3.0, -9.0),
                        (0.0, 0.0, TRI_Z), (5.0, 1.0, -12.0), (-7.0, 1.0, -12.0), (40.0, 40.0, -5.0)], f32)
    spread = centres[rng.integers(0, len(centres), 1500)] + rng.uniform(-1.6, 1.6, (1500, 3)).astype(f32)
    targets = np.concatenate([targets, spread.astype(f32)])
    rays = []
    for o in (np.array([0.0, 0.0, 2.0], f32), np.array([0.7, -0.4, 1.0], f32)):
        d = (targets - o).astype(f32)
        d = (d / np.sqrt((d * d).sum(1, keepdims=True))).astype(f32)
        rays.append(np.concatenate([np.broadcast_to(o, d.shape), d], 1))
    # the z = TRI_Z plane seen head-on: the hit point's x and y are the origin's, bit for bit or an ulp off
    head_on = np.concatenate([targets[:, :2], np.full((len(targets), 1), 2.0, f32), np.tile(np.array([0, 0, -1], f32), (len(targets), 1))], 1)
    return np.ascontiguousarray(np.concatenate(rays + [head_on]), f32)


@pytest.mark.parametrize("builder", [None, "device"])
def test_the_hook_gives_the_restated_attenuation(hip, oracle, monkeypatch, builder):
    if builder:
        monkeypatch.setenv("RBRT_BVH_BUILDER", builder)
    else:
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    sc = hook_scene(oracle)
    rays = hook_rays(np.random.default_rng(4))
    exp = NP.surface_albedo(oracle, sc, rays)
    with hip.HipScene(sc) as hs:
        got = hs.surface_albedo(rays)
        if builder is None:
            assert hs.refine_wait(120.0)[0] in (0, 1)
            assert same_bits(hs.surface_albedo(rays), exp)  # (the other trees of the handle)
    bad = np.argwhere(~np.all((bits(got) == bits(exp)) | (np.isnan(got) & np.isnan(exp)), axis=1))[:, 0]
    assert same_bits(got, exp), (len(bad), bad[:5], got[bad[:3]], exp[bad[:3]], rays[bad[:3]])
    _, obj, _, _ = oracle.trace_rays(sc, rays, 0.001, 2000.0)
    table = np_features.object_albedos(sc)
    for k in range(9):  # every object is hit; every patterned one shows both colours, every other one what the header says
        on = obj == k
        assert on.sum() >= 20, k
        colours = {tuple(c) for c in got[on].tolist()}
        if k in sc.pattern_of:
            assert colours == {tuple(table[k].tolist()), tuple(np.array(list(sc.pattern_of[k].albedo2), f32).tolist())}, k
        else:
            assert colours == {tuple(table[k].tolist())}, k
    assert tuple(table[3]) == (1.0, 1.0, 1.0) and tuple(table[4]) == (4.0, 3.0, 2.0)
    assert np.isnan(got[obj < 0]).all() and (obj < 0).sum() >= 20


# ---- images against the restatement -------------------------------------------------------------------------------------------
IMG_W, IMG_H, IMG_SPP, IMG_DEPTH, IMG_SEED = 20, 12, 3, 8, 9


def image_opts(**kw):
    return abi.default_opts(spp=IMG_SPP, seed=IMG_SEED, max_depth=IMG_DEPTH, **kw)


@functools.lru_cache(maxsize=None)
def sphere_reference():
    oracle = _from_oracle()
    cam = scenes.camera(oracle, IMG_W, IMG_H)
    traces = {}
    rad, rgb = NP.restated_image(cam, sphere_scene(), image_opts(), traces=traces)
    rad.setflags(write=False), rgb.setflags(write=False)
    return rad, rgb, traces


def device_image(hip, hs, cam, opts, **kw):
    import torch
    out = torch.full((cam.img_height_pix, cam.img_width_pix, 3), float("nan"), dtype=torch.float32, device="cuda")
    out8 = torch.zeros((cam.img_height_pix, cam.img_width_pix, 3), dtype=torch.uint8, device="cuda")
    hs.render_device(cam, opts, out.data_ptr(), out8.data_ptr(), **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), out8.cpu().numpy()


@pytest.mark.parametrize("short_paths", [0, 2])
def test_sphere_scene_gives_the_restated_image(hip, oracle, short_paths):
    """Ragged tiles both ways; the short-path stage off and on every launch (the ground sphere is what it finishes)."""
    cam = scenes.camera(oracle, IMG_W, IMG_H)
    exp, exp8, traces = sphere_reference()
    assert sum(1 for tr in traces.values() for _, second in tr if second) > 50  # (the second colour is in the paths)
    with hip.HipScene(sphere_scene()) as hs:
        hs.set_short_paths(short_paths)
        got, got8 = device_image(hip, hs, cam, image_opts())
        if short_paths:
            masks = hs.short_masks()
            assert len(masks) and np.any(masks != 0)  # (the stage finished samples itself)
        hs.check()
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    plain, _ = hip.render_scene(cam, IMG_SPP, sphere_scene(None), seed=IMG_SEED, max_depth=IMG_DEPTH)
    assert not np.array_equal(bits(plain), bits(got))


MESH_PIXELS = [(r, c) for r in range(2, 24, 3) for c in range(1, 32, 4)]


def mesh_scene(oracle):
    """A patterned smooth stand-in mesh of 203 triangles and a patterned BasicTriangle on the example's spheres."""
    smooth = np_smooth.standin_smooth(oracle, 203, 45.0, (5.0, -1.8, -12.5), abi.material(L, (0.7, 0.3, 0.2)), "computed")
    tri = [(((-6.0, 0.02, -5.0), (1.0, 0.02, -5.5), (-3.0, 3.5, -8.5)), abi.material(L, (0.8, 0.3, 0.1)))]
    n_elem = len(scenes.EXAMPLE_SPHERES) + 1
    pats = {n_elem - 1: abi.checker((0.1, 0.3, 0.8), 0.3, (0.11, -0.07, 0.23)), n_elem: abi.checker((0.2, 0.7, 0.3), 0.7, (0.5, 0.25, -0.125))}
    return abi.SceneData(spheres=scenes.EXAMPLE_SPHERES, triangles=tri, meshes=[smooth], patterns=pats)


@functools.lru_cache(maxsize=None)
def mesh_reference():
    oracle = _from_oracle()
    cam = scenes.camera(oracle, 32, 24)
    traces = {}
    rad, _ = NP.restated_image(cam, mesh_scene(oracle), abi.default_opts(spp=2, seed=5, max_depth=6), MESH_PIXELS, traces)
    rad.setflags(write=False)
    return rad, traces


@pytest.mark.parametrize("builder", [None, "device"])
def test_mesh_and_triangle_give_the_restated_pixels_on_both_trees(hip, oracle, monkeypatch, builder):
    if builder:
        monkeypatch.setenv("RBRT_BVH_BUILDER", builder)
    else:
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    cam = scenes.camera(oracle, 32, 24)
    sc = mesh_scene(oracle)
    exp, traces = mesh_reference()
    seen = {(o, s) for tr in traces.values() for o, s in tr}
    n_elem = len(sc.spheres) + len(sc.triangles)
    assert {(n_elem - 1, 0), (n_elem - 1, 1), (n_elem, 0), (n_elem, 1)} <= seen  # both colours of the triangle and of the mesh
    rows, cols = np.array([p[0] for p in MESH_PIXELS]), np.array([p[1] for p in MESH_PIXELS])
    opts = abi.default_opts(spp=2, seed=5, max_depth=6)
    with hip.HipScene(sc) as hs:
        got, _ = device_image(hip, hs, cam, opts)
        assert np.array_equal(bits(got[rows, cols]), bits(exp[rows, cols])), "first trees"
        if builder is None:
            assert hs.refine_wait(120.0)[0] in (0, 1)
            again, _ = device_image(hip, hs, cam, opts)
            assert np.array_equal(bits(again), bits(got)), "the refined trees"
        hs.check()


# ---- long records --------------------------------------------------------------------------------------------------------------
def facing_scene():
    """Two large patterned spheres facing each other, the camera in the gap between them: a path bounces from one to the other
    until it leaves through the rim, where the sky is."""
    spheres = [((0.0, -1000.0, -5.0), 1000.0, abi.material(L, (0.95, 0.9, 0.85))), ((0.0, 1008.0, -5.0), 1000.0, abi.material(L, (0.9, 0.95, 0.8)))]
    return abi.SceneData(spheres=spheres, patterns={0: abi.checker((0.8, 0.9, 0.97), 3.0, (0.4, -1.5, 0.2)),
                                                    1: abi.checker((0.97, 0.8, 0.9), 2.5, (0.1, 0.3, -0.2))})


def test_long_records_carry_second_entries_through_the_spilled_words(hip, oracle):
    cam = scenes.camera(oracle, 8, 8)
    opts = abi.default_opts(spp=2, seed=21, max_depth=50)
    traces = {}
    exp, exp8 = NP.restated_image(cam, facing_scene(), opts, traces=traces)
    # paths that reached the sky (a black path shows nothing of its record) after more than four and more than eight recorded
    # bounces, with a second entry in one of the first four of them: that byte was written to a gseq word and read back
    lit = {k: tr for k, tr in traces.items() if len(tr) < 50}
    over4 = [k for k, tr in lit.items() if len(tr) > 4 and any(s for _, s in tr[:4])]
    over8 = [k for k, tr in lit.items() if len(tr) > 8 and any(s for _, s in tr[:4]) and any(s for _, s in tr[4:8])]
    assert len(over4) >= 5 and len(over8) >= 3, (len(over4), len(over8))
    with hip.HipScene(facing_scene()) as hs:
        got, got8 = device_image(hip, hs, cam, opts)
        hs.check()
    for row, col, _ in over4 + over8:
        assert np.array_equal(bits(got[row, col]), bits(exp[row, col])) and np.any(exp[row, col] > 0), (row, col)
    assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8)


# ---- the limit -----------------------------------------------------------------------------------------------------------------
def limit_scene(n):
    """n lambertian spheres in a grid in front of the camera, every one patterned: entries n .. 2n - 1 are the second ones."""
    spheres, pats = [], {}
    for k in range(n):
        i, j = k % 16, k // 16
        last = k == n - 1
        c = (0.0, 3.0, -4.0) if last else (-9.0 + 1.2 * i, -1.0 + 1.1 * j, -14.0)  # the last one large, in front of the others
        spheres.append((c, 1.5 if last else 0.5, abi.material(L, (0.2 + 0.005 * k, 0.5, 0.9 - 0.005 * k))))
        pats[k] = abi.checker((0.9 - 0.005 * k, 0.3, 0.1 + 0.005 * k), 0.3, (0.11, -0.07, 0.23))
    return abi.SceneData(spheres=spheres, patterns=pats)


def test_as_many_entries_as_the_record_byte_holds(hip, oracle):
    n = 128  # 128 objects + 128 patterns = 256 entries: the last second entry is number 255
    cam = scenes.camera(oracle, 16, 16)
    sc = limit_scene(n)
    opts = abi.default_opts(spp=2, seed=3, max_depth=4)
    rays = np_features.primary_rays(cam, opts.seed, opts.spp)
    _, obj, _, _ = oracle.trace_rays(sc, np.ascontiguousarray(rays.reshape(-1, 6)), opts.min_dist, opts.max_dist)
    obj = obj.reshape(16, 16, opts.spp)
    pixels = [(r, c) for r in range(16) for c in range(16) if np.all(obj[r, c] == n - 1)][:12]
    assert len(pixels) >= 6
    traces = {}
    exp, _ = NP.restated_image(cam, sc, opts, pixels, traces)
    odd_last = {(k[0], k[1]) for k, tr in traces.items() if (n - 1, 1) in tr}
    assert len(odd_last) >= 3  # pixels whose paths record entry 255
    got, _ = hip.render_scene(cam, opts.spp, sc, seed=opts.seed, max_depth=opts.max_depth)
    for r, c in pixels:
        assert np.array_equal(bits(got[r, c]), bits(exp[r, c])), (r, c)
    # one pattern more: 129 objects and 128 patterns
    more = limit_scene(n)
    one_more = abi.SceneData(spheres=more.spheres + [((0.0, 30.0, -14.0), 0.5, abi.material(L, (0.5, 0.5, 0.5)))], patterns=more.pattern_of)
    with pytest.raises(abi.RbrtError) as e:
        hip.HipScene(one_more)
    assert e.value.code == abi.RBRT_ERR_UNSUPPORTED


# ---- anchors to the oracle -----------------------------------------------------------------------------------------------------
def test_equal_colours_give_the_oracles_image(hip, oracle):
    cam = scenes.camera(oracle, 24, 16)
    plain = scenes.triangle_scene(oracle, 203)
    opts = abi.default_opts(spp=4, seed=2)
    order = plain.element_order
    mats = [plain.triangles[e & 0x7FFFFFFF][1] if e >> 31 else plain.spheres[e][2] for e in order] + [m.struct.mat for m in plain.meshes]
    pats = {k: abi.checker(tuple(m.albedo), 0.3, (0.11, -0.07, 0.23)) for k, m in enumerate(mats) if m.kind == L}
    assert len(pats) >= 3
    sc = abi.SceneData(spheres=plain.spheres, meshes=plain.meshes, triangles=plain.triangles, element_order=order, patterns=pats)
    got, got8 = hip.render_scene(cam, 4, sc, seed=2)
    exp, exp8, _ = oracle.render(cam, plain, opts)
    assert np.array_equal(bits(got), bits(exp)) and np.array_equal(got8, exp8)


def test_swapped_colours_and_a_shifted_origin_give_the_same_image(hip, oracle):
    cam = scenes.camera(oracle, IMG_W, IMG_H)
    ref, _ = hip.render_scene(cam, IMG_SPP, sphere_scene(), seed=IMG_SEED, max_depth=IMG_DEPTH)
    assert np.array_equal(bits(ref), bits(sphere_reference()[0]))
    for origin in ((2.0, -1.0, 0.0), (0.0, -3.0, 0.0), (0.0, -1.0, 2.0), (0.0, 1.0, 0.0)):
        sc = sphere_scene(abi.checker(A1, 2.0, origin), ground=A2)
        got, _ = hip.render_scene(cam, IMG_SPP, sc, seed=IMG_SEED, max_depth=IMG_DEPTH)
        assert np.array_equal(bits(got), bits(ref)), origin


def test_an_unpatterned_scene_through_create_patterned_is_create_shaded(hip, oracle):
    lib = abi.load_hip()
    cam = scenes.camera(oracle, 24, 16)
    sc = scenes.triangle_scene(oracle, 203)
    opts = abi.default_opts(spp=3, seed=6)
    n_obj = len(sc.spheres) + len(sc.triangles) + len(sc.meshes)
    none = (abi.Pattern * n_obj)()

    class Raw(hip.HipScene):
        def __init__(self, make):
            self._lib, self._h, self.device, self.scene = lib, C.c_void_p(), 0, sc
            abi.check(make(C.byref(self._h)))

    results = []
    makers = [lambda h: lib.rbrt_hip_scene_create_shaded(sc.ptr(), None, 0, h),
              lambda h: lib.rbrt_hip_scene_create_patterned(sc.ptr(), None, None, 0, h),
              lambda h: lib.rbrt_hip_scene_create_patterned(sc.ptr(), None, C.byref(abi.ScenePatterns(n_obj, 0, None)), 0, h),
              lambda h: lib.rbrt_hip_scene_create_patterned(sc.ptr(), None, C.byref(abi.ScenePatterns(n_obj, 0, none)), 0, h)]
    for make in makers:
        with Raw(make) as hs:
            results.append((device_image(hip, hs, cam, opts)[0], hs.info()["lds_bytes_per_wave"]))
    for img, lds in results[1:]:
        assert np.array_equal(bits(img), bits(results[0][0])) and lds == results[0][1]
    assert np.array_equal(bits(results[0][0]), bits(oracle.render(cam, sc, opts)[0]))
    with hip.HipScene(sphere_scene()) as hp, hip.HipScene(sphere_scene(None)) as hn:
        assert hp.info()["lds_bytes_per_wave"] == hn.info()["lds_bytes_per_wave"] + 4 * 9  # a second entry and a record


# ---- every entry point -----------------------------------------------------------------------------------------------------------
def test_every_entry_point_gives_the_same_image(hip, oracle):
    import torch
    w, h, spp = IMG_W, IMG_H, IMG_SPP
    cam = scenes.camera(oracle, w, h)
    sc = sphere_scene()
    opts = image_opts()
    exp = sphere_reference()[0]

    def img():
        return torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")

    def same(t, what):
        torch.cuda.synchronize()
        assert np.array_equal(bits(t.cpu().numpy()), bits(exp)), what

    one_shot, _ = hip.render_scene(cam, spp, sc, seed=IMG_SEED, max_depth=IMG_DEPTH)
    assert np.array_equal(bits(one_shot), bits(exp)), "rbrt_hip_render_patterned"
    with hip.HipScene(sc) as hs:
        out = img()
        hs.render_device(cam, opts, out.data_ptr())
        same(out, "render_device")
        acc = torch.full((hip.packed_pixels(w, h, 0, 1) * 3,), float("nan"), dtype=torch.float32, device="cuda")
        out = img()
        hs.render_pass(cam, opts, 0, 2, acc.data_ptr(), None)
        hs.render_pass(cam, opts, 2, spp, acc.data_ptr(), out.data_ptr())
        same(out, "render_pass in two passes")
        out = img()
        hs.render_adaptive(cam, opts, 0.0, min_samples=2, step=1, d_radiance=out.data_ptr())
        same(out, "render_adaptive, threshold 0")
        world = 2
        slot = hip.packed_pixels(w, h, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            hs.render_device(cam, image_opts(tile_rank=r, tile_world=world), slots[r * slot * 3:].data_ptr())
        merged = img()
        hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        same(merged, "two ranks, unpacked")
        out = img()
        hs.render_device(cam, image_opts(flags=abi.FLAG_COLLECT_STATS), out.data_ptr())
        same(out, "the counting kernel")
        hs.check()


def lens_scene():
    """The sphere scene with a patterned BasicTriangle: its tables sit behind the materials in LDS, the lens words behind them."""
    s = sphere_scene()
    tri = [(((2.0, 0.02, -6.0), (5.5, 0.02, -7.0), (3.0, 2.0, -9.5)), abi.material(L, (0.8, 0.3, 0.1)))]
    pats = dict(s.pattern_of)
    pats[len(s.spheres)] = abi.checker((0.1, 0.3, 0.8), 0.3, (0.11, -0.07, 0.23))
    return abi.SceneData(spheres=s.spheres, triangles=tri, patterns=pats)


def test_a_lens_launch_and_an_environment_keep_the_tables_apart(hip, oracle):
    """Both put words behind the scene tables in LDS, which the patterns lengthen. The lens image against the restatement;
    with an environment, the pattern's image with the short-path stage off and on, and equal colours against no pattern."""
    cam = scenes.camera(oracle, 12, 8)
    sc = lens_scene()
    opts = abi.default_opts(spp=2, seed=4, max_depth=6)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 7.0, 10.0)
    exp, _ = NP.restated_image(cam, sc, opts, lens=lens)
    rng = np.random.default_rng(8)
    env = rng.uniform(0.0, 2.0, (5, 5, 3)).astype(f32)
    equal = abi.SceneData(spheres=sc.spheres, triangles=sc.triangles,
                          patterns={k: abi.checker(tuple((sc.spheres + sc.triangles)[k][-1].albedo), p.size, tuple(p.origin)) for k, p in sc.pattern_of.items()})
    plain = abi.SceneData(spheres=sc.spheres, triangles=sc.triangles)
    with hip.HipScene(sc) as hs, hip.HipScene(equal) as he, hip.HipScene(plain) as hp:
        got, _ = device_image(hip, hs, cam, opts, lens=lens)
        assert np.array_equal(bits(got), bits(exp)), "thin lens"
        for x in (hs, he, hp):
            x.set_environment(env)
        images = []
        for mode in (0, 2):
            hs.set_short_paths(mode)
            images.append(device_image(hip, hs, cam, opts, lens=lens)[0])
        assert np.array_equal(bits(images[0]), bits(images[1])), "environment + lens: the short-path stage"
        e, _ = device_image(hip, he, cam, opts, lens=lens)
        p, _ = device_image(hip, hp, cam, opts, lens=lens)
        assert np.array_equal(bits(e), bits(p)), "environment + lens: equal colours"
        assert not np.array_equal(bits(images[0]), bits(p)) and np.isfinite(images[0]).all()
        # without the lens the paths that end on a hit or stay black are the restatement's, whatever the rays that escape see
        hs.set_environment(None)
        assert np.array_equal(bits(device_image(hip, hs, cam, opts)[0]), bits(NP.restated_image(cam, sc, opts)[0]))
        hs.check()


# ---- features ------------------------------------------------------------------------------------------------------------------
def test_features_give_the_cells_colour_per_sample(hip, oracle):
    import torch
    cam = scenes.camera(oracle, 16, 16)
    sc = sphere_scene()
    opts = abi.default_opts(spp=1, seed=7)
    exp_a, exp_obj, straddles = NP.feature_albedo(oracle, cam, sc, opts, 4)
    assert sum(straddles) >= 5  # pixels whose four samples saw both colours of the ground: their albedo is a mean
    a = torch.full((16, 16, 3), float("nan"), dtype=torch.float32, device="cuda")
    o = torch.full((16, 16), -7, dtype=torch.int32, device="cuda")
    with hip.HipScene(sc) as hs:
        hs.render_features(cam, opts, 4, d_albedo=a.data_ptr(), d_object=o.data_ptr())
        torch.cuda.synchronize()
    assert np.array_equal(bits(a.cpu().numpy()), bits(exp_a)), np.argwhere(bits(a.cpu().numpy()) != bits(exp_a))[:5]
    assert np.array_equal(o.cpu().numpy(), exp_obj)
    plain_a = np_features.features(oracle, cam, sphere_scene(None), opts, 4).albedo
    assert not np.array_equal(bits(plain_a), bits(exp_a))


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def test_the_cli_writes_the_librarys_bytes(hip, tmp_path):
    w, h, spp, seed = 28, 20, 2, 3
    out, pfm = tmp_path / "o.png", tmp_path / "o.pfm"
    r = subprocess.run([str(EXE), "-c", str(SHIPPED), "-t", str(out), "--height", str(h), "-w", str(w), "-s", str(spp), "--seed", str(seed),
                        "--radiance", str(pfm)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    host = abi.HostScene(SHIPPED, h, w)
    assert host.patterns_ptr() is not None
    got, _ = hip.render_scene(host.camera, spp, host, seed=seed)
    assert np.array_equal(bits(abi.read_pfm(pfm, any_value=True)), bits(got))
    # ... which is the restatement's image of the same scene, so the checker is in it
    st = host.struct
    spheres = [(tuple(st.spheres[i].center), st.spheres[i].radius, st.spheres[i].mat) for i in range(st.n_spheres)]
    sc = abi.SceneData(spheres=spheres, patterns={0: host.patterns.objects[0]})
    exp, _ = NP.restated_image(host.camera, sc, abi.default_opts(spp=spp, seed=seed), [(r_, c_) for r_ in (10, 15, 19) for c_ in range(0, w, 3)])
    for r_ in (10, 15, 19):
        for c_ in range(0, w, 3):
            assert np.array_equal(bits(got[r_, c_]), bits(exp[r_, c_])), (r_, c_)
