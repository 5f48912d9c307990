"""Scenes and host-side restatements for test_short_paths_scenes_gpu.py and test_short_paths_conditions.py: the inputs on
which the short-path stage (short_paths.inl) had never run -- more elements than the culling word has bits for, element
orders in which position and sphere index disagree around 24, several meshes, images smaller than a tile, batches longer
than one mask -- and the stage's rule walked sample by sample through np_reference, so that a condition on an input ("some
second ray's closest hit is element 24 or later") is computed, not hoped for.

The walk is test_short_paths_gpu.restated_masks with three additions: it keeps what each ray hit, it knows emitters (a ray
that ends on one ends the path: classify() in megakernel.inl), and it takes a lens. Where a scene has meshes its `fin` is
not the stage's (the stage declines a second ray that passes a mesh's box, which is not restated here): only the hits are
used there."""
from __future__ import annotations

import numpy as np

import np_lens
import np_reference as R
import np_smooth
import scenes
import test_np_reference as T
from rbrt_amd import abi

f32 = np.float32
L, M, D, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
GROUND = ((0.0, -1000.0, -5.0), 1000.0, abi.material(L, (0.02, 0.2, 0.1)))
TRI = 0x80000000
PROBE, KEEP_NUM, KEEP_DEN = 2, 3, 4  # short_paths.inl: kShortProbe, kShortKeepNum / kShortKeepDen

# ---- cameras -----------------------------------------------------------------------------------------------------------------
DOWN = dict(look_at=(0.0, -0.7, -1.0))        # the example camera tilted down: the ground from z = 0 to z = -30 fills the image
CEILING_LOOK = dict(look_at=(0.0, -1.0, -0.3))  # test_short_paths_gpu's camera under the ceiling


def ceiling_scene():
    """test_short_paths_gpu's "under a ceiling": a second huge sphere eight units above the ground."""
    return abi.SceneData(spheres=[GROUND, ((0.0, 1008.0, -5.0), 1000.0, abi.material(L, (0.5, 0.6, 0.7)))])


def overhang_scene():
    """A sphere of radius 6 hanging over one side of the ground the CEILING_LOOK camera sees: under it about half the second rays
    escape, beside it most do -- the stage gives tiles up whose probe finished some samples, and keeps others."""
    return abi.SceneData(spheres=[GROUND, ((7.0, 6.0, 2.5), 6.0, abi.material(L, (0.5, 0.6, 0.7)))])


COVERED = {"ceiling": ceiling_scene, "overhang": overhang_scene}


# ---- 1. more elements than element bits --------------------------------------------------------------------------------------
def _mat(k):
    kind = (L, M, D, EM)[k % 4]
    if kind == L:
        return abi.material(L, (0.2 + 0.1 * (k % 7), 0.8 - 0.1 * (k % 5), 0.5))
    if kind == M:
        return abi.material(M, (0.9, 0.8, 0.7), 0.05 * (k % 4))
    if kind == D:
        return abi.material(D, (0, 0, 0), 1.5)
    return abi.material(EM, (3.0, 2.5, 2.0))


def small_spheres(n):
    """n spheres of radius 0.7 on the ground, the n most central places of an 8 x 4 grid in front of the DOWN camera, the
    outermost first: the spheres with the highest indices are in the middle of the image. Materials in turn: lambertian,
    metal, glass, emitter."""
    places = [(-5.25 + 1.5 * i, -3.0 - 2.0 * j) for j in range(4) for i in range(8)]
    places.sort(key=lambda p: (p[0] ** 2 + (p[1] + 5.0) ** 2, p))
    places = places[:n][::-1]
    return [((x, 0.7, z), 0.7, _mat(k)) for k, (x, z) in enumerate(places)]


def grid_scene(n_total):
    """The ground and n_total - 1 small spheres: n_total elements, positions = sphere indices."""
    return abi.SceneData(spheres=[GROUND] + small_spheres(n_total - 1))


# 26 spheres and scenes.TRIANGLES' four BasicTriangles, 30 elements: spheres 25 and 24 at positions 2 and 3, triangles at
# positions 1 and 23, spheres 20 to 23 at positions 24 to 27 (an element bit belongs to a POSITION: primary_cull_kernel).
MIXED_ORDER = [0, TRI | 0, 25, 24] + list(range(1, 20)) + [TRI | 3, 20, 21, 22, 23, TRI | 1, TRI | 2]


def mixed_scene():
    return abi.SceneData(spheres=[GROUND] + small_spheres(25), triangles=scenes.TRIANGLES, element_order=MIXED_ORDER)


def check_mixed_order():
    o = MIXED_ORDER
    assert len(o) == 30 and sorted(e for e in o if not e >> 31) == list(range(26)) and sorted(e & 0xFF for e in o if e >> 31) == [0, 1, 2, 3]
    assert any(not e >> 31 and e >= 24 and p < 24 for p, e in enumerate(o))   # a sphere with index >= 24 at a position < 24
    assert any(not e >> 31 and e < 24 and p >= 24 for p, e in enumerate(o))   # a sphere with index < 24 at a position >= 24
    assert any(e >> 31 and p < 24 for p, e in enumerate(o))                   # a triangle at a position < 24


ELEMENT_SCENES = {"grid24": lambda: grid_scene(24), "grid25": lambda: grid_scene(25), "grid32": lambda: grid_scene(32), "mixed30": mixed_scene}
ELEMENT_SIZE, ELEMENT_OPTS = (32, 24), dict(spp=3, seed=17)


def element_camera(oracle):
    return scenes.camera(oracle, *ELEMENT_SIZE, **DOWN)


def grid_and_mesh_scene(oracle):
    """grid32 and a mesh at the right edge: the only kind of scene in which a tile of the stage has a set bit at 24 or above
    (the mesh's) AND elements at positions 24 and above."""
    mesh = scenes.standin_mesh(oracle, 12, 30.0, (7.5, -2.4, -10.0), (0.0, 0.0, 0.0), abi.material(L, (0.9, 0.2, 0.2)))
    return abi.SceneData(spheres=[GROUND] + small_spheres(31), meshes=[mesh])


# ---- 2. several meshes -------------------------------------------------------------------------------------------------------
MESH_PLACES = [(-3.6, -4.0), (0.3, -4.0), (4.0, -4.0), (-1.5, -7.0), (-3.5, -12.5), (7.5, -13.0), (-8.5, -14.0), (5.5, -19.0)]
MESH_SIZE, MESH_OPTS = (96, 64), dict(spp=3, seed=23)


def mesh_scene(oracle, n):
    """The example spheres and n small stand-in meshes (12 triangles, about 1.3 x 0.9 x 1.0) standing apart on the ground."""
    kinds = [abi.material(L, (0.9, 0.2, 0.2)), abi.material(M, (0.8, 0.8, 0.6), 0.1), abi.material(D, (0, 0, 0), 1.5)]
    meshes = [scenes.standin_mesh(oracle, 12, 14.0, (x, -1.12, z), (0.0, 0.0, 0.0), kinds[k % 3]) for k, (x, z) in enumerate(MESH_PLACES[:n])]
    assert all(m.n_real == 12 for m in meshes)
    return abi.SceneData(spheres=scenes.EXAMPLE_SPHERES, meshes=meshes)


def mesh_camera(oracle):
    return scenes.camera(oracle, *MESH_SIZE, **DOWN)


# Tiles (ty, tx) of mesh_camera's image next to mesh 0 and next to the last mesh, which the culling table of the device gives
# to the stage (asserted in the GPU test) and from which second rays reach those meshes (asserted in the CPU test).
NEIGHBOUR_TILES = {2: {0: (3, 3), 1: (4, 5)}, 7: {0: (3, 3), 6: (1, 0)}}


# ---- the walk ----------------------------------------------------------------------------------------------------------------
NO_RAY, RAGGED = -2, -3  # in `first` / `second`: there was no such ray; the slot is beyond the image's edge


def walk(cam, sc, opts, tile_list, lens=None):
    """Every sample of the launch (opts.spp of them) of the tiles in tile_list [(ty, tx), ...], pixel slot by pixel slot:
    {(ty, tx): (first, second, fin)}, int arrays [spp, 64] of the position of the camera ray's and the second ray's closest
    hit (scene_hit's obj: an element's position, number of elements + k for mesh k, -1 for nothing) and the bool array of the
    samples a stage without meshes finishes."""
    nc, ns = T.np_cam(cam), np_smooth.np_scene(sc)
    H, W = nc["H"], nc["W"]
    lo, hi = f32(opts.min_dist), f32(opts.max_dist)
    out = {}
    for ty, tx in tile_list:
        first = np.full((opts.spp, 64), RAGGED, np.int64)
        second = np.full((opts.spp, 64), NO_RAY, np.int64)
        fin = np.ones((opts.spp, 64), bool)  # (a slot beyond a ragged edge counts as finished)
        for s in range(opts.spp):
            for p in range(64):
                row, col = ty * 8 + p // 8, tx * 8 + p % 8
                if not (row < H and col < W):
                    continue
                rng = R.Rng(opts.seed, row * W + col, s)
                o, d = R.camera_ray(nc, row, col, rng) if lens is None else np_lens.camera_ray_lens(nc, lens, row, col, rng)
                hit = R.scene_hit(ns, o, d, lo, hi)
                first[s, p] = -1 if hit is None else hit["obj"]
                if hit is None or opts.max_depth == 0 or hit["mat"][0] == EM:
                    continue
                ok, _, o2, d2 = R.scatter(hit["mat"], d, hit, rng)
                if not ok:
                    continue
                hit2 = R.scene_hit(ns, o2, d2, lo, hi)
                second[s, p] = -1 if hit2 is None else hit2["obj"]
                fin[s, p] = hit2 is None or opts.max_depth == 1 or hit2["mat"][0] == EM
        out[(ty, tx)] = (first, second, fin)
    return out


def tile_masks(fin):
    """The masks of one tile of the stage from its walk's `fin`, and whether the stage gave the tile up after the probe:
    it goes on only if at least three quarters of the first two samples' 128 slots finished."""
    spp = fin.shape[0]
    raw = [sum(int(b) << p for p, b in enumerate(row)) for row in fin]
    probe = int(fin[:PROBE].sum())
    gave_up = spp > PROBE and probe * KEEP_DEN < PROBE * 64 * KEEP_NUM
    return (raw[:PROBE] + [0] * (spp - PROBE) if gave_up else raw), gave_up


def work_tiles(cull):
    return [tuple(t) for t in np.argwhere((cull >> 31) == 0).tolist()]


def restated_masks(cam, sc, opts, cull, lens=None, walked=None):
    """test_short_paths_gpu.restated_masks for scenes that may have emitters, an element order and a lens (no meshes)."""
    assert not sc.meshes
    walked = walked if walked is not None else walk(cam, sc, opts, work_tiles(cull), lens)
    out = []
    for t in work_tiles(cull):
        out += tile_masks(walked[t][2])[0]
    return sorted(out)


def assert_masks(masks, cam, sc, opts, cull, what, lens=None, walked=None):
    exp = restated_masks(cam, sc, opts, cull, lens, walked)
    assert sorted(int(m) for m in masks) == exp, f"{what}: the finished masks are not the restated rule's"


_WALKS = {}


def element_walk(oracle, name):
    """The walk of ELEMENT_SCENES[name] over every tile of element_camera's image, made once."""
    if name not in _WALKS:
        cam = element_camera(oracle)
        tiles = [(ty, tx) for ty in range((ELEMENT_SIZE[1] + 7) // 8) for tx in range((ELEMENT_SIZE[0] + 7) // 8)]
        _WALKS[name] = walk(cam, ELEMENT_SCENES[name](), abi.default_opts(**ELEMENT_OPTS), tiles)
    return _WALKS[name]


# ---- 3. a lens and a mesh ----------------------------------------------------------------------------------------------------
WIDE_APERTURE_MM = 600.0  # a lens 0.6 units across: wide enough to bring a mesh's box into reach of more tiles


# ---- 4. the cull fuzz through the stage --------------------------------------------------------------------------------------
N_FUZZ, FUZZ_BASE = 24, 96000


def fuzz_case(oracle, k, base=None):
    """Case k: test_primary_cull's fuzz_scene and fuzz_camera from the seed base + k, 9 to 48 pixels each way, 1 to 4 samples,
    max_depth 12, a lens on every third case. `mode` is fuzz_camera's (its first draw); `on_sphere`: the camera is inside a
    sphere, on its surface or within a thousandth of its radius of it (modes 1 to 3 of a scene that has spheres)."""
    import copy
    from types import SimpleNamespace

    import test_primary_cull as PC
    rng = np.random.default_rng((FUZZ_BASE if base is None else base) + k)
    sc = PC.fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 49)), int(rng.integers(9, 49))
    mode = int(copy.deepcopy(rng).integers(0, 8))
    cam = PC.fuzz_camera(oracle, rng, sc, w, h)
    spp = int(rng.integers(1, 5))
    lens = None
    if k % 3 == 2:
        r, focus = float(rng.uniform(0.005, 0.1)), float(rng.uniform(3.0, 15.0))
        plane = float(np.linalg.norm(np.array(list(cam.img_center_point), np.float64) - np.array(list(cam.position), np.float64)))
        lens = (tuple(r * float(x) for x in cam.right), tuple(r * float(x) for x in cam.up), focus / plane)
    return SimpleNamespace(sc=sc, cam=cam, w=w, h=h, mode=mode, on_sphere=bool(sc.spheres) and mode in (1, 2, 3), lens=lens,
                           opts=abi.default_opts(spp=spp, seed=k, max_depth=12))


# ---- 5. masks nobody rewrote -------------------------------------------------------------------------------------------------
def two_camera_scene(oracle):
    """The ground and a mesh about 2.7 x 1.9 x 2.1 standing on it at z = -10."""
    mesh = scenes.standin_mesh(oracle, 12, 30.0, (0.0, -2.4, -10.0), (0.0, 0.0, 0.0), abi.material(L, (0.9, 0.2, 0.2)))
    return abi.SceneData(spheres=[GROUND], meshes=[mesh])


TWO_CAMERAS = dict(up=(0.0, 0.0, -1.0), focal_mm=80.0)
_FAR = (float(np.sin(0.5)), float(np.cos(0.5)), 0.0)  # half a radian round the ground sphere from the mesh


def camera_away(oracle):
    """Three units above the ground half a radian (480 units) round its sphere from the mesh, looking straight down: the
    mesh is out of view, and 120 units below the horizon of every ground point in view -- no scattered ray can pass its box
    either, so with max_depth 1 the stage finishes every sample."""
    c = GROUND[0]
    position = tuple(c[k] + 1003.0 * _FAR[k] for k in range(3))
    return scenes.camera(oracle, 16, 16, position=position, look_at=tuple(-x for x in _FAR), **TWO_CAMERAS)


def camera_at_the_mesh(oracle):
    """Three units in front of the mesh with a long lens: every pixel's ray enters the mesh's box."""
    return scenes.camera(oracle, 16, 16, position=(-0.5, 1.0, -6.0), look_at=(0.0, 0.0, -1.0), up=(0.0, 1.0, 0.0), focal_mm=80.0)


# ---- 6. smaller than a tile --------------------------------------------------------------------------------------------------
SMALL_SIZES, SMALL_OPTS = [(1, 1), (5, 3), (8, 8), (9, 8)], dict(spp=4, seed=37)


def small_case(oracle, scene, size):
    if scene == "ceiling":
        return ceiling_scene(), scenes.camera(oracle, *size, **CEILING_LOOK)
    return scenes.spheres_scene(), scenes.camera(oracle, *size)
