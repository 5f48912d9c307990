"""The numpy restatement of the feature buffers (np_features.py) pinned from two independent sides, without a GPU: the CPU
oracle's render of a scene made only of emitters must be its albedo buffer bit for bit, and the hits it takes from the oracle
must be those of the pure-numpy Scene::hit. Then the edge cases: an empty scene, and a sphere on the optical axis."""
import numpy as np
import pytest

import np_features as F
import np_lens
import np_reference as R
import np_smooth
import scenes
from rbrt_amd import abi

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def lens_of(cam):
    """full_scenes.all_features_camera's lens: 20 mm of aperture, focused at 9 units."""
    return np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 20.0, 9.0)


@pytest.mark.parametrize("with_lens", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("w,h", [(37, 21), (16, 16)])
def test_an_emitters_only_scene_renders_to_its_albedo_buffer(oracle, w, h, with_lens):
    """Both are the same sums of L and +0 in sample order, times 1.0f / n: the oracle's render shares no code with the table."""
    cam = scenes.camera(oracle, w, h)
    lens = lens_of(cam) if with_lens else None
    sc = F.emitter_scene(oracle)
    rays = F.primary_rays(cam, 3, 5, lens)
    seen = set()
    for n in (1, 2, 5):
        opts = F.emitter_opts(n)
        rad, _, _ = oracle.render(cam, sc, opts, want_rgb8=False, lens=lens)
        got = F.features(oracle, cam, sc, opts, n, lens, rays=rays)
        assert np.array_equal(bits(rad), bits(got.albedo)), (w, h, n, with_lens)
        # ... and the other buffers agree with it about what is covered
        assert np.array_equal(got.coverage > 0, rad.sum(-1) > 0)
        assert ((got.depth > 0) == (got.coverage > 0)).all() and (got.coverage <= 1).all()
        seen |= set(np.unique(got.object).tolist())
    assert seen == {-1, 0, 1, 2, 3}  # every emitter and the background are in view
    assert rad.max() > 4.0  # (radiance above 1 comes through)


def mixed_scene(oracle):
    """All four materials on spheres and BasicTriangles in a mixed element order, a flat and a smooth mesh."""
    flat = scenes.standin_mesh(oracle, 203, **scenes.EXAMPLE_MESH)
    smooth = np_smooth.standin_smooth(oracle, 157, 30.0, (-1.0, -1.3, -6.5), abi.material(abi.MAT_METAL, (0.8, 0.8, 0.75), 0.05), "computed")
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(abi.MAT_EMISSIVE, (3.0, 2.5, 1.5)))]
    return abi.SceneData(spheres=sph, meshes=[flat, smooth], triangles=scenes.TRIANGLES, element_order=scenes.TRIANGLE_ORDER + [4])


def test_the_hits_are_those_of_the_pure_numpy_scene_hit(oracle):
    cam = scenes.camera(oracle, 40, 30)
    sc = mixed_scene(oracle)
    ns = np_smooth.np_scene(sc)
    pix = F.all_pixels(cam)[::6]
    assert len(pix) == 200
    rays = F.primary_rays(cam, 11, 1, None, pix)[:, 0]
    obj, dist, g = F.hits(oracle, sc, rays, 0.001, 2000.0)
    kinds = set()
    for k, ray in enumerate(rays):
        h = np_smooth.scene_hit(ns, ray[:3].copy(), ray[3:].copy(), f32(0.001), f32(2000.0))
        if h is None:
            assert obj[k] == -1 and np.isnan(g[k]).all(), k
            continue
        assert h["obj"] == obj[k], k
        assert bits(h["dist"]) == bits(dist[k]), k
        assert np.array_equal(bits(h["normal"]), bits(g[k])), k
        kinds.add("mesh" if h["tri"] >= 0 else "elem")
        kinds.add(int(obj[k]))
    assert {"mesh", "elem", 9, 10} <= kinds and (obj == -1).any()  # both meshes, elements and the sky
    # the table on top of them, by hand for a few rays
    got = F.from_hits(sc, obj[:, None], dist[:, None], g[:, None], 1)
    table = F.object_albedos(sc)
    assert np.array_equal(table[3], f32([1, 1, 1])) and np.array_equal(table[8], f32([3.0, 2.5, 1.5]))  # glass, the lamp
    for k in range(0, 200, 7):
        if obj[k] < 0:
            assert not got.albedo[k].any() and not got.normal[k].any() and got.depth[k] == 0 and got.coverage[k] == 0
        else:
            assert np.array_equal(bits(got.albedo[k]), bits(table[obj[k]])) and got.coverage[k] == 1
            assert bits(got.depth[k]) == bits(dist[k])
            assert np.array_equal(bits(got.normal[k]), bits(np.zeros(3, f32) + R.normalize(g[k])))  # (a sum from 0: a -0 comes out +0)
        assert got.object[k] == obj[k]


def test_an_empty_scene_gives_zeros(oracle):
    cam = scenes.camera(oracle, 11, 9)
    for lens in (None, lens_of(cam)):
        got = F.features(oracle, cam, abi.SceneData(), abi.default_opts(seed=2), 3, lens)
        for a in got[:4]:
            assert a.dtype == f32 and not bits(a).any()
        assert got.object.dtype == np.int32 and (got.object == -1).all()
        assert got.albedo.shape == got.normal.shape == (9, 11, 3) and got.depth.shape == got.coverage.shape == got.object.shape == (9, 11)


def test_a_sphere_on_the_optical_axis(oracle):
    cam = scenes.camera(oracle, 101, 101)
    pos = np.array(scenes.CAMERA["position"], np.float64)
    axis = np.array(list(cam.img_center_point), np.float64) - pos
    axis /= np.linalg.norm(axis)
    sc = abi.SceneData(spheres=[(tuple(pos + 8.0 * axis), 2.0, abi.material(abi.MAT_LAMBERTIAN, (0.25, 0.5, 0.75)))])
    centre = [(50, 50)]
    opts = abi.default_opts(seed=4)
    one = F.features(oracle, cam, sc, opts, 1, pixels=centre)
    N = one.normal[50, 50].astype(np.float64)
    assert abs(np.linalg.norm(N) - 1.0) <= 2 * 2.0 ** -23
    d = F.primary_rays(cam, 4, 1, None, centre)[0, 0, 3:].astype(np.float64)
    assert N @ d < -0.99  # it faces the camera: not flipped, it simply does
    assert one.coverage[50, 50] == 1 and one.object[50, 50] == 0 and abs(one.depth[50, 50] - 6.0) < 1e-3
    five = F.features(oracle, cam, sc, opts, 5, pixels=centre)
    a, s = f32([0.25, 0.5, 0.75]), np.zeros(3, f32)
    for _ in range(5):
        s = s + a
    assert five.coverage[50, 50] == 1 and np.array_equal(bits(five.albedo[50, 50]), bits(s * (f32(1.0) / f32(5))))
    assert 0.999 < np.linalg.norm(five.normal[50, 50].astype(np.float64)) <= 1.0 + 2.0 ** -22  # a mean of unit vectors: not renormalised
    assert not one.coverage[0, 0] and one.object[0, 0] == -1  # (a pixel that was not asked for)
