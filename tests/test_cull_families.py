"""The culling pad on the GPU under the rays it is tightest for (tests/cull_families.py): Scene::hit through the host tree,
the device PLOC tree and the device LBVH tree must equal the brute-force scan bit for bit, and one small render per
geometry family through the megakernel (which shares make_cull / node4_visit but has its own leaf rounds) must equal the
oracle's image."""
import numpy as np
import pytest

import cull_families
import scenes
from rbrt_amd import abi
from test_bvh_host import build

pytestmark = pytest.mark.gpu

FAMILIES = ["far+1e+03", "far-3e+04", "far+1e+05", "slivers", "grid", "rough_spatial"]


@pytest.fixture(scope="module")
def fams(oracle):
    return cull_families.families(oracle)


def _set_env(monkeypatch, env, builder):
    monkeypatch.setenv("RBRT_HIP_LAB", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    if builder == "host":
        monkeypatch.setenv("RBRT_BVH_BUILDER", "host")
    else:
        monkeypatch.setenv("RBRT_BVH_BUILDER", "device")
        monkeypatch.setenv("RBRT_BVH_DEVICE_ALGO", builder)


@pytest.mark.parametrize("builder", ["host", "ploc", "lbvh"])
@pytest.mark.parametrize("family", FAMILIES)
def test_trace_rays_adversarial_equals_brute_force(hip, oracle, fams, monkeypatch, family, builder):
    md, env = fams[family]
    _set_env(monkeypatch, env, builder)
    N, T, _, _ = build(md)  # (the rays aim at the host tree's boxes: the device trees' boxes are near the same planes)
    rays = cull_families.rays(md, N, T, 60000, seed=7 + len(family))
    sc = abi.SceneData(meshes=[md])
    et, eo, ei, ed = oracle.trace_rays(sc, rays)
    with hip.HipScene(sc) as hs:
        gt, go, gi, gd = hs.trace_rays(rays)
    assert np.array_equal(eo, go) and np.array_equal(ei, gi)
    assert np.array_equal(et.view(np.uint32), gt.view(np.uint32))
    assert np.array_equal(ed.view(np.uint32), gd.view(np.uint32))
    assert (eo >= 0).sum() > 1000


@pytest.mark.parametrize("family", FAMILIES)
def test_render_of_each_family_equals_the_oracle(hip, oracle, fams, monkeypatch, family):
    md, env = fams[family]
    monkeypatch.setenv("RBRT_HIP_LAB", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = ((md.bbox_lo + md.bbox_hi) / 2).astype(np.float64)
    R = float(np.linalg.norm((md.bbox_hi - md.bbox_lo).astype(np.float64)) / 2)
    pos = tuple(float(x) for x in c + np.array([0.3, 0.8, 1.6]) * R * 1.2)
    cam = scenes.camera(oracle, 96, 64, position=pos, look_at=tuple(float(x) for x in c), up=(0.0, 1.0, 0.0))
    sc = abi.SceneData(spheres=[(tuple(float(x) for x in c - np.array([0.0, R * 3, 0.0])), R * 2.0,
                                 abi.material(abi.MAT_LAMBERTIAN, (0.4, 0.4, 0.4)))], meshes=[md])
    exp, exp8, _ = oracle.render(cam, sc, abi.default_opts(spp=3, seed=5))
    got, got8 = hip.render_scene(cam, 3, sc, seed=5)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and np.array_equal(got8, exp8)
    assert (exp != exp[0, 0]).any()  # not a blank frame
