"""The culling pad on the GPU under the rays it is tightest for (tests/cull_families.py): Scene::hit through the host tree,
the device PLOC tree and the device LBVH tree must equal the brute-force scan bit for bit, and one small render per
geometry family through the megakernel (which shares make_cull / node4_visit but has its own leaf rounds) must equal the
oracle's image. Both over the six families at the reference's default window and over cull_families.sweep(): the window
of mesh sizes, min_dist and direction lengths in which the reference's own test can accept a hit at all. The rendered
rows' tile-pass tables (whose tree boxes are grown by the same pad) are checked against the oracle's rays as well."""
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
    """name -> (MeshData, lab environment, min_dist, max_dist, direction lengths): the families at the reference's default
    window with rays()'s default lengths, and the rows of the sweep."""
    out = {k: (md, env, 0.001, 2000.0, (0.2, 1.0, 3.0)) for k, (md, env) in cull_families.families(oracle).items()}
    out.update(cull_families.sweep(oracle))
    return out


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
@pytest.mark.parametrize("family", FAMILIES + cull_families.SWEEP)
def test_trace_rays_adversarial_equals_brute_force(hip, oracle, fams, monkeypatch, family, builder):
    md, env, min_dist, max_dist, lengths = fams[family]
    _set_env(monkeypatch, env, builder)
    N, T, _, _ = build(md)  # (the rays aim at the host tree's boxes: the device trees' boxes are near the same planes)
    rays = cull_families.rays(md, N, T, 60000, seed=7 + len(family), eps=min_dist, lengths=lengths)
    sc = abi.SceneData(meshes=[md])
    et, eo, ei, ed = oracle.trace_rays(sc, rays, min_dist, max_dist)
    print(f"{family} x {builder}: {int((eo >= 0).sum())} scan hits of {len(rays)} rays")
    assert (eo >= 0).sum() > 1000  # (the oracle alone: a condition on the row)
    with hip.HipScene(sc) as hs:
        gt, go, gi, gd = hs.trace_rays(rays, min_dist, max_dist)
        # the tree under test is the named builder's: a device builder that declined the mesh would leave the host's
        assert hs.info()["n_meshes_device_built"] == (0 if builder == "host" else 1)
    lost = np.flatnonzero((eo >= 0) & (go < 0))
    assert np.array_equal(eo, go) and np.array_equal(ei, gi), (
        f"{len(lost)} hits lost, {int(np.count_nonzero((eo != go) | (ei != gi)))} rays differ; first rays {np.flatnonzero((eo != go) | (ei != gi))[:8].tolist()}")
    assert np.array_equal(et.view(np.uint32), gt.view(np.uint32))
    assert np.array_equal(ed.view(np.uint32), gd.view(np.uint32))


@pytest.mark.parametrize("family", FAMILIES)
def test_render_of_each_family_equals_the_oracle(hip, oracle, fams, monkeypatch, family):
    md, env = fams[family][:2]
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


# Rows of the sweep that only trace_rays reaches: a camera ray is a unit vector, and a frame has 96 x 64 x 3 of them.
#  * the short_long / long rows exist for their direction lengths; with unit directions "s1.5e-3_e1e-7_short_long" has
#    |a| ~ L^2 ~ 1e-10 < min_dist for every triangle (the oracle's frame has no pixel of the mesh), and the three others are
#    the mesh and window of another row;
#  * "slivers_e1e-6": triangles 1e-6 wide seen from 9 units away are missed by every camera ray of so small a frame (the
#    oracle's frame has no pixel of the mesh either); the rays of cull_families.rays are aimed at them;
#  * "s1.5e7_e1e-9": the reference itself cannot render a frame at that size. A ray scattered off a mesh leaves along the
#    UNNORMALISED triangle normal, about L^2 = 1e11 long there: next to a sphere, sphere.rs:22-33 squares b = 2 oc . d
#    into inf - inf = NaN, where it panics (the oracle counts 3400 such discriminants in this frame), and the frame of the
#    mesh alone holds NaN radiance in a thousand pixels.
TRACE_ONLY = {"s15_e1e-3_short_long", "s15_e1e-3_long", "s1.5e-3_e1e-7_short_long", "s1.5e7_e1e-9", "s1.5e7_e1e-9_short_long",
              "slivers_e1e-6"}
RENDERED = [r for r in cull_families.SWEEP if r not in TRACE_ONLY]


def sweep_view(oracle, md):
    """A 96x64 camera 1.2 bounding radii from the mesh, looking at it, and the mesh over a large diffuse sphere: both
    follow the row's size and place. Returns the camera, the scene, and the scene without the mesh."""
    c = ((md.bbox_lo + md.bbox_hi) / 2).astype(np.float64)
    R = cull_families.radius(md)
    off = np.array([0.3, 0.8, 1.6]) / np.linalg.norm([0.3, 0.8, 1.6]) * R * 1.2
    cam = scenes.camera(oracle, 96, 64, position=tuple(float(x) for x in c + off), look_at=tuple(float(x) for x in -off), up=(0.0, 1.0, 0.0))
    ground = [(tuple(float(x) for x in c - np.array([0.0, R * 3, 0.0])), R * 2.0, abi.material(abi.MAT_LAMBERTIAN, (0.4, 0.4, 0.4)))]
    return cam, abi.SceneData(spheres=ground, meshes=[md]), abi.SceneData(spheres=ground)


@pytest.mark.parametrize("row", RENDERED)
def test_render_of_each_sweep_row_equals_the_oracle(hip, oracle, fams, monkeypatch, row):
    """One small frame per row through the megakernel with the row's window in the options on both sides, and the tile
    pass's table for that camera and window against the oracle's rays (test_primary_cull.check_table). TRACE_ONLY above
    says which rows have no frame, and why."""
    import test_primary_cull as PC
    md, env, min_dist, max_dist, _ = fams[row]
    monkeypatch.setenv("RBRT_HIP_LAB", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cam, sc, without = sweep_view(oracle, md)
    opts = abi.default_opts(spp=3, seed=5, min_dist=min_dist, max_dist=max_dist)
    panics = oracle.lib().rbrt_oracle_nan_discriminants()
    exp, exp8, _ = oracle.render(cam, sc, opts)
    # (the oracle alone: a frame the reference renders at all, and without NaN)
    assert oracle.lib().rbrt_oracle_nan_discriminants() == panics and not np.isnan(exp).any()
    bare, _, _ = oracle.render(cam, without, opts)
    seen = int(np.count_nonzero((exp != bare).any(-1)))
    print(f"{row}: the mesh changes {seen} of {96 * 64} pixels")
    assert seen > 300 and (exp != exp[0, 0]).any()  # (the oracle alone: the mesh is in the frame, which is not blank)
    got, got8 = hip.render_scene(cam, 3, sc, seed=5, min_dist=min_dist, max_dist=max_dist)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)) and np.array_equal(got8, exp8)
    PC.check_table(hip, oracle, cam, sc, np.random.default_rng(len(row)), max_dist=max_dist, min_dist=min_dist)
