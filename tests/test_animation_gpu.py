"""Animation on the GPU (include/rbrt_hip.h "Animation"): the phase of a handle's motion, the motion buffer and the accumulation
that follows the spheres, each bit for bit against np_animation.py.

The phase: images for a pinhole and for lens, shutter and environment together, with a small mesh in front so that paths are
parked and resumed, at phases -3, 0.5, 7 and 40; a phase of 0 and no phase call against each other and np_motion; the phase
through the lab knobs' rows that shrink the grid, a helper launch, the short-path stage, render_pass and render_adaptive; the
handle's state and the refusals. The tile pass at those phases: no restated ray hits a sphere, where its own s puts it, in a
tile that culls it, the image with the table is the image without it, and the bound follows the sphere out of the view. The
motion buffer, the moving accumulation in every mode of the plain one's tests, and, end to end, the quality property of
test_np_animation.py on real renders and the command line's --motion-step."""
from __future__ import annotations

import ctypes as C
import functools
import json
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import full_scenes as F
import np_animation as NA
import np_env
import np_features
import np_motion as NM
import np_temporal as NT
import scenes
import temporal_cases as TC
import test_motion_gpu as MG
import test_np_animation as Q
import test_primary_cull as PC
from rbrt_amd import abi
from test_temporal_gpu import ppm, read_pfm

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
CFG = ROOT / "scenes" / "motion" / "animated_spheres.yaml"
f32 = np.float32
L_, M_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_EMISSIVE
PHASES = (-3.0, 0.5, 7.0, 40.0)
DEPTH = 8
bits, render = MG.bits, MG.render


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


# ---- the phase: images ----------------------------------------------------------------------------------------------------------------
IMG_W, IMG_H, IMG_SPP, IMG_SEED = 40, 24, 3, 7
# the ground stays; the matte sphere and the glass one each move their own way, slowly enough to be in view at phase 40 still
IMG_TRAVELS = np.array([(0.0, 0.0, 0.0), (0.05, 0.0, 0.0), (-0.02, 0.01, 0.03)], f32)
IMG_SHUTTER = (0.3, -0.2, 0.1)


def image_scene(oracle, mesh=True):
    sph = [scenes.EXAMPLE_SPHERES[0], scenes.EXAMPLE_SPHERES[1], scenes.EXAMPLE_SPHERES[3]]
    meshes = [scenes.standin_mesh(oracle, 13, 25.0, (0.5, -0.6, -4.5), (0.0, 0.4, 0.0), abi.material(M_, (0.8, 0.7, 0.6), 0.05))] if mesh else []
    return abi.SceneData(spheres=sph, meshes=meshes)


def image_setup(oracle, case):
    cam = scenes.camera(oracle, IMG_W, IMG_H)
    everything = case == "lens_shutter_environment"
    return SimpleNamespace(cam=cam, sc=image_scene(oracle), opts=abi.default_opts(spp=IMG_SPP, seed=IMG_SEED, max_depth=DEPTH),
                           lens=MG.lens_of(cam) if everything else None, shutter=IMG_SHUTTER if everything else None,
                           nodes=np_env.noise_map(8, 3) if everything else None)


@functools.lru_cache(maxsize=None)
def image_reference(case, phase):
    """The restated image of a case at a phase (None: np_motion's, which knows no phase), made once and left unchanged."""
    from oracle import pyoracle
    s = image_setup(pyoracle, case)
    if phase is None:
        exp = NM.restated_image(s.cam, s.sc, s.opts, IMG_TRAVELS, lens=s.lens, shutter=s.shutter, nodes=s.nodes)
    else:
        exp = NA.restated_image(s.cam, s.sc, s.opts, IMG_TRAVELS, phase, lens=s.lens, shutter=s.shutter, nodes=s.nodes)
    for a in exp:
        a.setflags(write=False)
    return exp


def configured(hip, s):
    hs = hip.HipScene(s.sc)
    if s.nodes is not None:
        hs.set_environment(s.nodes)
    hs.set_shutter(s.shutter)
    hs.set_motion(IMG_TRAVELS)
    return hs


@pytest.mark.parametrize("case", ["pinhole", "lens_shutter_environment"])
def test_images_at_a_phase_are_bit_identical_to_the_restatement(hip, oracle, case):
    """40 x 24 x 3, depth 8: three spheres of which two move, one small mesh; one handle through the four phases."""
    s = image_setup(oracle, case)
    seen = []
    with configured(hip, s) as hs:
        for phase in PHASES:
            exp, exp8 = image_reference(case, phase)
            hs.set_motion_phase(phase)
            got, got8 = render(hs, s.cam, s.opts, s.lens)
            hs.check()
            assert hs.last_trace_build() == "general"
            assert same(got, exp), (phase, np.argwhere(bits(got) != bits(exp))[:5])
            assert np.array_equal(got8, exp8), phase
            seen.append(exp)
    assert all(not same(a, b) for k, a in enumerate(seen) for b in seen[k + 1:])  # (every phase is another image)


@pytest.mark.parametrize("case", ["pinhole", "lens_shutter_environment"])
def test_a_phase_of_zero_is_no_phase_at_all(hip, oracle, case):
    """No phase call, a phase of 0, of -0 and of 0 again after another: one image, np_motion's, bit for bit."""
    s = image_setup(oracle, case)
    exp, exp8 = image_reference(case, None)
    assert same(image_reference(case, 0.0)[0], exp)
    with configured(hip, s) as hs:
        never, never8 = render(hs, s.cam, s.opts, s.lens)
        hs.set_motion_phase(0.0)
        zero, _ = render(hs, s.cam, s.opts, s.lens)
        hs.set_motion_phase(-0.0)
        minus, _ = render(hs, s.cam, s.opts, s.lens)
        hs.set_motion_phase(7.0)
        other, _ = render(hs, s.cam, s.opts, s.lens)
        hs.set_motion_phase(0.0)
        again, _ = render(hs, s.cam, s.opts, s.lens)
        hs.check()
    assert same(never, exp) and np.array_equal(never8, exp8)
    assert same(zero, exp) and same(minus, exp) and same(again, exp) and not same(other, exp)


# ---- the phase survives parking ---------------------------------------------------------------------------------------------------------
PARK_PHASE = 0.5


@functools.lru_cache(maxsize=None)
def parked_reference():
    """test_motion_gpu's scene with a small mesh in front, at PARK_PHASE: made once for every row below (and left unchanged)."""
    from oracle import pyoracle
    sc = MG.moving_scene(pyoracle, mesh=True)
    cam = scenes.camera(pyoracle, MG.PARK_W, MG.PARK_H)
    opts = abi.default_opts(spp=MG.PARK_SPP, seed=MG.PARK_SEED, max_depth=DEPTH)
    exp, _ = NA.restated_image(cam, sc, opts, MG.TRAVELS, PARK_PHASE)
    exp.setflags(write=False)
    return exp


@pytest.mark.parametrize("rid,env", MG.PARK_ROWS, ids=[r[0] for r in MG.PARK_ROWS])
def test_the_phase_survives_every_park_and_resume(hip, oracle, monkeypatch, rid, env):
    """test_motion_gpu's rows (one wave per CU, two shade rounds, forced helper launches) at a phase of 0.5: the word beside the
    path is s, not t. Two frames issued back to back, a render_pass series and render_adaptive with threshold 0: the one image."""
    import torch
    exp = parked_reference()
    assert not same(exp, MG.parked_reference())  # (the phase does something here)
    sc = MG.moving_scene(oracle, mesh=True)
    cam = scenes.camera(oracle, MG.PARK_W, MG.PARK_H)
    opts = abi.default_opts(spp=MG.PARK_SPP, seed=MG.PARK_SEED, max_depth=DEPTH)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    new = lambda: torch.full((MG.PARK_H, MG.PARK_W, 3), float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    with hip.HipScene(sc) as hs:
        hs.set_motion(MG.TRAVELS)
        hs.set_motion_phase(PARK_PHASE)
        hs.set_timing(True)
        outs = [new(), new()]
        for o in outs:
            hs.render_device(cam, opts, o.data_ptr())
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            assert same(o.cpu().numpy(), exp), (rid, k)
        acc, out = torch.zeros((MG.PARK_H, MG.PARK_W, 3), dtype=torch.float32, device="cuda"), new()
        for b, e in ((0, 1), (1, 5), (5, MG.PARK_SPP)):
            hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == MG.PARK_SPP else None)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), exp), (rid, "render_pass")
        out = new()
        res = hs.render_adaptive(cam, opts, 0.0, 2, 3, out.data_ptr())
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), exp) and res["rounds"] > 1, (rid, "render_adaptive", res)
        hs.check()


def test_the_short_path_stage_at_a_phase(hip, oracle):
    """No mesh anywhere: every tile that is not background only is the stage's. Stage off, forced, and numpy, at a phase of 7."""
    s = image_setup(oracle, "pinhole")
    s.sc = image_scene(oracle, mesh=False)
    exp, _ = NA.restated_image(s.cam, s.sc, s.opts, IMG_TRAVELS, 7.0)
    got = {}
    for mode in (0, 2):
        with hip.HipScene(s.sc) as hs:
            hs.set_motion(IMG_TRAVELS)
            hs.set_motion_phase(7.0)
            hs.set_short_paths(mode)
            got[mode], _ = render(hs, s.cam, s.opts)
            if mode == 2:
                assert hs.short_masks().any()  # (the stage finished samples of this launch)
            hs.check()
    assert same(got[0], got[2]) and same(got[2], exp)
    assert not same(exp, NM.restated_image(s.cam, s.sc, s.opts, IMG_TRAVELS)[0])


# ---- the phase: the handle's state --------------------------------------------------------------------------------------------------------
def test_the_phase_is_set_replaced_kept_and_cleared(hip, oracle):
    """Set, replace, survive set_motion (replace, clear and set again), clear; and a launch in flight keeps its phase: two renders
    issued with a phase change between them and no wait, each its own restatement."""
    import torch
    w, h = 20, 12
    cam = scenes.camera(oracle, w, h)
    sc = image_scene(oracle, mesh=False)
    opts = abi.default_opts(spp=4, seed=5, max_depth=DEPTH)
    other = (IMG_TRAVELS * f32(-2.0)).astype(f32)
    ref = lambda tv, ph: NA.restated_image(cam, sc, opts, tv, ph)[0]  # noqa: E731
    with hip.HipScene(sc) as hs:
        hs.set_motion_phase(3.0)  # before any motion: kept, without effect
        plain, _ = render(hs, cam, opts)
        assert same(plain, oracle.render(cam, sc, opts)[0])
        hs.set_motion(IMG_TRAVELS)
        assert same(render(hs, cam, opts)[0], ref(IMG_TRAVELS, 3.0)), "set before the motion"
        hs.set_motion_phase(-1.5)
        assert same(render(hs, cam, opts)[0], ref(IMG_TRAVELS, -1.5)), "replaced"
        hs.set_motion(other)
        assert same(render(hs, cam, opts)[0], ref(other, -1.5)), "survives a replaced motion"
        hs.set_motion(None)
        assert same(render(hs, cam, opts)[0], plain), "no motion, no effect"
        hs.set_motion(IMG_TRAVELS)
        assert same(render(hs, cam, opts)[0], ref(IMG_TRAVELS, -1.5)), "survives a cleared motion"
        hs.set_motion_phase(0.0)
        assert same(render(hs, cam, opts)[0], NM.restated_image(cam, sc, opts, IMG_TRAVELS)[0]), "cleared"
        # in flight
        a = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        b = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.set_motion_phase(7.0)
        hs.render_device(cam, opts, a.data_ptr())
        hs.set_motion_phase(40.0)
        hs.render_device(cam, opts, b.data_ptr())
        torch.cuda.synchronize()
        assert same(a.cpu().numpy(), ref(IMG_TRAVELS, 7.0)) and same(b.cpu().numpy(), ref(IMG_TRAVELS, 40.0))
        hs.check()


def test_phase_refusals_through_the_c_abi(hip, oracle):
    lib = abi.load_hip()
    assert lib.rbrt_hip_scene_set_motion_phase(None, C.c_float(0.0)) == abi.RBRT_ERR_INVALID_ARG
    cam = scenes.camera(oracle, 16, 8)
    sc = abi.SceneData(spheres=[((0.0, -1000.0, -5.0), 1000.0, abi.material(L_, (0.5, 0.5, 0.5))), ((0.0, 1.0, -8.0), 1.0, abi.material(M_, (0.8, 0.8, 0.8), 0.1))])
    opts = abi.default_opts(spp=1, seed=1)
    tv = np.array([(0.0, 0.0, 0.0), (0.5, 0.0, 0.0)], f32)

    def refused(word, call, *a, **kw):
        with pytest.raises(abi.RbrtError) as e:
            call(*a, **kw)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG and word in str(e.value), str(e.value)

    with hip.HipScene(sc) as hs:
        hs.set_motion(tv)
        hs.set_motion_phase(2.0)
        kept, _ = render(hs, cam, opts)
        for v in (float("nan"), float("inf"), -float("inf")):
            refused("not finite", hs.set_motion_phase, v)
        assert same(render(hs, cam, opts)[0], kept)  # (a refused call leaves the phase as it was)
        assert same(kept, NA.restated_image(cam, sc, opts, tv, 2.0)[0])
    far = abi.SceneData(spheres=[((0.0, 1.0, -8.0), 1.0, abi.material(L_, (0.5, 0.5, 0.5)))])
    with hip.HipScene(far) as hs:  # (never rendered)
        hs.set_motion([(1.0e30, 0.0, 0.0)])
        refused("(phase + 1) * travel", hs.set_motion_phase, 1.0e9)   # 1e39 is not a float32
        hs.set_motion_phase(1.0e8)                                     # 1e38 is
        refused("(phase + 1) * travel", hs.set_motion, [(1.0e31, 0.0, 0.0)])  # set_motion checks against the handle's phase
        hs.set_motion([(-1.0e30, 0.0, 0.0)])
        hs.set_motion(None)
        hs.set_motion_phase(1.0e30)  # without a motion any finite phase is accepted ...
        refused("(phase + 1) * travel", hs.set_motion, [(1.0e30, 0.0, 0.0)])  # ... and the next motion answers for it


# ---- the tile pass ---------------------------------------------------------------------------------------------------------------------
def check_phase_table(hip, monkeypatch, cam, sc, travels, phase, shutter=None, n=3, seed=3):
    """test_motion_gpu.check_motion_table's property at a phase: no ray of np_animation.primary_rays hits sphere e, where its own
    s puts it, in a tile whose word has bit e; and the image with the table is the image without it. Returns the table."""
    travels = NM.travels_of(travels)
    opts = abi.default_opts(spp=n, seed=seed, max_depth=DEPTH)
    rays, ss = NA.primary_rays(cam, seed, n, phase, shutter=shutter)
    flat, sf = rays.reshape(-1, 6), ss.reshape(-1)
    images = {}
    for cull in ("1", "0"):
        monkeypatch.setenv("RBRT_PRIMARY_CULL", cull)
        with hip.HipScene(sc) as hs:
            hs.set_shutter(shutter)
            hs.set_motion(travels)
            hs.set_motion_phase(phase)
            if cull == "1":
                table = hs.primary_cull(cam)
            try:
                images[cull], _ = render(hs, cam, opts)
                hs.check()
            except abi.RbrtError as e:  # (a NaN discriminant, sphere.rs:33: both renders meet it)
                assert e.code == abi.RBRT_ERR_NAN
                images[cull] = None
    assert (images["1"] is None) == (images["0"] is None)
    if images["1"] is not None:
        assert F.same_bits(images["1"], images["0"])
    pix = np_features.all_pixels(cam)
    tile_of = np.repeat(np.array([(r // 8) * table.shape[1] + (c // 8) for r, c in pix]), n)
    words = table.reshape(-1)[tile_of]
    for e, (c, r, _) in enumerate(sc.spheres[:24]):
        centres = (np.asarray(c, f32)[None, :] + (sf[:, None] * travels[e][None, :]).astype(f32)).astype(f32)
        bad = MG.sphere_hits(flat, centres, r, opts.min_dist, opts.max_dist) & (((words >> e) & 1) != 0)
        assert not bad.any(), f"sphere {e}: culled in tiles {sorted(set(tile_of[bad].tolist()))[:5]} where a ray of the restatement hits it"
    return table


@pytest.mark.parametrize("name,centre,travel", MG.HAND_PICKED, ids=[c[0] for c in MG.HAND_PICKED])
def test_no_ray_hits_a_sphere_its_tile_culled_at_phase_7(hip, oracle, monkeypatch, name, centre, travel):
    """test_motion_gpu's hand-picked pairs, seven exposures later (the opening centre moved back so that the sweep is in view)."""
    cam = MG.axis_camera(oracle)
    back = tuple(float(f32(c) - f32(7.0) * f32(t)) for c, t in zip(centre, travel))
    sc = MG.pair((3.0, 0.0, -10.0), back)
    table = check_phase_table(hip, monkeypatch, cam, sc, [(0.0, 0.0, 0.0), travel], 7.0)
    s_bit, m_bit = (table & 1) != 0, (table & 2) != 0
    print(f"{name}: static culled in {int(s_bit.sum())}, moving culled in {int(m_bit.sum())} of {table.size} tiles")
    assert s_bit.any() and not s_bit.all()
    if name in ("sweeps_in_from_outside", "past_the_camera", "longer_than_the_distance"):
        assert not m_bit.all()  # (seen somewhere)
    if name == "sweeps_in_from_outside":
        assert m_bit[:, table.shape[1] // 2:].all()  # (it ends at x = -3: the right half never sees it)


@pytest.mark.parametrize("k", range(12))
def test_fuzzed_cameras_travels_and_phases(hip, oracle, monkeypatch, k):
    """The random scenes and cameras of test_primary_cull, test_motion_gpu's travels, and a phase log-uniform from 1e-3 to 100,
    either sign; the four named phases take the first rows."""
    rng = np.random.default_rng(93000 + k)
    sc = PC.fuzz_scene(oracle, rng)
    w, h = int(rng.integers(9, 49)), int(rng.integers(9, 33))
    cam = PC.fuzz_camera(oracle, rng, sc, w, h)
    travels = np.array([PC._log_uniform(rng, 1e-4, 100.0) * PC._unit(rng) * (rng.random() >= 0.25) for _ in sc.spheres], f32).reshape(-1, 3)
    shutter = tuple(float(f32(v)) for v in PC._log_uniform(rng, 1e-3, 10.0) * PC._unit(rng)) if k % 3 == 0 else None
    phase = PHASES[k] if k < len(PHASES) else float(f32(PC._log_uniform(rng, 1e-3, 100.0) * (1 if rng.random() < 0.5 else -1)))
    table = check_phase_table(hip, monkeypatch, cam, sc, travels, phase, shutter=shutter, n=2, seed=k)
    print(f"fuzz {k}: {w}x{h}, {len(sc.spheres)} spheres, {len(sc.meshes)} meshes, phase {phase:.4g}: {int(np.count_nonzero(table))} tiles with bits")


def test_the_bound_follows_the_sphere(hip, oracle):
    """A lone sphere of radius 0.5 in the middle of the view, 10 units ahead, moving 0.25 units an exposure to the right. The view
    is 3.5 units to either side there: at phases 40 and -40 the advanced centre is 13 radii outside it and every tile culls the
    sphere; a margin of (|phase| + 1) |travel| around the opening centre would have culled it nowhere. At phase 0 the middle
    tiles see it; at phase 12 it stands on the view's right edge (x = 3 to 3.25 during the exposure): the tiles there keep it."""
    cam = MG.axis_camera(oracle)
    sc = abi.SceneData(spheres=[((0.0, 0.0, -10.0), 0.5, abi.material(L_, (0.7, 0.4, 0.3)))])
    opts = abi.default_opts(spp=2, seed=3)
    with hip.HipScene(sc) as hs:
        hs.set_motion([(0.25, 0.0, 0.0)])
        at0 = (hs.primary_cull(cam) & 1) != 0
        assert not at0.all() and at0.any() and not at0[at0.shape[0] // 2, at0.shape[1] // 2]
        for phase in (40.0, -40.0):
            hs.set_motion_phase(phase)
            assert ((hs.primary_cull(cam) & 1) != 0).all(), phase
            got, _ = render(hs, cam, opts)
            assert same(got, oracle.render(cam, abi.SceneData(spheres=[((1.0e6, 0.0, 0.0), 0.5, sc.spheres[0][2])]), opts)[0]), phase  # (sky only)
        hs.set_motion_phase(12.0)
        near = (hs.primary_cull(cam) & 1) != 0
        assert not near.all() and near[:, : near.shape[1] // 2].all()  # (the right edge's tiles keep it, the left half never does)
        hs.check()


def test_the_table_key_covers_the_phase(hip, oracle):
    """Two renders on one handle, one camera, at different phases, the second after the first's table exists: each its own
    restatement, and back again."""
    cam = MG.axis_camera(oracle, 32, 24)
    sc = MG.pair((3.0, 0.0, -10.0), (-3.0, 0.0, -10.0))
    tv = [(0.0, 0.0, 0.0), (0.25, 0.0, 0.0)]
    opts = abi.default_opts(spp=3, seed=3, max_depth=DEPTH)
    exp = {ph: NA.restated_image(cam, sc, opts, tv, ph)[0] for ph in (0.0, 20.0)}
    assert not same(exp[0.0], exp[20.0])
    with hip.HipScene(sc) as hs:
        hs.set_motion(tv)
        for ph in (0.0, 20.0, 0.0, 20.0):
            hs.set_motion_phase(ph)
            assert same(render(hs, cam, opts)[0], exp[ph]), ph
        hs.check()


# ---- the motion buffer --------------------------------------------------------------------------------------------------------------------
def feature_buffers(torch, w, h):
    return dict(albedo=torch.full((h, w, 3), float("nan"), device="cuda"), normal=torch.full((h, w, 3), float("nan"), device="cuda"),
                depth=torch.full((h, w), float("nan"), device="cuda"), coverage=torch.full((h, w), float("nan"), device="cuda"),
                object=torch.full((h, w), -7, dtype=torch.int32, device="cuda"), motion=torch.full((h, w, 3), float("nan"), device="cuda"))


def check_motion_buffer(hip, oracle, w, h, n, travels, phase=0.0, lens=False, shutter=None):
    """Every kind of object under the rays: test_motion_gpu's spheres with a BasicTriangle between them and a small mesh in front.
    The six buffers against np_animation.features; the five against rbrt_hip_render_features' on the same handle; d_motion alone."""
    import torch
    cam = scenes.camera(oracle, w, h)
    sc = MG.moving_scene(oracle, triangle=True, mesh=True)
    opts = abi.default_opts(spp=2, seed=5)
    ln = MG.lens_of(cam) if lens else None
    exp, exp_mv = NA.features(cam, sc, opts, n, travels, phase, lens=ln, shutter=shutter)
    bufs, old, alone = feature_buffers(torch, w, h), feature_buffers(torch, w, h), torch.full((h, w, 3), float("nan"), device="cuda")
    with hip.HipScene(sc) as hs:
        hs.set_shutter(shutter)
        hs.set_motion(travels)
        hs.set_motion_phase(phase)
        hs.render_features(cam, opts, n, lens=ln, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        hs.render_features(cam, opts, n, lens=ln, **{f"d_{k}": v.data_ptr() for k, v in old.items() if k != "motion"})
        hs.render_features(cam, opts, n, lens=ln, d_motion=alone.data_ptr())
        torch.cuda.synchronize()
        hs.check()
    for k in ("albedo", "normal", "depth", "coverage"):
        assert same(bufs[k].cpu().numpy(), getattr(exp, k)), k
        assert same(old[k].cpu().numpy(), getattr(exp, k)), ("rbrt_hip_render_features", k)
    assert np.array_equal(bufs["object"].cpu().numpy(), exp.object) and np.array_equal(old["object"].cpu().numpy(), exp.object)
    assert torch.isnan(old["motion"]).all()  # (the old entry point knows no such buffer)
    assert same(bufs["motion"].cpu().numpy(), exp_mv) and same(alone.cpu().numpy(), exp_mv)
    return exp, exp_mv


@pytest.mark.parametrize("w,h", [(1, 1), (8, 8), (17, 9)], ids=["one_lane", "one_tile", "ragged_17x9"])
def test_the_motion_buffer_from_one_lane_to_ragged_tiles(hip, oracle, w, h):
    exp, mv = check_motion_buffer(hip, oracle, w, h, 3, MG.TRAVELS)
    if (w, h) == (17, 9):  # every kind of object under some ray: a moving sphere, the ground that stays, the triangle, the mesh, the sky
        ids = set(np.unique(exp.object).tolist())
        order = MG.moving_scene(oracle, triangle=True, mesh=True).element_order
        assert -1 in ids and len(order) in ids and order.index(scenes.T | 0) in ids and 0 in ids, ids
        assert mv.any() and not mv[exp.coverage == 0].any()


@pytest.mark.parametrize("lens,shutter,phase", [(False, MG.SKEW, 0.0), (True, None, 0.5), (True, MG.SKEW, -3.0)], ids=["shutter", "lens_phase", "lens_shutter_phase"])
def test_the_motion_buffer_with_shutter_lens_and_phase(hip, oracle, lens, shutter, phase):
    check_motion_buffer(hip, oracle, 17, 9, 3, MG.TRAVELS, phase=phase, lens=lens, shutter=shutter)


def test_the_motion_buffer_is_exact_and_zero_without_a_motion(hip, oracle):
    """A handle without a motion: all +0 whatever is hit, and the other five what they are. A travel of few mantissa bits, n = 4:
    a pixel every sample of which hits that sphere holds the travel itself, at any phase."""
    import torch
    w, h, n = 17, 9, 4
    cam = scenes.camera(oracle, w, h)
    sc = MG.moving_scene(oracle, triangle=True, mesh=True)
    opts = abi.default_opts(spp=2, seed=5)
    exp, exp_mv = NA.features(cam, sc, opts, n, None)
    assert not bits(exp_mv).any()
    bufs = feature_buffers(torch, w, h)
    with hip.HipScene(sc) as hs:
        hs.set_motion_phase(7.0)  # (no motion: no effect)
        hs.render_features(cam, opts, n, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        assert not bits(bufs["motion"].cpu().numpy()).any()  # +0, sign bit included
        for k in ("albedo", "normal", "depth", "coverage"):
            assert same(bufs[k].cpu().numpy(), getattr(exp, k)), k
        hs.check()
    travel = (0.25, -0.5, 0.125)
    one = abi.SceneData(spheres=[((0.0, 1.0, -7.0), 3.0, abi.material(L_, (0.5, 0.5, 0.5)))])
    mv, cov = torch.full((h, w, 3), float("nan"), device="cuda"), torch.full((h, w), float("nan"), device="cuda")
    with hip.HipScene(one) as hs:
        hs.set_motion([travel])
        hs.set_motion_phase(0.5)
        hs.render_features(cam, opts, n, d_coverage=cov.data_ptr(), d_motion=mv.data_ptr())
        torch.cuda.synchronize()
    mv, cov = mv.cpu().numpy(), cov.cpu().numpy()
    inside = cov == 1
    assert inside.sum() >= 10 and (cov == 0).any()
    assert same(mv[inside], np.broadcast_to(np.array(travel, f32), mv[inside].shape)) and not bits(mv[cov == 0]).any()


# ---- the moving accumulation ---------------------------------------------------------------------------------------------------------------
def up(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def run_moving(hip, torch, c, Mv, step, hist_packed, p=None, want=("hist", "a", "b", "len"), in_place=False, hist_out=None, cam_prev="case", old_call=False):
    """test_temporal_gpu.run_temporal with the motion buffer and the step: one call into buffers full of sentinels. Mv None: a
    NULL d_motion through the moving call -- or, with old_call, rbrt_hip_temporal_accumulate itself."""
    h, w = c.z.shape
    dev = SimpleNamespace(**{k: up(torch, getattr(c, k)) for k in ("A", "B", "N", "z", "c")})
    mv = up(torch, Mv) if Mv is not None else None
    hin = None if hist_packed is None else hist_packed if torch.is_tensor(hist_packed) else up(torch, hist_packed)
    n_hist = hip.temporal_history_bytes(w, h)
    hout = hist_out if hist_out is not None else torch.full((n_hist,), 0xAB, dtype=torch.uint8, device="cuda")
    assert hout.data_ptr() % 16 == 0 and (hin is None or hin.data_ptr() % 16 == 0)
    oa = dev.A if in_place else torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    ob = dev.B if in_place else torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    ol = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
    prev = (c.cam_prev if hin is not None else None) if isinstance(cam_prev, str) else cam_prev
    extra = {} if old_call else dict(d_motion=mv.data_ptr() if mv is not None else 0, phase_step=step)
    hip.temporal_accumulate(0, dev.A.data_ptr(), dev.B.data_ptr(), dev.N.data_ptr(), dev.z.data_ptr(), dev.c.data_ptr(), c.cam, prev,
                            hin.data_ptr() if hin is not None else None, hout.data_ptr() if "hist" in want else None,
                            oa.data_ptr() if "a" in want else None, ob.data_ptr() if "b" in want else None,
                            ol.data_ptr() if "len" in want else None, hip.temporal_opts(**(p or {})), **extra)
    torch.cuda.synchronize()
    return SimpleNamespace(a=oa.cpu().numpy(), b=ob.cpu().numpy(), len=ol.cpu().numpy(),
                           hist=hout.cpu().numpy()[:n_hist].view(f32).reshape(3, h, w, 4), hist_t=hout)


@functools.lru_cache(maxsize=None)
def moving_expected(pair, w, h, step):
    c, Mv = Q.moving_case(pair, w, h)
    oa, ob, ln, nxt, info = NA.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, Mv=Mv, phase_step=step, **NT.DEFAULTS)
    packed = NT.pack(nxt)
    for a in (oa, ob, ln, packed):
        a.flags.writeable = False
    return oa, ob, ln, packed, info


SIZES = [(1, 1), (16, 16), (17, 15), (257, 1), (33, 31)]  # around the 256-thread workgroup: one thread, one full, ragged, one over, four and a part


@pytest.mark.parametrize("pair", ["static", "drift_0.2"])
@pytest.mark.parametrize("step", [0.0, 1.0, -2.5])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_the_moving_accumulation_is_bit_identical(hip, w, h, step, pair):
    import torch
    c, Mv = Q.moving_case(pair, w, h)
    ea, eb, el, eh, _ = moving_expected(pair, w, h, step)
    g = run_moving(hip, torch, c, Mv, step, NT.pack(c.hist))
    assert same(g.a, ea) and same(g.b, eb) and same(g.len, el), (int((bits(g.a) != bits(ea)).sum()), int((bits(g.len) != bits(el)).sum()))
    assert same(g.hist, eh)


def test_the_motion_matters_and_a_null_buffer_is_the_old_call(hip):
    import torch
    pair, w, h = "drift_0.2", 33, 31
    c, Mv = Q.moving_case(pair, w, h)
    packed = NT.pack(c.hist)
    ea, eb, el, eh, _ = moving_expected(pair, w, h, 1.0)
    pa, pb, pl, ph, _ = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, **NT.DEFAULTS)
    assert not same(el, pl)  # (the inputs exercise the insertion)
    old = run_moving(hip, torch, c, None, 0.0, packed, old_call=True)
    for step in (1.0, float("nan"), float("inf")):  # (d_motion NULL: phase_step is not read)
        g = run_moving(hip, torch, c, None, step, packed)
        for k in ("a", "b", "len", "hist"):
            assert same(getattr(g, k), getattr(old, k)), (step, k)
    assert same(old.a, pa) and same(old.b, pb) and same(old.len, pl) and same(old.hist, NT.pack(ph))
    # a history written by one call, read by the other: the layout is one
    moved = run_moving(hip, torch, c, Mv, 1.0, packed)
    assert same(moved.hist, eh)
    nxt = SimpleNamespace(A=c.B, B=c.A, N=c.N, z=c.z, c=c.c, cam=c.cam, cam_prev=c.cam_prev)
    h_m = NT.History(ea, eb, el, c.N, c.z, c.c)
    g = run_moving(hip, torch, nxt, None, 0.0, moved.hist_t.view(torch.float32), old_call=True)
    xa, xb, xl, _, _ = NT.accumulate(nxt.A, nxt.B, nxt.N, nxt.z, nxt.c, nxt.cam, nxt.cam_prev, h_m, **NT.DEFAULTS)
    assert same(g.a, xa) and same(g.b, xb) and same(g.len, xl)
    g = run_moving(hip, torch, nxt, Mv, -2.5, old.hist_t.view(torch.float32))
    xa, xb, xl, _, _ = NA.accumulate(nxt.A, nxt.B, nxt.N, nxt.z, nxt.c, nxt.cam, nxt.cam_prev, NT.History(pa, pb, pl, c.N, c.z, c.c), Mv=Mv, phase_step=-2.5, **NT.DEFAULTS)
    assert same(g.a, xa) and same(g.b, xb) and same(g.len, xl)


def test_each_output_alone_in_place_and_the_first_frame(hip):
    import torch
    pair, w, h, step = "drift_0.2", 33, 31, 1.0
    c, Mv = Q.moving_case(pair, w, h)
    ea, eb, el, eh, _ = moving_expected(pair, w, h, step)
    packed = NT.pack(c.hist)
    untouched = dict(a=lambda g: np.isnan(g.a).all(), b=lambda g: np.isnan(g.b).all(), len=lambda g: (g.len == -7).all(),
                     hist=lambda g: (g.hist_t == 0xAB).all())
    exp = dict(a=ea, b=eb, len=el, hist=eh)
    for only in ("a", "b", "len", "hist"):
        g = run_moving(hip, torch, c, Mv, step, packed, want=(only,))
        assert same(getattr(g, only), exp[only]), only
        assert all(check(g) for name, check in untouched.items() if name != only), only
    g = run_moving(hip, torch, c, Mv, step, packed, want=())
    assert all(check(g) for check in untouched.values())
    g = run_moving(hip, torch, c, Mv, step, packed, in_place=True)
    assert same(g.a, ea) and same(g.b, eb) and same(g.len, el) and same(g.hist, eh)
    g = run_moving(hip, torch, c, Mv, step, None)  # the first frame: the identity, with a motion buffer as without
    assert same(g.a, c.A) and same(g.b, c.B) and (g.len == 1).all()


@pytest.mark.parametrize("w,h", [(33, 31), (257, 3)])
def test_a_chain_of_four_frames_alternates_two_dirty_histories(hip, w, h):
    """The analytic scene's features under a camera that drifts, with a motion buffer of its own every frame and another step:
    frame 0 has no history, frames 1 to 3 read what the frame before wrote through the packed history on the device alone. The
    two histories start dirty and the second round reuses them as the first left them."""
    import torch
    cams = [TC.camera(w, h, **TC.PAIRS["drift_0.2"]), TC.camera(w, h, **TC.PAIRS["drift_0.002"]), TC.camera(w, h), TC.camera(w, h)]
    steps = (0.0, 1.0, -2.5, 0.5)
    rng = np.random.default_rng(w * 100 + h)
    frames = []
    for k, cam in enumerate(cams):
        N, z, c = TC.features(cam)
        t = TC.truth(N, c)
        Mv = (c[..., None] * rng.uniform(-0.3, 0.3, (h, w, 3))).astype(f32)
        frames.append(SimpleNamespace(A=TC.noisy(t, rng), B=TC.noisy(t, rng), N=N, z=z, c=c, cam=cam, cam_prev=cams[k - 1] if k else None, Mv=Mv))
    hist, exp = None, []
    for fr, step in zip(frames, steps):
        oa, ob, ln, hist, info = NA.accumulate(fr.A, fr.B, fr.N, fr.z, fr.c, fr.cam, fr.cam_prev, hist, Mv=fr.Mv, phase_step=step, **NT.DEFAULTS)
        exp.append((oa, ob, ln, NT.pack(hist)))
    assert exp[3][2].max() > 3  # the fourth frame has histories of length 4
    n_hist = hip.temporal_history_bytes(w, h)
    two = [torch.full((n_hist,), v, dtype=torch.uint8, device="cuda") for v in (0xAB, 0x7F)]
    for round_ in range(2):
        hin = None
        for k, (fr, step) in enumerate(zip(frames, steps)):
            g = run_moving(hip, torch, fr, fr.Mv, step, hin, hist_out=two[k & 1])
            hin = two[k & 1].view(torch.float32)
            oa, ob, ln, packed = exp[k]
            assert same(g.a, oa) and same(g.b, ob) and same(g.len, ln) and same(g.hist, packed), (round_, k)


def test_non_finite_motion_stays_in_its_own_pixel(hip):
    """A NaN and infinities of either sign planted in d_motion: the motion of a pixel moves that pixel's own lookup and nothing
    else, so every other pixel holds the bits of the run without them; and a buffer that is nothing but NaN or infinities, with
    steps that overflow: every pixel passes through or holds something, no read leaves the buffers, no fault."""
    import torch
    pair, w, h, step = "drift_0.2", 33, 31, 1.0
    c, Mv = Q.moving_case(pair, w, h)
    ea, eb, el, eh, _ = moving_expected(pair, w, h, step)
    nan, inf = f32(np.nan), f32(np.inf)
    planted, reached = Mv.copy(), np.zeros((h, w), bool)
    for (y, x, k), v in {(0, 0, 0): nan, (5, 7, 1): inf, (20, 30, 2): -inf, (30, 32, 0): nan, (15, 15, 1): f32(3.0e38), (16, 15, 0): f32(-3.0e38),
                         (30, 0, 2): inf, (0, 32, 0): -inf}.items():
        planted[y, x, k] = v
        reached[y, x] = True
    packed = NT.pack(c.hist)
    g = run_moving(hip, torch, c, planted, step, packed)
    keep = ~reached
    assert same(g.a[keep], ea[keep]) and same(g.b[keep], eb[keep]) and same(g.len[keep], el[keep]) and same(g.hist[:, keep], eh[:, keep])
    assert (g.len[reached] >= 1).all()  # (a length all the same: 1 without a valid history)
    for v, s in ((nan, 1.0), (inf, 1.0), (-inf, -2.5), (f32(3.0e38), 3.0e38), (f32(1.0), 3.0e38)):
        g = run_moving(hip, torch, c, np.full((h, w, 3), v, f32), s, packed)
        assert (g.len != -7).all() and (g.len >= 1).all()


def test_the_moving_calls_refusals_write_nothing(hip):
    import torch
    c, Mv = Q.moving_case("turn", 37, 21)
    packed = up(torch, NT.pack(c.hist))
    g = None
    rows = [dict(p=dict(max_history=0.5)), dict(p=dict(depth=-1.0)), dict(p=dict(normal=float("nan"))), dict(p=dict(flags=1)), dict(p=dict(reserved=(0, 0, 0, 1))),
            dict(cam_prev=None), dict(cam_prev=TC.camera(36, 21)), dict(hist_out=packed.view(torch.uint8))]
    for kw in rows:  # everything the plain call refuses, with a motion buffer and with a NULL one
        for mv in (Mv, None):
            with pytest.raises(abi.RbrtError) as e:
                g = run_moving(hip, torch, c, mv, 1.0, packed, **kw)
            assert e.value.code == abi.RBRT_ERR_INVALID_ARG, kw
    for step in (float("nan"), float("inf"), -float("inf")):
        with pytest.raises(abi.RbrtError) as e:
            g = run_moving(hip, torch, c, Mv, step, packed)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG and "phase_step" in str(e.value)
    assert g is None and same(packed.cpu().numpy(), NT.pack(c.hist))
    lib = abi.load_hip()
    assert lib.rbrt_hip_temporal_accumulate_moving(0, None, None, None, None, None, None, None, C.c_float(0.0), C.byref(c.cam), None,
                                                   C.byref(hip.temporal_opts()), None, None, None, None, None) == abi.RBRT_ERR_INVALID_ARG


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_the_history_follows_a_moving_sphere_on_real_renders(hip, oracle):
    """test_np_animation's quality property through one handle: six frames of render_adaptive's halves, render_features with the
    motion buffer and the moving accumulation at a step of two exposures; the lengths the device wrote are judged, and the plain
    rule runs beside them on the same features. The device's feature buffers are the restatement's, so the count is its 120."""
    import torch
    w, h, n = Q.Q_W, Q.Q_H, Q.Q_SAMPLES
    cam = scenes.camera(oracle, w, h)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")  # noqa: E731
    two = [torch.full((hip.temporal_history_bytes(w, h),), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    two_plain = [torch.full((hip.temporal_history_bytes(w, h),), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    frames, lengths, plain = [], [], []
    with hip.HipScene(Q.quality_scene()) as hs:
        hs.set_motion([Q.Q_TRAVEL])
        for k in range(Q.Q_FRAMES):
            o = Q.quality_opts(k, spp=4)
            hs.set_motion_phase(float(f32(k) * f32(Q.Q_STEP)))
            rad, ha, hb, nor, dep, cov, mv, ol, pl = new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w), new(h, w), new(h, w, 3), new(h, w), new(h, w)
            assert hs.render_adaptive(cam, o, 0.0, 4, 4, rad.data_ptr())["rounds"] == 1
            hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
            hs.render_features(cam, o, n, None, nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), d_motion=mv.data_ptr())
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, cam if k else None,
                                    two_plain[(k - 1) & 1].data_ptr() if k else None, two_plain[k & 1].data_ptr(), None, None, pl.data_ptr())
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, cam if k else None,
                                    two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr(),
                                    d_motion=mv.data_ptr(), phase_step=Q.Q_STEP)
            torch.cuda.synchronize()
            assert torch.isfinite(ha).all() and torch.isfinite(hb).all()
            frames.append(tuple(t.cpu().numpy() for t in (nor, dep, cov, mv)))
            lengths.append(ol.cpu().numpy()), plain.append(pl.cpu().numpy())
        hs.check()
    for got, exp in zip(frames, Q.quality_frames()):  # (what the restatement has shown to satisfy the property)
        assert all(same(a, b) for a, b in zip(got, exp))
    # the restatement, fed the device's features, gives the device's lengths; and they satisfy the property
    hist = None
    cov_last = None
    for k, (N, z, c, Mv) in enumerate(frames):
        zeros = np.zeros((h, w, 3), f32)
        _, _, el, hist, info = NA.accumulate(zeros, zeros, N, z, c, cam, cam, hist, Mv=Mv, phase_step=Q.Q_STEP)
        assert same(lengths[k], el), k
        if k:
            el_mask = Q.eligible(c, cov_last, info)
            off = np.abs(lengths[k][el_mask].astype(np.float64) - (k + 1))
            assert el_mask.any() and (off <= Q.length_tolerance(k)).all(), (k, float(off.max()))
            assert (plain[k][el_mask] < (k + 1) - Q.length_tolerance(k)).any(), k
            print(f"frame {k}: {int(el_mask.sum())} eligible pixels of length {k + 1}; {int((plain[k][el_mask] < (k + 1) - Q.length_tolerance(k)).sum())} shorter under the plain rule")
        cov_last = c
    assert int(el_mask.sum()) >= Q.Q_MIN_PIXELS


W, H, N_SPP, FS, FRAMES, SEED = 64, 48, 4, 3, 3, 3


def run_cli(tmp_path, name, *args):
    out = tmp_path / f"{name}.ppm"
    files = dict(out=out, pfm=tmp_path / f"{name}.pfm", hmap=tmp_path / f"{name}.h.ppm", rep=tmp_path / f"{name}.json", feat=tmp_path / f"{name}.f")
    r = subprocess.run([str(EXE), "-c", str(CFG), "--height", str(H), "-w", str(W), "-s", str(N_SPP), "--seed", str(SEED), "--feature-samples", str(FS),
                        "--frames", str(FRAMES), "--radiance", str(files["pfm"]), "--history-map", str(files["hmap"]), "--report", str(files["rep"]),
                        "--features", str(files["feat"]), "-t", str(out), *args], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return SimpleNamespace(**files)


def library_frames(hip, torch, hsn, step, factor, moving):
    """The library calls of the command line's frame loop from here, with the accumulation of every frame checked against
    np_animation.accumulate fed the device's halves and features. -> the filtered radiance, its 8-bit image, the last length, the
    last frame's features and motion buffer."""
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")  # noqa: E731
    ha, hb, alb, nor, dep, cov, mv, ol, rad = new(H, W, 3), new(H, W, 3), new(H, W, 3), new(H, W, 3), new(H, W), new(H, W), new(H, W, 3), new(H, W), new(H, W, 3)
    rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
    two = [torch.zeros((hip.temporal_history_bytes(W, H),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    cam = hsn.camera
    traced = hip.upsample_camera(cam, factor) if factor > 1 else cam
    w, h = traced.img_width_pix, traced.img_height_pix
    la, lb = new(h, w, 3), new(h, w, 3)
    hist = None
    with hip.HipScene(hsn) as hs:
        hs.set_motion(hsn.motion)
        for k in range(FRAMES):
            if moving:
                hs.set_motion_phase(float(f32(k) * f32(step)))
            o = abi.default_opts(spp=N_SPP, seed=SEED + k)
            assert hs.render_adaptive(traced, o, 0.0, N_SPP, N_SPP)["rounds"] == 1
            hs.denoise(None, None, (la if factor > 1 else ha).data_ptr(), (lb if factor > 1 else hb).data_ptr())
            hs.render_features(cam, o, FS, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), d_motion=mv.data_ptr())
            if factor > 1:
                ws = torch.zeros((hip.upsample_workspace_bytes(W, H, factor),), dtype=torch.uint8, device="cuda")
                hip.upsample_halves(0, la.data_ptr(), lb.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H, ws.data_ptr(),
                                    ha.data_ptr(), hb.data_ptr(), None, hip.upsample_opts(factor=factor))
            torch.cuda.synchronize()
            A, B, N, z, c, Mv = (t.cpu().numpy() for t in (ha, hb, nor, dep, cov, mv))
            extra = dict(d_motion=mv.data_ptr(), phase_step=step) if moving else {}
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, cam if k else None,
                                    two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr(), **extra)
            torch.cuda.synchronize()
            ea, eb, el, hist, _ = NA.accumulate(A, B, N, z, c, cam, cam, hist, Mv=Mv if moving else None, phase_step=step, **NT.DEFAULTS)
            assert same(ha.cpu().numpy(), ea) and same(hb.cpu().numpy(), eb) and same(ol.cpu().numpy(), el), k
        hs.check()
    wa = torch.full((H, W), float(f32((N_SPP + 1) // 2) * (f32(1) / f32(N_SPP))), dtype=torch.float32, device="cuda")
    gws = torch.zeros((hip.guided_workspace_bytes(W, H),), dtype=torch.uint8, device="cuda")
    hip.denoise_guided(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H, gws.data_ptr(),
                       rad.data_ptr(), rgb.data_ptr(), hip.guided_opts())
    torch.cuda.synchronize()
    host = lambda t: t.cpu().numpy()  # noqa: E731
    return SimpleNamespace(rad=host(rad), rgb=host(rgb), length=host(ol), albedo=host(alb), normal=host(nor), depth=host(dep), coverage=host(cov), motion=host(mv))


def check_files(f, lib):
    assert same(read_pfm(f.pfm), lib.rad)
    assert np.array_equal(ppm(f.out, W, H), lib.rgb)
    grey = ppm(f.hmap, W, H)
    assert np.array_equal(grey[..., 0], ((lib.length / f32(32)) * f32(255)).astype(np.uint8))
    assert same(read_pfm(f"{f.feat}.albedo.pfm"), lib.albedo) and same(read_pfm(f"{f.feat}.normal.pfm"), lib.normal)
    assert same(read_pfm(f"{f.feat}.depth.pfm")[..., 1], lib.depth) and same(read_pfm(f"{f.feat}.coverage.pfm")[..., 2], lib.coverage)
    assert same(read_pfm(f"{f.feat}.motion.pfm"), lib.motion)


@pytest.mark.parametrize("factor", [1, 2], ids=["full_size", "upscale_2"])
def test_cli_motion_step_equals_the_library_calls(hip, tmp_path, factor):
    """--frames 3 --motion-step 1 --denoise-guided, and again with --upscale 2: the image, the radiance, the history map and the
    five feature files are what the library calls give, whose accumulation is np_animation's in numpy frame by frame; the motion
    file is the restatement's motion buffer of the last frame's phase; the report names the step."""
    import torch
    hsn = abi.HostScene(CFG, H, W)
    assert hsn.motion is not None and hsn.lens is None
    f = run_cli(tmp_path, "step", "--motion-step", "1", "--denoise-guided", *(("--upscale", "2") if factor > 1 else ()))
    js = json.loads(Path(f.rep).read_text())
    assert js["motion_step"] == 1 and js["frames"] == FRAMES and len(js["moving_spheres"]) == 2
    lib = library_frames(hip, torch, hsn, 1.0, factor, True)
    check_files(f, lib)
    sc = abi.SceneData(spheres=[(tuple(s.center), s.radius, s.mat) for s in (hsn.struct.spheres[i] for i in range(hsn.struct.n_spheres))])
    _, mv = NA.features(hsn.camera, sc, abi.default_opts(spp=N_SPP, seed=SEED + FRAMES - 1), FS, hsn.motion, phase=f32(FRAMES - 1) * f32(1.0))
    assert same(lib.motion, mv) and mv.any()
    assert lib.length.max() == FRAMES


def test_cli_a_step_of_zero_is_no_flag_at_all(hip, tmp_path):
    """--motion-step 0 and no flag: every file byte for byte; both are the plain accumulation's library calls; --no-motion with a
    step renders the still scene and reports no step."""
    import torch
    hsn = abi.HostScene(CFG, H, W)
    a = run_cli(tmp_path, "none", "--denoise-guided")
    b = run_cli(tmp_path, "zero", "--denoise-guided", "--motion-step", "0")
    names = [("out", "out"), ("pfm", "pfm"), ("hmap", "hmap")]
    for x, y in names:
        assert Path(getattr(a, x)).read_bytes() == Path(getattr(b, y)).read_bytes(), x
    for ext in ("albedo", "normal", "depth", "coverage", "motion"):
        assert Path(f"{a.feat}.{ext}.pfm").read_bytes() == Path(f"{b.feat}.{ext}.pfm").read_bytes(), ext
    ja, jb = json.loads(Path(a.rep).read_text()), json.loads(Path(b.rep).read_text())
    assert "motion_step" not in ja and jb["motion_step"] == 0
    lib = library_frames(hip, torch, hsn, 0.0, 1, False)
    check_files(a, lib)
    moved = run_cli(tmp_path, "one", "--denoise-guided", "--motion-step", "1")
    assert Path(moved.pfm).read_bytes() != Path(a.pfm).read_bytes()
    still = run_cli(tmp_path, "still", "--denoise-guided", "--motion-step", "1", "--no-motion")
    js = json.loads(Path(still.rep).read_text())
    assert "motion_step" not in js and "moving_spheres" not in js and not Path(f"{still.feat}.motion.pfm").exists()
