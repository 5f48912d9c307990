"""Every per-sample feature together on the GPU -- environment lighting, solid patterns, the camera shutter, moving spheres and
the phase, on top of emitters, backgrounds, the lens, smooth meshes and BasicTriangles -- bit for bit against the one joined
restatement, np_whole.py (pinned on the CPU by test_np_whole.py).

The arithmetic of a sample is written out in the trace kernel, in the short-path stage and in the feature kernel, and the tile
pass bounds it: a fuzz over whole_scenes.fuzz_case holds the first against the restatement and the others against the first
(the stage off and forced, the tile pass off, render_pass, render_adaptive, two ranks' tiles), every third seed the feature
buffers too; a hand-built scene shows that the stage finishes most samples with everything on, by the restated rule; the scene
whose every path is parked and resumed runs with everything on under the rows that shrink the grid; and one handle is walked
through sixteen states, each the image of a fresh handle."""
from __future__ import annotations

import functools
import time
from types import SimpleNamespace

import numpy as np
import pytest

import np_env
import np_whole as NW
import scenes
import test_motion_gpu as MG
import whole_scenes as WS
from rbrt_amd import abi, tiles
from test_short_paths_gpu import popcount

pytestmark = pytest.mark.gpu

f32 = np.float32
bits, render = MG.bits, MG.render
ONES = (1 << 64) - 1


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


def where(got, exp):
    return np.argwhere(bits(got) != bits(exp))[:5].tolist()


def copy_opts(opts, **kw):
    o = abi.default_opts(spp=opts.spp, seed=opts.seed, max_depth=opts.max_depth, min_dist=opts.min_dist, max_dist=opts.max_dist, bg=tuple(opts.bg),
                         flags=opts.flags)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def frame(torch, cam):
    return torch.full((cam.img_height_pix, cam.img_width_pix, 3), float("nan"), dtype=torch.float32, device="cuda")


# ---- the fuzz -------------------------------------------------------------------------------------------------------------------------
def feature_buffers(torch, w, h):
    return dict(albedo=torch.full((h, w, 3), float("nan"), device="cuda"), normal=torch.full((h, w, 3), float("nan"), device="cuda"),
                depth=torch.full((h, w), float("nan"), device="cuda"), coverage=torch.full((h, w), float("nan"), device="cuda"),
                object=torch.full((h, w), -7, dtype=torch.int32, device="cuda"), motion=torch.full((h, w, 3), float("nan"), device="cuda"))


@pytest.mark.parametrize("seed", range(WS.N_FUZZ))
def test_fuzzed_scenes_with_every_feature_of_both_generations(hip, oracle, monkeypatch, seed):
    """whole_scenes.fuzz_case: render_device against np_whole.restated_image; then, against that image, the short-path stage off
    and forced, a handle made without the tile pass, render_pass one sample at a time, render_adaptive with threshold 0 and the
    two ranks of tile_world = 2. No case meets a NaN discriminant (test_np_whole.py): no RbrtError is accepted."""
    import torch
    case = WS.fuzz_case(oracle, seed)
    cam, lens, opts = case.cam, case.lens, case.opts
    w, h = cam.img_width_pix, cam.img_height_pix
    if case.builder:
        monkeypatch.setenv("RBRT_BVH_BUILDER", case.builder)
    else:
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    exp, exp8 = WS.restate(NW, case)
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        got, got8 = render(hs, cam, opts, lens)
        hs.check()
        assert same(got, exp), (case.what, where(got, exp))
        assert np.array_equal(got8, exp8), case.what
        for mode in (0, 2):
            hs.set_short_paths(mode)
            again, _ = render(hs, cam, opts, lens)
            assert same(again, got), (case.what, f"set_short_paths({mode})", where(again, got))
        hs.set_short_paths(1)
        acc, out = frame(torch, cam), frame(torch, cam)
        for s in range(opts.spp):
            hs.render_pass(cam, opts, s, s + 1, acc.data_ptr(), out.data_ptr() if s + 1 == opts.spp else None, lens=lens)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), got), (case.what, "render_pass", where(out.cpu().numpy(), got))
        out = frame(torch, cam)
        hs.render_adaptive(cam, opts, 0.0, 2, 1, out.data_ptr(), lens=lens)
        torch.cuda.synchronize()
        assert same(out.cpu().numpy(), got), (case.what, "render_adaptive", where(out.cpu().numpy(), got))
        packed = []
        for rank in range(2):
            buf = torch.full((max(1, hip.packed_pixels(w, h, rank, 2)), 3), float("nan"), dtype=torch.float32, device="cuda")
            hs.render_device(cam, copy_opts(opts, tile_rank=rank, tile_world=2), buf.data_ptr(), lens=lens)
            torch.cuda.synchronize()
            packed.append(buf.cpu().numpy()[:tiles.packed_pixels(w, h, rank, 2)])
        merged = tiles.unpack(packed, w, h)
        assert same(merged, got), (case.what, "tile_world 2", where(merged, got))
        if seed % 3 == 0:
            n = 3
            efeat, emv = NW.features(cam, case.sc, opts, n, lens=lens, shutter=case.shutter, travels=case.travels, phase=case.phase)
            bufs = feature_buffers(torch, w, h)
            hs.render_features(cam, opts, n, lens=lens, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
            torch.cuda.synchronize()
            for k in ("albedo", "normal", "depth", "coverage"):
                g = bufs[k].cpu().numpy()
                assert WS.F.same_bits(g, getattr(efeat, k)), (case.what, k, where(np.nan_to_num(g), np.nan_to_num(getattr(efeat, k))))
            assert np.array_equal(bufs["object"].cpu().numpy(), efeat.object), case.what
            assert same(bufs["motion"].cpu().numpy(), emv), case.what
            if case.travels is None:
                assert not bits(bufs["motion"].cpu().numpy()).any()  # (+0, the sign bit included)
        hs.check()
    monkeypatch.setenv("RBRT_HIP_LAB", "1")
    monkeypatch.setenv("RBRT_PRIMARY_CULL", "0")  # (read when a handle is made)
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        uncut, _ = render(hs, cam, opts, lens)
        hs.check()
    assert same(uncut, got), (case.what, "RBRT_PRIMARY_CULL=0", where(uncut, got))


# ---- the short-path stage does work -----------------------------------------------------------------------------------------------------
SHORT_W, SHORT_H, SHORT_SPP = 24, 16, 4


def restated_masks(case, cull, scatters):
    """The stage's rule (short_paths.inl) for a scene without meshes, from np_whole's record of the hits scatter was called for: a
    sample is finished unless its second ray hits something it has to scatter from; a tile whose first two samples finish fewer
    than three quarters of their slots is given up. -> ({(ty, tx, s): mask} of the tiles on the work list, the masks sorted)."""
    out = {}
    spp = case.opts.spp
    for ty, tx in np.argwhere((cull >> 31) == 0).tolist():
        probe = 0
        for s in range(spp):
            if s == 2 and probe * 4 < 2 * 64 * 3:
                for k in range(2, spp):
                    out[(ty, tx, k)] = 0
                break
            m = 0
            for p in range(64):
                row, col = ty * 8 + p // 8, tx * 8 + p % 8
                fin = not (row < case.cam.img_height_pix and col < case.cam.img_width_pix) or len(scatters[(row, col, s)]) <= 1
                m |= int(fin) << p
            probe += bin(m).count("1") if s < 2 else 0
            out[(ty, tx, s)] = m
    return out, sorted(out.values())


def test_the_short_path_stage_finishes_most_samples_with_everything_on(hip, oracle):
    """whole_scenes.hand_case without a mesh: the example spheres and an emitter, the ground and the moving lambertian patterned, a
    BasicTriangle between them, a lens, a shutter, phase 0.5 and a noise environment. Forced, the stage finishes more than half of
    all sample slots -- the masks are the restated rule's -- and among them samples that took the second colour of the moving
    sphere: surface_entry on the first hit of a moved sphere, environment_radiance at the end."""
    case = WS.hand_case(oracle, SHORT_W, SHORT_H, SHORT_SPP)
    traces, scatters = {}, {}
    exp, exp8 = WS.restate(NW, case, traces=traces, scatters=scatters)
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        hs.set_short_paths(2)
        cull = hs.primary_cull(case.cam, case.opts, case.lens)
        got, got8 = render(hs, case.cam, case.opts, case.lens)
        masks = hs.short_masks()
        hs.check()
        assert hs.last_trace_build() == "general"
    assert same(got, exp), where(got, exp)
    assert np.array_equal(got8, exp8)
    finished = int(popcount(masks).sum())
    print(f"short-path stage: {finished} of {SHORT_W * SHORT_H * SHORT_SPP} sample slots finished, {len(masks)} chunks")
    assert 2 * finished > SHORT_W * SHORT_H * SHORT_SPP
    by_chunk, ordered = restated_masks(case, cull, scatters)
    assert sorted(int(m) for m in masks) == ordered  # (the order of the work list is the library's business)
    second = [(k, p) for k, m in by_chunk.items() for p in range(64)
              if (m >> p) & 1 and (WS.HAND_MOVING, 1) in traces[(k[0] * 8 + p // 8, k[1] * 8 + p % 8, k[2])]]
    first = [(k, p) for k, m in by_chunk.items() for p in range(64)
             if (m >> p) & 1 and (WS.HAND_MOVING, 0) in traces[(k[0] * 8 + p // 8, k[1] * 8 + p % 8, k[2])]]
    print(f"finished samples on the moving sphere: {len(first)} in its first colour, {len(second)} in its second")
    assert second and first


def test_the_short_path_stage_leaves_alone_what_passes_a_mesh(hip, oracle):
    """The same scene with a 13-entry stand-in in front: the tiles whose camera rays can pass its box are the trace kernel's, in
    the others the second rays that pass it are: the image is the restatement's, the masks neither all zero nor all ones."""
    case = WS.hand_case(oracle, SHORT_W, SHORT_H, SHORT_SPP, mesh=True)
    exp, exp8 = WS.restate(NW, case)
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        hs.set_short_paths(2)
        got, got8 = render(hs, case.cam, case.opts, case.lens)
        masks = hs.short_masks()
        hs.set_short_paths(0)
        off, _ = render(hs, case.cam, case.opts, case.lens)
        hs.check()
    assert same(got, exp), where(got, exp)
    assert np.array_equal(got8, exp8) and same(off, got)
    n = popcount(masks)
    print(f"with a mesh in front: {int(n.sum())} sample slots finished in {len(masks)} chunks, {int((n == 0).sum())} chunks left alone")
    assert len(masks) and masks.any() and not (masks == np.uint64(ONES)).all()
    assert (n == 0).any() and (n > 0).any()


def test_the_feature_buffers_with_everything_on(hip, oracle):
    """The same scene with the mesh: the six buffers of three samples under lens, shutter and phase 0.5. The albedo of the patterned
    spheres is the cell's colour at the hit point of the shuttered ray on the sphere where its own s puts it; the motion buffer is
    the moving sphere's travel there; both colours of the moving sphere occur among the primary hits."""
    import torch
    w, h, n = 20, 12, 3
    case = WS.hand_case(oracle, w, h, 2, mesh=True)
    exp, exp_mv = NW.features(case.cam, case.sc, case.opts, n, lens=case.lens, shutter=case.shutter, travels=case.travels, phase=case.phase)
    flat, _ = NW.features(case.cam, WS.with_patterns(case.sc, None), case.opts, n, lens=case.lens, shutter=case.shutter, travels=case.travels, phase=case.phase)
    on_moving = exp.object == WS.HAND_MOVING
    assert (bits(exp.albedo) != bits(flat.albedo)).any(-1)[on_moving].any() and (bits(exp.albedo) == bits(flat.albedo)).all(-1)[on_moving].any()
    bufs = feature_buffers(torch, w, h)
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        hs.render_features(case.cam, case.opts, n, lens=case.lens, **{f"d_{k}": v.data_ptr() for k, v in bufs.items()})
        torch.cuda.synchronize()
        hs.check()
    for k in ("albedo", "normal", "depth", "coverage"):
        assert same(bufs[k].cpu().numpy(), getattr(exp, k)), (k, where(bufs[k].cpu().numpy(), getattr(exp, k)))
    assert np.array_equal(bufs["object"].cpu().numpy(), exp.object)
    assert same(bufs["motion"].cpu().numpy(), exp_mv) and exp_mv[on_moving].any()


# ---- parking with everything on ---------------------------------------------------------------------------------------------------------
PARK_PHASE = 0.5


def park_case(oracle):
    """test_motion_gpu.moving_scene(mesh=True) with patterns on the ground and on the moving lambertian sphere, a noise environment,
    a lens, the SKEW shutter and a phase of 0.5, at test_motion_gpu's size (more chunks than one wave per CU has waves)."""
    base = MG.moving_scene(oracle, mesh=True)
    patterns = {0: abi.checker((0.8, 0.8, 0.7), 1.5, (0.13, -0.21, 0.37)), 1: abi.checker((0.9, 0.2, 0.1), 0.4, (-0.31, 0.17, 0.05))}
    sc = abi.SceneData(spheres=base.spheres, meshes=base.meshes, patterns=patterns)
    cam = scenes.camera(oracle, MG.PARK_W, MG.PARK_H)
    return SimpleNamespace(cam=cam, lens=MG.lens_of(cam), sc=sc, opts=abi.default_opts(spp=MG.PARK_SPP, seed=MG.PARK_SEED, max_depth=MG.DEPTH, bg=(0.4, 0.3, 0.2)),
                           shutter=MG.SKEW, travels=MG.TRAVELS, phase=PARK_PHASE, nodes=np_env.noise_map(8, 3))


def park_pixels():
    """A fixed pseudo-random third of the pixels, as (row, col) in image order."""
    keep = np.random.default_rng(64048).random((MG.PARK_H, MG.PARK_W)) < 1.0 / 3.0
    return [(int(r), int(c)) for r, c in np.argwhere(keep)]


@functools.lru_cache(maxsize=None)
def parked_reference():
    """The restated image of park_case at park_pixels(), made once for every row below (and left unchanged); the seconds it took."""
    from oracle import pyoracle
    case = park_case(pyoracle)
    t0 = time.perf_counter()
    exp, _ = WS.restate(NW, case, pixels=park_pixels())
    seconds = time.perf_counter() - t0
    exp.setflags(write=False)
    return exp, seconds


PARK_DEFAULT = {}  # "image": the default row's first frame, kept for the pixels the restatement leaves out


@pytest.mark.parametrize("rid,env", MG.PARK_ROWS, ids=[r[0] for r in MG.PARK_ROWS])
def test_everything_survives_every_park_and_resume(hip, oracle, monkeypatch, rid, env):
    """Every path alternates between traversals and sphere bounces and is parked and resumed, with one wave per CU and two shade
    rounds in slots that are used again and again: s, the shifted origin, the cell's colour and the environment at the end survive
    it. Two frames issued back to back and a render_pass series; a third of the pixels against the restatement, the others against
    the default row's image."""
    import torch
    exp, seconds = parked_reference()
    print(f"parked reference: {len(park_pixels())} of {MG.PARK_W * MG.PARK_H} pixels restated in {seconds:.1f} s")
    case = park_case(oracle)
    rows, cols = (np.array(x) for x in zip(*park_pixels()))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    outs = [frame(torch, case.cam) for _ in range(2)]
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        hs.set_timing(True)
        for o in outs:
            hs.render_device(case.cam, case.opts, o.data_ptr(), lens=case.lens)
        torch.cuda.synchronize()
        acc, out = frame(torch, case.cam), frame(torch, case.cam)
        for b, e in ((0, 1), (1, 5), (5, MG.PARK_SPP)):
            hs.render_pass(case.cam, case.opts, b, e, acc.data_ptr(), out.data_ptr() if e == MG.PARK_SPP else None, lens=case.lens)
        torch.cuda.synchronize()
        hs.check()
        assert hs.last_trace_build() == "general"
    keep = PARK_DEFAULT
    if rid == "default":
        keep["image"] = outs[0].cpu().numpy()
    for k, o in enumerate(outs + [out]):
        g = o.cpu().numpy()
        assert same(g[rows, cols], exp[rows, cols]), (rid, k, np.argwhere((bits(g[rows, cols]) != bits(exp[rows, cols])).any(-1))[:5].tolist())
        if "image" in keep:
            assert same(g, keep["image"]), (rid, k, where(g, keep["image"]))


# ---- one handle through its states ------------------------------------------------------------------------------------------------------
def test_one_handle_through_sixteen_states(hip, oracle):
    """whole_scenes.walk: one change at a time on one handle -- the tile table's key has to cover camera, lens, shutter, motion and
    phase -- and after each the image of a fresh handle configured directly into that state; after steps 4, 8 and 16 the
    restatement's as well. (test_np_whole.py: the sequence sets, replaces and clears, and reaches every part of the state.)"""
    steps = WS.walk()
    assert len(steps) == 16
    case = WS.walk_case(oracle, steps[0][1])
    with hip.HipScene(case.sc) as hs:
        for k, (what, state) in enumerate(steps, 1):
            case = WS.walk_case(oracle, state)
            kind = what.split()[-1]
            if kind == "shutter":
                hs.set_shutter(case.shutter)
            elif kind == "motion":
                hs.set_motion(case.travels)
            elif kind == "phase":
                hs.set_motion_phase(case.phase)
            elif kind == "environment":
                hs.set_environment(case.nodes)
            got, got8 = render(hs, case.cam, case.opts, case.lens)
            assert hs.last_trace_build() == "general", (k, what)
            with WS.configure(hip.HipScene(case.sc), case) as fresh:
                exp, exp8 = render(fresh, case.cam, case.opts, case.lens)
                fresh.check()
            assert same(got, exp) and np.array_equal(got8, exp8), (k, what, state, where(got, exp))
            if k in (4, 8, 16):
                ref, ref8 = WS.restate(NW, case)
                assert same(got, ref) and np.array_equal(got8, ref8), (k, what, state, where(got, ref))
        hs.check()
