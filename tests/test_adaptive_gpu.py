"""Adaptive sampling on the GPU (rbrt_hip_render_adaptive) against its numpy restatement (np_adaptive.py) and the CPU oracle.

The per-sample radiance the restatement needs comes from the oracle-checked fixed path: sample s of every pixel is
render_pass(spp = N + 1, s, s + 1) into a zeroed accumulator. Thresholds come from the restatement, never from the call
under test. Shapes: 40 x 24 (15 whole tiles) and 37 x 21 (ragged both ways), N = 12 in rounds of 4 and N = 11 after 4 in
rounds of 3. The scene with every feature is seen through a camera aimed at its lamps and objects (FULL_VIEW): through the
example camera more than half of the fifteen tiles are black after four samples -- the constant black background, and
ground no path has yet found a lamp from --, their error is exactly 0, so is the median, and a threshold of 0 stops
nothing: the median row would have one count."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import full_scenes as F
import np_adaptive as A
import np_lens
import scenes
from rbrt_amd import abi, tiles

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
SEED = 7
HUGE = 1e30
FULL_VIEW = dict(look_at=(0.0, -0.3, -1.0), focal_mm=45.0)

#        id                 scene      W   H   N   min step
CASES = [("spheres_40x24", "spheres", 40, 24, 12, 4, 4),
         ("spheres_37x21", "spheres", 37, 21, 12, 4, 4),
         ("spheres_37x21_odd", "spheres", 37, 21, 11, 4, 3),
         ("full_40x24", "full", 40, 24, 12, 4, 4),
         ("full_37x21_odd", "full", 37, 21, 11, 4, 3),
         ("sky_40x24", "sky", 40, 24, 12, 4, 4)]
IDS = [c[0] for c in CASES]
KINDS = ("zero", "huge", "median", "half_median")


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def build(oracle, scene, w, h):
    """(camera, lens or None, scene data, options for spp samples)."""
    if scene == "full":  # (all_features_camera's lens: 20 mm, focused at 9 units)
        cam = scenes.camera(oracle, w, h, **FULL_VIEW)
        lens = np_lens.lens_for(cam, FULL_VIEW["look_at"], FULL_VIEW["focal_mm"], 20.0, 9.0)
        return cam, lens, F.all_features_scene(oracle), lambda spp, **kw: F.all_features_opts(spp, SEED, **kw)
    if scene == "sky":  # looking up: no ray reaches a sphere
        cam = scenes.camera(oracle, w, h, look_at=(0.0, 40.0, -10.0), up=(0.0, 0.0, -1.0))
    else:
        cam = scenes.camera(oracle, w, h)
    return cam, None, scenes.spheres_scene(), lambda spp, **kw: abi.default_opts(spp=spp, seed=SEED, **kw)


def extract_samples(hs, torch, cam, lens, opts_of, n):
    """[n, H, W, 3]: sample s of every pixel, through render_pass into a zeroed accumulator. (The running sums are kept in
    packed tile order whatever tile_world is -- 64 slots per tile, ragged tiles included: the accumulator has that size.)"""
    w, h = cam.img_width_pix, cam.img_height_pix
    out = []
    for s in range(n):
        acc = torch.zeros((tiles.packed_pixels(w, h, 0, 1), 3), dtype=torch.float32, device="cuda")
        hs.render_pass(cam, opts_of(n + 1), s, s + 1, acc.data_ptr(), lens=lens)
        torch.cuda.synchronize()
        out.append(tiles.unpack([acc.cpu().numpy()], w, h))
    return np.stack(out)


@pytest.fixture(scope="module")
def data(hip, oracle):
    """Per case: scene, per-sample radiance, and the restatement's result for the four thresholds. Made once, never changed."""
    import torch
    d = {}
    for cid, scene, w, h, n, mn, step in CASES:
        cam, lens, sc, opts_of = build(oracle, scene, w, h)
        with hip.HipScene(sc) as hs:
            samples = extract_samples(hs, torch, cam, lens, opts_of, n)
            hs.check()
        r0 = A.adaptive(samples, 0.0, mn, step)
        med = f32(np.median(r0.round_errors[0]))  # (fifteen tiles: the median is one of them)
        thr = dict(zero=0.0, huge=HUGE, median=float(med), half_median=float(f32(0.5) * med))
        rest = {k: A.adaptive(samples, thr[k], mn, step) for k in KINDS}
        samples.flags.writeable = False
        d[cid] = SimpleNamespace(cid=cid, scene=scene, w=w, h=h, n=n, mn=mn, step=step, cam=cam, lens=lens, sc=sc, opts_of=opts_of,
                                 samples=samples, thr=thr, rest=rest)
    return d


def run_adaptive(hs, torch, c, threshold, rank=0, world=1, cam=None, n=None):
    """One call with every output asked for, into buffers full of sentinels."""
    cam = cam or c.cam
    w, h = cam.img_width_pix, cam.img_height_pix
    n = n or c.n
    n_local = tiles.local_tiles(w, h, rank, world)
    shape = (h, w, 3) if world == 1 else (n_local * 64, 3)
    rad = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    rgb = torch.full(shape, 77, dtype=torch.uint8, device="cuda")
    cnt = torch.full((n_local,), -1, dtype=torch.int32, device="cuda")
    err = torch.full((n_local,), float("nan"), dtype=torch.float32, device="cuda")
    res = hs.render_adaptive(cam, c.opts_of(n, tile_rank=rank, tile_world=world), threshold, c.mn, c.step, rad.data_ptr(),
                             rgb.data_ptr(), cnt.data_ptr(), err.data_ptr(), lens=c.lens)
    # (no synchronisation here on purpose: the call is blocking, its outputs are complete)
    return SimpleNamespace(rad=rad.cpu().numpy(), rgb=rgb.cpu().numpy(), counts=cnt.cpu().numpy().astype(np.uint32),
                           errors=err.cpu().numpy(), res=res, rounds_active=hs.adaptive_rounds())


def tile_of_pixel(h, w):
    ty, tx = np.meshgrid(np.arange(h) // 8, np.arange(w) // 8, indexing="ij")
    return ty, tx


# ---- 1. the thresholds make the rows they are meant to make ------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_the_restated_thresholds_cover_every_outcome(data, cid):
    c = data[cid]
    n0 = min(c.mn, c.n)
    assert (c.rest["zero"].counts == c.n).all()
    assert (c.rest["huge"].counts == n0).all() and c.rest["huge"].rounds == 1
    assert len(np.unique(c.rest["median"].counts)) >= 2, (cid, c.thr, c.rest["median"].counts)  # (a condition on the case)
    assert c.thr["median"] > 0.0 and np.isfinite(c.thr["median"])
    # the extraction is the oracle's render: the sequential sum of the samples times 1 / N
    s = np.zeros_like(c.samples[0])
    for k in range(c.n):
        s = s + c.samples[k]
    assert np.array_equal(bits(s * (f32(1.0) / f32(c.n))), bits(c.rest["zero"].image))


# ---- 2. against the restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", IDS)
def test_against_the_restatement(hip, data, cid, kind):
    import torch
    c = data[cid]
    r = c.rest[kind]
    with hip.HipScene(c.sc) as hs:
        g = run_adaptive(hs, torch, c, c.thr[kind])
        hs.check()
    what = f"{cid} {kind} threshold {c.thr[kind]!r}"
    assert np.array_equal(g.counts, A.per_rank(r.counts)), (what, g.counts, A.per_rank(r.counts))
    assert np.array_equal(bits(g.errors), bits(A.per_rank(r.errors))), (what, g.errors, A.per_rank(r.errors))
    assert g.res["rounds"] == r.rounds and g.rounds_active == r.round_active, (what, g.res, g.rounds_active, r.round_active)
    assert np.array_equal(bits(g.rad), bits(r.image)), what
    assert np.array_equal(g.rgb, r.rgb8), what
    assert g.res["samples"] == r.samples and g.res["samples_fixed"] == r.samples_fixed == c.w * c.h * c.n, (what, g.res)


# ---- 3. against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", IDS)
def test_every_tile_is_the_fixed_render_at_its_count(hip, oracle, data, cid):
    import torch
    c = data[cid]
    ty, tx = tile_of_pixel(c.h, c.w)
    exp = {}
    exp[c.n] = oracle.render(c.cam, c.sc, c.opts_of(c.n), lens=c.lens)[0]
    assert np.array_equal(bits(exp[c.n]), bits(c.rest["zero"].image))  # (ties the extracted samples to the oracle)
    seen = set()
    with hip.HipScene(c.sc) as hs:
        for kind in ("median", "half_median", "huge"):
            g = run_adaptive(hs, torch, c, c.thr[kind])
            per_pixel = g.counts[tiles.tile_number(ty, tx, (c.w + 7) // 8)]  # every pixel's tile's count
            for n in np.unique(per_pixel):
                n = int(n)
                if n not in exp:
                    exp[n] = oracle.render(c.cam, c.sc, c.opts_of(n), lens=c.lens)[0]
                m = per_pixel == n
                assert np.array_equal(bits(g.rad[m]), bits(exp[n][m])), (cid, kind, n)
                seen.add(n)
        hs.check()
    assert len(seen) >= 2, seen


# ---- 4. threshold 0 is render_device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["spheres_37x21", "full_37x21_odd", "sky_40x24"])
def test_threshold_zero_is_render_device(hip, data, cid):
    import torch
    c = data[cid]
    with hip.HipScene(c.sc) as hs:
        ref = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        ref8 = torch.zeros((c.h, c.w, 3), dtype=torch.uint8, device="cuda")
        hs.render_device(c.cam, c.opts_of(c.n), ref.data_ptr(), ref8.data_ptr(), lens=c.lens)
        torch.cuda.synchronize()
        g = run_adaptive(hs, torch, c, 0.0)
        assert np.array_equal(bits(g.rad), bits(ref.cpu().numpy())) and np.array_equal(g.rgb, ref8.cpu().numpy())
        assert (g.counts == c.n).all() and g.res["samples"] == g.res["samples_fixed"]
        # three ranks' packed tiles, unpacked
        world = 3
        slot = hip.packed_pixels(c.w, c.h, 0, world)
        slots = torch.full((world * slot, 3), float("nan"), dtype=torch.float32, device="cuda")
        total = 0
        for r in range(world):
            p = run_adaptive(hs, torch, c, 0.0, rank=r, world=world)
            assert (p.counts == c.n).all() and len(p.counts) == tiles.local_tiles(c.w, c.h, r, world)
            slots[r * slot:r * slot + p.rad.shape[0]] = torch.from_numpy(p.rad).cuda()
            ref_p = torch.full((p.rad.shape[0], 3), float("nan"), dtype=torch.float32, device="cuda")
            ref_p8 = torch.zeros((p.rad.shape[0], 3), dtype=torch.uint8, device="cuda")
            hs.render_device(c.cam, c.opts_of(c.n, tile_rank=r, tile_world=world), ref_p.data_ptr(), ref_p8.data_ptr(), lens=c.lens)
            torch.cuda.synchronize()
            assert np.array_equal(bits(p.rad), bits(ref_p.cpu().numpy())) and np.array_equal(p.rgb, ref_p8.cpu().numpy())  # (padding slots too)
            total += p.res["samples"]
        merged = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hip.unpack_tiles(0, slots.data_ptr(), c.w, c.h, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        torch.cuda.synchronize()
        assert np.array_equal(bits(merged.cpu().numpy()), bits(ref.cpu().numpy()))
        assert total == c.w * c.h * c.n
        hs.check()


def test_the_ranks_of_a_mixed_render_are_the_whole_render(hip, data):
    """The median row as three ranks: every rank's tiles have the whole render's counts, errors and pixels."""
    import torch
    c = data["full_37x21_odd"]
    r = c.rest["median"]
    with hip.HipScene(c.sc) as hs:
        for rank in range(3):
            p = run_adaptive(hs, torch, c, c.thr["median"], rank=rank, world=3)
            assert np.array_equal(p.counts, A.per_rank(r.counts, rank, 3))
            assert np.array_equal(bits(p.errors), bits(A.per_rank(r.errors, rank, 3)))
            assert np.array_equal(bits(p.rad), bits(tiles.pack(r.image, rank, 3)))
            assert np.array_equal(p.rgb, tiles.pack(r.rgb8, rank, 3))
        hs.check()


CHILD = """import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
import rbrt_amd
from oracle import pyoracle
import test_adaptive_gpu as T
from types import SimpleNamespace
out = {{}}
for cid, scene, w, h, n, mn, step in {cases!r}:
    cam, lens, sc, opts_of = T.build(pyoracle, scene, w, h)
    c = SimpleNamespace(cam=cam, lens=lens, sc=sc, opts_of=opts_of, n=n, mn=mn, step=step)
    with rbrt_amd.HipScene(sc) as hs:
        if {pipeline}:
            hs.set_pipeline({pipeline})
        hs.set_timing(True)
        ref = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(cam, opts_of(n), ref.data_ptr(), lens=lens)
        torch.cuda.synchronize()
        g = T.run_adaptive(hs, torch, c, 0.0)
        out[cid + "_batches"] = np.array(hs.last_batches())
        g2 = T.run_adaptive(hs, torch, c, {huge})
        hs.check()
    out[cid + "_ref"], out[cid + "_rad"], out[cid + "_counts"], out[cid + "_counts_huge"] = ref.cpu().numpy(), g.rad, g.counts, g2.counts
np.savez({out!r}, **out)
"""

ENV_ROWS = [("tile_pass_off", {"RBRT_PRIMARY_CULL": "0"}, 0, None),
            ("helpers_2", {"RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": "1", "RBRT_HELPER_MIN_LAUNCH_MI": "0", "RBRT_HELPER_MIN_FREE": "1"}, 3, None),
            # 168 x 136: 357 tiles, 274,176 B per sample: three samples per batch in 1 MiB, so a round of four is 3 + 1
            ("small_workspace", {"RBRT_HIP_WORKSPACE_MB": "1"}, 0, ("spheres_168x136", "spheres", 168, 136, 12, 4, 4))]


@pytest.mark.parametrize("rid,env,pipeline,extra", ENV_ROWS, ids=[r[0] for r in ENV_ROWS])
def test_threshold_zero_under_other_schedules(hip, data, tmp_path, rid, env, pipeline, extra):
    """Each row in a fresh child process (the knobs are read when the library first needs them): threshold 0 equals the
    child's own render_device and the parent's, bit for bit."""
    import torch
    cases = [CASES[1], CASES[3]] + ([extra] if extra else [])
    script, out = tmp_path / "child.py", tmp_path / "child.npz"
    script.write_text(CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), cases=cases, pipeline=pipeline, huge=HUGE, out=str(out)))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=dict(os.environ, RBRT_HIP_LAB="1", **env))
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    for cid, scene, w, h, n, mn, step in cases:
        assert np.array_equal(bits(z[cid + "_rad"]), bits(z[cid + "_ref"])), (rid, cid)
        assert (z[cid + "_counts"] == n).all() and (z[cid + "_counts_huge"] == mn).all(), (rid, cid)
        if cid in data:
            assert np.array_equal(bits(z[cid + "_rad"]), bits(data[cid].rest["zero"].image)), (rid, cid)
        if extra and cid == extra[0]:
            assert z[cid + "_batches"][1] >= 2 and z[cid + "_batches"][0] < mn, (rid, z[cid + "_batches"])  # a round split into batches


# ---- 5. the handle's other state ----------------------------------------------------------------------------------------------
def test_plain_renders_before_and_after_and_two_sizes_on_one_handle(hip, data):
    """Two image sizes and cameras on one handle, plain renders around every adaptive call. Both sizes, 37 x 21 and 40 x 24,
    are 5 x 3 = 15 tiles: the adaptive state is sized by tiles, so it is allocated once here and never grows. Growth and the
    shrink after it are covered by test_adaptive_many_tiles_gpu.py (test_the_adaptive_state_grows_and_shrinks_on_one_handle)."""
    import torch
    a, b = data["spheres_37x21"], data["spheres_40x24"]

    def plain(hs, c):
        t = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(c.cam, c.opts_of(c.n), t.data_ptr(), lens=c.lens)
        torch.cuda.synchronize()
        return t.cpu().numpy()

    with hip.HipScene(a.sc) as hs:
        for c in (a, b, a):  # (the second size is the larger image, of as many tiles; then the smaller one again)
            before = plain(hs, c)
            assert np.array_equal(bits(before), bits(c.rest["zero"].image))
            for kind in ("median", "zero"):
                g = run_adaptive(hs, torch, c, c.thr[kind])
                assert np.array_equal(g.counts, A.per_rank(c.rest[kind].counts)) and np.array_equal(bits(g.rad), bits(c.rest[kind].image)), (c.cid, kind)
            assert np.array_equal(bits(plain(hs, c)), bits(before)), c.cid
        # a stream of plain frames around an adaptive call
        hs.set_pipeline(3)
        outs = [torch.full((a.h, a.w, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(4)]
        for o in outs[:2]:
            hs.render_device(a.cam, a.opts_of(a.n), o.data_ptr())
        g = run_adaptive(hs, torch, a, a.thr["median"])
        for o in outs[2:]:
            hs.render_device(a.cam, a.opts_of(a.n), o.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(bits(g.rad), bits(a.rest["median"].image))
        for o in outs:
            assert np.array_equal(bits(o.cpu().numpy()), bits(a.rest["zero"].image))
        hs.check()


def test_null_outputs_are_allowed(hip, data):
    c = data["spheres_40x24"]
    with hip.HipScene(c.sc) as hs:
        res = hs.render_adaptive(c.cam, c.opts_of(c.n), c.thr["median"], c.mn, c.step)
        assert res["samples"] == c.rest["median"].samples and res["rounds"] == c.rest["median"].rounds
        a = abi.AdaptiveOpts(c.thr["median"], c.mn, c.step, 0)
        o = c.opts_of(c.n)
        abi.check(hs._lib.rbrt_hip_render_adaptive(hs._h, C.byref(c.cam), C.byref(o), C.byref(a), None, None, None, None, None, None))
        hs.check()


# ---- 6. entry points ----------------------------------------------------------------------------------------------------------
def test_refusals(hip, data):
    c = data["spheres_40x24"]
    lib = hip.load_hip()
    with hip.HipScene(c.sc) as hs:
        def call(scene=True, cam=True, opts=None, a=None, no_opts=False, no_a=False):
            o = opts if opts is not None else c.opts_of(c.n)
            ad = a if a is not None else abi.AdaptiveOpts(0.1, 4, 4, 0)
            res = abi.AdaptiveResult()
            rc = lib.rbrt_hip_render_adaptive(hs._h if scene else None, C.byref(c.cam) if cam else None, None if no_opts else C.byref(o),
                                              None if no_a else C.byref(ad), None, None, None, None, None, C.byref(res))
            return rc, lib.rbrt_hip_last_error().decode()

        zero_cam = abi.Camera()
        C.memmove(C.byref(zero_cam), C.byref(c.cam), C.sizeof(zero_cam))
        zero_cam.img_width_pix = 0
        rows = {
            "null scene": dict(scene=False), "null camera": dict(cam=False), "null options": dict(no_opts=True), "null adaptive": dict(no_a=True),
            "reserved": dict(a=abi.AdaptiveOpts(0.1, 4, 4, 1)),
            "nan threshold": dict(a=abi.AdaptiveOpts(float("nan"), 4, 4, 0)), "inf threshold": dict(a=abi.AdaptiveOpts(float("inf"), 4, 4, 0)),
            "negative threshold": dict(a=abi.AdaptiveOpts(-0.5, 4, 4, 0)),
            "min_samples 0": dict(a=abi.AdaptiveOpts(0.1, 0, 4, 0)), "min_samples 1": dict(a=abi.AdaptiveOpts(0.1, 1, 4, 0)),
            "step 0": dict(a=abi.AdaptiveOpts(0.1, 4, 0, 0)),
            "collect stats": dict(opts=c.opts_of(c.n, flags=abi.FLAG_COLLECT_STATS)),
            "spp 0": dict(opts=c.opts_of(0)), "rank >= world": dict(opts=c.opts_of(c.n, tile_rank=3, tile_world=3)),
            "lens flag without a valid lens": dict(opts=c.opts_of(c.n, flags=abi.FLAG_THIN_LENS)),
        }
        for what, kw in rows.items():
            if what == "lens flag without a valid lens":
                # (the camera is read as the first member of a lens: give it one with a focus_scale of 0)
                bad = abi.camera_lens(c.cam, (0.1, 0.0, 0.0), (0.0, 0.1, 0.0), 1.0)
                bad.focus_scale = 0.0
                res = abi.AdaptiveResult()
                ad = abi.AdaptiveOpts(0.1, 4, 4, 0)
                rc = lib.rbrt_hip_render_adaptive(hs._h, C.byref(bad.cam), C.byref(kw["opts"]), C.byref(ad), None, None, None, None, None, C.byref(res))
                msg = lib.rbrt_hip_last_error().decode()
            else:
                rc, msg = call(**kw)
            assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (what, rc, msg)
        rc, msg = call(opts=c.opts_of(c.n, max_depth=65))  # (render_device's own answer for this one)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and msg
        o = c.opts_of(c.n)
        res = abi.AdaptiveResult()
        ad = abi.AdaptiveOpts(0.1, 4, 4, 0)
        assert lib.rbrt_hip_render_adaptive(hs._h, C.byref(zero_cam), C.byref(o), C.byref(ad), None, None, None, None, None,
                                            C.byref(res)) == abi.RBRT_ERR_INVALID_ARG
        # ... and the handle still renders
        assert hs.render_adaptive(c.cam, c.opts_of(c.n), HUGE, c.mn, c.step)["rounds"] == 1
        hs.check()


def test_cli_renders_adaptively_and_reports_what_the_call_reports(hip, tmp_path):
    import torch
    w, h, n, mn, step, thr = 72, 40, 24, 4, 8, 0.02
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    png, smap, rep = tmp_path / "a.ppm", tmp_path / "map.ppm", tmp_path / "rep.json"
    r = subprocess.run([str(EXE), "-c", str(cfg), "-t", str(png), "--height", str(h), "-w", str(w), "-s", str(n), "--seed", "3",
                        "--background", "0,0,0", "--adaptive", str(thr), "--min-samples", str(mn), "--adaptive-step", str(step),
                        "--sample-map", str(smap), "--report", str(rep)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(rep.read_text())
    hsn = abi.HostScene(cfg, h, w)
    o = abi.default_opts(spp=n, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    n_tiles = tiles.n_tiles(w, h)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros((n_tiles,), dtype=torch.int32, device="cuda")
    with hip.HipScene(hsn) as hs:
        res = hs.render_adaptive(hsn.camera, o, thr, mn, step, None, rgb.data_ptr(), cnt.data_ptr(), lens=hsn.lens)
        active = hs.adaptive_rounds()
        hs.check()
    assert js["adaptive_rounds"] == res["rounds"] and js["samples_traced"] == res["samples"] and js["samples_fixed"] == res["samples_fixed"] == w * h * n
    assert js["active_tiles_per_round"] == active and active[0] == n_tiles and js["samples"] == n
    assert res["samples"] < res["samples_fixed"]  # (the scene's dark tiles stop early)

    def ppm(p):
        raw = p.read_bytes()
        head = f"P6\n{w} {h}\n255\n".encode()
        assert raw.startswith(head)
        return np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)
    assert np.array_equal(ppm(png), rgb.cpu().numpy())
    ty, tx = tile_of_pixel(h, w)
    per_pixel = cnt.cpu().numpy()[tiles.tile_number(ty, tx, (w + 7) // 8)].astype(np.uint64)
    assert np.array_equal(ppm(smap), np.repeat((per_pixel * 255 // n).astype(np.uint8)[..., None], 3, axis=2))
