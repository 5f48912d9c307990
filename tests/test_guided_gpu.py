"""The guided denoiser on the GPU (rbrt_hip_denoise_guided, rbrt_hip_scene_denoise_guided) against its numpy restatement
(np_guided.py), bit for bit, and against a converged render.

Synthetic inputs (guided_cases.synthetic) go through denoise_guided: weights strictly between 0 and 1, a block with A == B, a
block of values up to 1e6, steps in every feature; sizes below the filter's reach, ragged, one below / at / one above the level
kernel's tile edge (RBRT_GUIDED_TILE) in each direction, with interior workgroups, and sizes at which the widest level's 25 taps
are all inside for some pixels and not for others. Every case runs with the level kernel reading global memory and with its
tiles staged in LDS at every step that allows it: both are the rule. Through a handle the cases are test_adaptive_gpu.py's."""
from __future__ import annotations

import ctypes as C
import functools
import json
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import guided_cases as GC
import np_adaptive as A
import np_denoise as D
import np_guided as G
import scenes
import test_adaptive_gpu as T
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
EDGE = int(re.search(r"#define RBRT_GUIDED_TILE (\d+)u", (ROOT / "include" / "rbrt_hip_debug.h").read_text()).group(1))

#         W   H
SIZES = [(1, 1), (5, 3), (8, 8), (37, 21),
         (EDGE - 1, 3), (EDGE, 3), (EDGE + 1, 3), (3, EDGE - 1), (3, EDGE), (3, EDGE + 1),
         (48, 48), (50, 47), (80, 17), (17, 80)]   # ... with interior workgroups, ragged last ones, rows of one pixel
# the parameter rows: the defaults with these changes
PARAMS = {"L1": dict(levels=1), "defaults": {}, "L6": dict(levels=6), "no_demodulation": dict(flags=G.NO_DEMODULATION),
          "colour_1e-3": dict(colour=1e-3), "sigmas_1e3": dict(colour=1e3, normal=1e3, depth=1e3, albedo=1e3), "wa_null": dict(wa=None)}
# sizes at which all 25 taps of the widest level (reach 2 << (L - 1)) are inside for some pixels and outside for others
WIDE = [(70, 70, 5), (130, 18, 6), (18, 130, 6), (140, 133, 6)]
STAGING = [0, 4]  # rbrt_hip_debug_guided_staging: no level staged in LDS / every level up to step 4


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def params_of(row):
    p = dict(G.DEFAULTS, **PARAMS[row])
    use_wa = p.pop("wa", True) is not None
    return p, use_wa


@functools.lru_cache(maxsize=None)
def expected(w, h, row, levels=None):
    """The restatement's result for a synthetic case: made once, shared, never changed."""
    a, b, wa, rho, N, z, cov = GC.synthetic(w, h)
    p, use_wa = params_of(row)
    if levels is not None:
        p["levels"] = levels
    out, rgb = G.denoise(a, b, wa if use_wa else None, rho, N, z, cov, **p)
    out.flags.writeable = False
    rgb.flags.writeable = False
    return out, rgb


@pytest.fixture
def staged(hip, request):
    """The level kernel's two forms, set for the test and put back behind it."""
    before = hip.guided_staging()
    assert hip.guided_staging(request.param) == request.param
    yield request.param
    hip.guided_staging(before)


def run_guided(hip, torch, inputs, p, use_wa=True, want_rad=True, want_rgb=True, out_on_a=False, workspace=None):
    """One denoise_guided call into buffers full of sentinels. -> (radiance, rgb8, workspace tensor)."""
    a, b, wa, rho, N, z, cov = inputs
    h, w, _ = a.shape
    dev = [torch.from_numpy(np.ascontiguousarray(x).copy()).cuda() for x in (a, b, wa, rho, N, z, cov)]
    rad = dev[0] if out_on_a else torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    rgb = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
    n_ws = hip.guided_workspace_bytes(w, h)
    assert n_ws == w * h * 96
    ws = workspace if workspace is not None else torch.full((n_ws,), 0xAB, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0 and ws.numel() >= n_ws
    hip.denoise_guided(0, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr() if use_wa else None, dev[3].data_ptr(),
                       dev[4].data_ptr(), dev[5].data_ptr(), dev[6].data_ptr(), w, h, ws.data_ptr(),
                       rad.data_ptr() if want_rad else None, rgb.data_ptr() if want_rgb else None, hip.guided_opts(**p))
    torch.cuda.synchronize()
    return rad.cpu().numpy(), rgb.cpu().numpy(), ws


# ---- 1. synthetic inputs against the restatement ------------------------------------------------------------------------------
def test_the_synthetic_inputs_exercise_the_rule():
    """Conditions on the inputs: at the defaults the weights of the taps one pixel to the right are neither all 0 nor all 1;
    there is a block with A == B (V = 0 inside it), a block that reaches 1e6 and stays within it, a step in albedo, normal and
    depth, background pixels and partly covered ones; and at the wide sizes some pixels have all 25 taps of the widest level
    inside and others do not."""
    for w, h in ((37, 21), (48, 48)):
        a, b, wa, rho, N, z, cov = GC.synthetic(w, h)
        m, u, I, V = G.prepare(a, b, wa, rho, cov)
        pr = G._pairs(h, w, 0, 1)
        wt = G.tap_weight(N, z, m, I, V, pr, f32(1), *G.constants(2.0, 0.35, 0.05, 0.1))
        assert ((wt > 0.01) & (wt < 0.99)).sum() > 100 and (wt == 0).any() and (wt > 0.9).any(), np.histogram(wt, 10, (0, 1))[0]
        assert (V[:h // 2 - 1, :w // 2 - 1] == 0).all() and (V[h // 2 + 2:] > 0).all()
        assert a.max() == f32(1e6) and b.max() == f32(1e6) and ((wa > 0) & (wa < 1)).all()
        assert (np.abs(np.diff(rho, axis=1)) > 0.15).any() and (np.abs(np.diff(N[..., 0], axis=1)) > 0.5).any()
        assert (np.abs(np.diff(z, axis=0)) > 2).any() and (cov == 0).any() and (cov == 0.5).any() and (z[cov == 0] == 0).all()
    for w, h, L in WIDE:
        reach = 2 << (L - 1)  # the outermost taps of the widest level, along an axis that is long enough for them
        some = [n for n in (w, h) if n > 2 * reach]
        assert some and all(n < 4 * reach for n in some), (w, h, L)  # (some pixels have both inside, the ones at the rim do not)


def check_case(hip, w, h, row, levels=None):
    import torch
    p, use_wa = params_of(row)
    if levels is not None:
        p["levels"] = levels
    exp, exp8 = expected(w, h, row, levels)
    rad, rgb, _ = run_guided(hip, torch, GC.synthetic(w, h), p, use_wa)
    assert np.array_equal(bits(rad), bits(exp)), (int((bits(rad) != bits(exp)).sum()), float(np.nanmax(np.abs(rad - exp))))
    assert np.array_equal(rgb, exp8)
    assert np.array_equal(exp8, G.quantise(exp))


@pytest.mark.parametrize("staged", STAGING, ids=["global", "lds"], indirect=True)
@pytest.mark.parametrize("row", list(PARAMS))
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_against_the_restatement(hip, staged, w, h, row):
    check_case(hip, w, h, row)


@pytest.mark.parametrize("staged", STAGING, ids=["global", "lds"], indirect=True)
@pytest.mark.parametrize("w,h,levels", WIDE, ids=[f"{w}x{h}_L{l}" for w, h, l in WIDE])
def test_the_widest_level_inside_and_outside(hip, staged, w, h, levels):
    check_case(hip, w, h, "defaults", levels)
    check_case(hip, w, h, "sigmas_1e3", levels)


# ---- 2. outputs and workspace ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("staged", STAGING, ids=["global", "lds"], indirect=True)
def test_outputs_one_at_a_time_in_place_and_any_workspace(hip, staged):
    import torch
    w, h = 50, 47
    inputs = GC.synthetic(w, h)
    p, _ = params_of("defaults")
    exp, exp8 = expected(w, h, "defaults")
    rad, rgb, _ = run_guided(hip, torch, inputs, p, want_rgb=False)
    assert np.array_equal(bits(rad), bits(exp)) and (rgb == 77).all()
    rad, rgb, _ = run_guided(hip, torch, inputs, p, want_rad=False)
    assert np.isnan(rad).all() and np.array_equal(rgb, exp8)
    rad, rgb, ws = run_guided(hip, torch, inputs, p, out_on_a=True)  # the output exactly on d_a
    assert np.array_equal(bits(rad), bits(exp)) and np.array_equal(rgb, exp8)
    rad, rgb, _ = run_guided(hip, torch, inputs, p, workspace=ws)    # a used workspace
    assert np.array_equal(bits(rad), bits(exp)) and np.array_equal(rgb, exp8)
    zeros = torch.zeros((hip.guided_workspace_bytes(w, h),), dtype=torch.uint8, device="cuda")
    rad, rgb, _ = run_guided(hip, torch, inputs, p, workspace=zeros)
    assert np.array_equal(bits(rad), bits(exp))
    rad, rgb, _ = run_guided(hip, torch, inputs, p, want_rad=False, want_rgb=False)  # nothing asked for: nothing written
    assert np.isnan(rad).all() and (rgb == 77).all()


# ---- 3. through a handle --------------------------------------------------------------------------------------------------------
FEATURE_SAMPLES = 3


@pytest.fixture(scope="module")
def data(hip, oracle):
    """Per case of test_adaptive_gpu.py, the ones test_denoise_gpu.py runs through a handle (the spheres scene, the scene with
    a mesh and every other feature, and a sky that is background only; even and odd counts, ragged sizes): the restatement's
    tile counts, half images and mix at the thresholds zero and median. Made once, never changed."""
    import torch
    d = {}
    for cid, scene, w, h, n, mn, step in T.CASES:
        cam, lens, sc, opts_of = T.build(oracle, scene, w, h)
        with hip.HipScene(sc) as hs:
            samples = T.extract_samples(hs, torch, cam, lens, opts_of, n)
            hs.check()
        r0 = A.adaptive(samples, 0.0, mn, step)
        thr = dict(zero=0.0, median=float(f32(np.median(r0.round_errors[0]))))
        rest = {}
        for kind, t in thr.items():
            r = r0 if kind == "zero" else A.adaptive(samples, t, mn, step)
            a, b, wa = D.halves(*D.halves_from_samples(samples, r.counts), r.counts)
            rest[kind] = SimpleNamespace(counts=r.counts, a=a, b=b, wa=wa, noisy=r.image)
        d[cid] = SimpleNamespace(cid=cid, scene=scene, w=w, h=h, n=n, mn=mn, step=step, cam=cam, lens=lens, sc=sc, opts_of=opts_of,
                                 thr=thr, rest=rest)
    return d


def features_of(hs, torch, cam, opts, w, h, lens=None, samples=FEATURE_SAMPLES):
    t = SimpleNamespace(albedo=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"),
                        normal=torch.zeros((h, w, 3), dtype=torch.float32, device="cuda"),
                        depth=torch.zeros((h, w), dtype=torch.float32, device="cuda"),
                        coverage=torch.zeros((h, w), dtype=torch.float32, device="cuda"))
    hs.render_features(cam, opts, samples, t.albedo.data_ptr(), t.normal.data_ptr(), t.depth.data_ptr(), t.coverage.data_ptr(), lens=lens)
    torch.cuda.synchronize()
    return t


def handle_guided(hip, hs, torch, ft, w, h, **p):
    rad = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    rgb = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
    ws = torch.full((hip.guided_workspace_bytes(w, h),), 0xAB, dtype=torch.uint8, device="cuda")
    hs.denoise_guided(ft.albedo.data_ptr(), ft.normal.data_ptr(), ft.depth.data_ptr(), ft.coverage.data_ptr(), ws.data_ptr(),
                      rad.data_ptr(), rgb.data_ptr(), hip.guided_opts(**p))
    torch.cuda.synchronize()
    return rad.cpu().numpy(), rgb.cpu().numpy()


def handle_nlm(hs, torch, w, h):
    rad = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    hs.denoise(rad.data_ptr())
    torch.cuda.synchronize()
    return rad.cpu().numpy()


@pytest.mark.parametrize("kind", ["zero", "median"])
@pytest.mark.parametrize("cid", T.IDS)
def test_a_handle_filters_its_last_adaptive_render(hip, data, cid, kind):
    import torch
    c = data[cid]
    r = c.rest[kind]
    with hip.HipScene(c.sc) as hs:
        g = T.run_adaptive(hs, torch, c, c.thr[kind])
        assert np.array_equal(g.counts, A.per_rank(r.counts)) and np.array_equal(bits(g.rad), bits(r.noisy)), (cid, kind)
        nlm_before = handle_nlm(hs, torch, c.w, c.h)
        ft = features_of(hs, torch, c.cam, c.opts_of(c.n), c.w, c.h, c.lens)
        feats = [x.cpu().numpy() for x in (ft.albedo, ft.normal, ft.depth, ft.coverage)]
        for p in ({}, dict(levels=3, flags=G.NO_DEMODULATION, colour=1.0)):
            exp, exp8 = G.denoise(r.a, r.b, r.wa, *feats, **dict(G.DEFAULTS, **p))
            rad, rgb = handle_guided(hip, hs, torch, ft, c.w, c.h, **p)
            assert np.array_equal(bits(rad), bits(exp)), (cid, kind, p, int((bits(rad) != bits(exp)).sum()))
            assert np.array_equal(rgb, exp8)
            assert not np.array_equal(bits(exp), bits(r.noisy))
        ws = torch.full((hip.guided_workspace_bytes(c.w, c.h),), 0xAB, dtype=torch.uint8, device="cuda")
        hs.denoise_guided(ft.albedo.data_ptr(), ft.normal.data_ptr(), ft.depth.data_ptr(), ft.coverage.data_ptr(), ws.data_ptr())
        torch.cuda.synchronize()
        assert (ws == 0xAB).all()                                                      # no output asked for: nothing ran
        assert np.array_equal(bits(handle_nlm(hs, torch, c.w, c.h)), bits(nlm_before))  # the other filter gives what it gave
        rad, _ = handle_guided(hip, hs, torch, ft, c.w, c.h)                           # ... and so does this one behind it
        assert np.array_equal(bits(rad), bits(G.denoise(r.a, r.b, r.wa, *feats)[0]))
        hs.check()


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals(hip, data):
    """Every refusal of both entry points with real device pointers: nothing is written."""
    import torch
    c = data["spheres_37x21_odd"]
    lib = hip.load_hip()
    w, h = c.w, c.h
    buf = torch.full((h, w, 3), 0.25, dtype=torch.float32, device="cuda")
    out = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    ws = torch.full((hip.guided_workspace_bytes(w, h),), 0xAB, dtype=torch.uint8, device="cuda")
    p, O = buf.data_ptr(), hip.guided_opts
    nan, inf = float("nan"), float("inf")
    ok = dict(a=p, b=p, albedo=p, normal=p, depth=p, coverage=p, w=w, h=h, opts=O(), ws=ws.data_ptr())
    bad = {"null albedo": dict(albedo=0), "null normal": dict(normal=0), "null depth": dict(depth=0), "null coverage": dict(coverage=0),
           "null opts": dict(opts=None), "null workspace": dict(ws=0), "misaligned workspace": dict(ws=ws.data_ptr() + 8),
           "levels 0": dict(opts=O(levels=0)), "levels 7": dict(opts=O(levels=7)), "flag 2": dict(opts=O(flags=2)),
           "reserved 0": dict(opts=O(reserved=(1, 0))), "reserved 1": dict(opts=O(reserved=(0, 1)))}
    for name in ("colour", "normal", "depth", "albedo"):
        for what, v in (("0", 0.0), ("negative", -0.5), ("nan", nan), ("inf", inf)):
            bad[f"{name} {what}"] = dict(opts=O(**{name: v}))

    def halves(**kw):
        k = dict(ok, **kw)
        o = k["opts"]
        rc = lib.rbrt_hip_denoise_guided(0, None, C.c_void_p(k["a"]), C.c_void_p(k["b"]), None, C.c_void_p(k["albedo"]),
                                         C.c_void_p(k["normal"]), C.c_void_p(k["depth"]), C.c_void_p(k["coverage"]), k["w"], k["h"],
                                         C.byref(o) if o is not None else None, C.c_void_p(k["ws"]), C.c_void_p(out.data_ptr()), None)
        return rc, lib.rbrt_hip_last_error().decode()

    def scene_call(hs, scene=True, **kw):
        k = dict(ok, **kw)
        o = k["opts"]
        rc = lib.rbrt_hip_scene_denoise_guided(hs._h if scene else None, C.byref(o) if o is not None else None, None,
                                               C.c_void_p(k["albedo"]), C.c_void_p(k["normal"]), C.c_void_p(k["depth"]),
                                               C.c_void_p(k["coverage"]), C.c_void_p(k["ws"]), C.c_void_p(out.data_ptr()), None)
        return rc, lib.rbrt_hip_last_error().decode()

    for what, kw in dict(bad, **{"null a": dict(a=0), "null b": dict(b=0), "width 0": dict(w=0), "height 0": dict(h=0)}).items():
        rc, msg = halves(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (what, rc, msg)
    assert halves(w=1 << 16, h=1 << 15)[0] == abi.RBRT_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all() and (ws == 0xAB).all()  # nothing ran
    assert halves()[0] == abi.RBRT_OK
    torch.cuda.synchronize()
    out.fill_(float("nan"))
    ws.fill_(0xAB)
    with hip.HipScene(c.sc) as hs:
        rc, msg = scene_call(hs)  # no adaptive render on the handle yet
        assert rc == abi.RBRT_ERR_INVALID_ARG and "adaptive" in msg, (rc, msg)
        hs.render_adaptive(c.cam, c.opts_of(c.n), T.HUGE, c.mn, c.step)
        for what, kw in dict(bad, **{"null scene": dict(scene=False)}).items():
            rc, msg = scene_call(hs, **kw)
            assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (what, rc, msg)
        hs.render_adaptive(c.cam, c.opts_of(1), T.HUGE, c.mn, c.step)  # spp 1: a half would be empty
        rc, msg = scene_call(hs)
        assert rc == abi.RBRT_ERR_INVALID_ARG and "spp" in msg, (rc, msg)
        hs.render_adaptive(c.cam, c.opts_of(c.n, tile_rank=0, tile_world=2), T.HUGE, c.mn, c.step)
        rc, msg = scene_call(hs)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and "tile_world" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert np.isnan(out.cpu().numpy()).all() and (ws == 0xAB).all()
        # ... and the handle still renders and filters
        T.run_adaptive(hs, torch, c, c.thr["median"])
        assert scene_call(hs)[0] == abi.RBRT_OK
        torch.cuda.synchronize()
        assert np.isfinite(out.cpu().numpy()).all()
        hs.check()


def test_defaults_and_tile_constant(hip):
    g = hip.guided_opts()
    assert (g.levels, g.flags, list(g.reserved)) == (5, 0, [0, 0])
    assert (g.colour, g.normal, g.depth, g.albedo) == (f32(2.0), f32(0.35), f32(0.05), f32(0.1))
    assert EDGE >= 8 and hip.guided_staging() in range(5)


# ---- 5. the command line ----------------------------------------------------------------------------------------------------------
def ppm(p, w, h):
    raw = p.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)


def test_cli_filters_writes_features_and_reports(hip, tmp_path):
    """--denoise-guided: -t gets the restatement's quantisation of the library's own halves and features of the same scene,
    --noisy the unfiltered image; with --features the four PFMs are those of --features alone; --report has the new keys."""
    import torch
    w, h, n, fs = 72, 40, 24, 5
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    out, noisy, rep = tmp_path / "a.ppm", tmp_path / "noisy.ppm", tmp_path / "rep.json"
    base = [str(EXE), "-c", str(cfg), "--height", str(h), "-w", str(w), "-s", str(n), "--seed", "3", "--background", "0,0,0",
            "--feature-samples", str(fs)]
    r = subprocess.run(base + ["-t", str(out), "--denoise-guided", "--guided-levels", "4", "--guided-colour", "1.5", "--noisy", str(noisy),
                               "--features", str(tmp_path / "g"), "--report", str(rep)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run(base + ["-t", str(tmp_path / "b.ppm"), "--features", str(tmp_path / "f")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    for kind in ("albedo", "normal", "depth", "coverage"):
        assert (tmp_path / f"g.{kind}.pfm").read_bytes() == (tmp_path / f"f.{kind}.pfm").read_bytes(), kind
    js = json.loads(rep.read_text())
    assert js["guided_levels"] == 4 and js["guided_colour"] == pytest.approx(1.5, rel=1e-6)
    assert (js["guided_normal"], js["guided_depth"], js["guided_albedo"]) == pytest.approx((0.35, 0.05, 0.1), rel=1e-6)
    assert 0.0 < js["guided_ms"] < 1000.0 and "denoise_ms" not in js
    hsn = abi.HostScene(cfg, h, w)
    o = abi.default_opts(spp=n, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    ha, hb = (torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(2))
    with hip.HipScene(hsn) as hs:
        res = hs.render_adaptive(hsn.camera, o, 0.0, n, n, None, rgb.data_ptr(), lens=hsn.lens)
        assert res["rounds"] == 1
        hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
        ft = features_of(hs, torch, hsn.camera, o, w, h, hsn.lens, fs)
        torch.cuda.synchronize()
        hs.check()
    half = (n + 1) // 2
    wa = np.full((h, w), f32(half) * (f32(1) / f32(n)), f32)
    exp, exp8 = G.denoise(ha.cpu().numpy(), hb.cpu().numpy(), wa, ft.albedo.cpu().numpy(), ft.normal.cpu().numpy(), ft.depth.cpu().numpy(),
                          ft.coverage.cpu().numpy(), **dict(G.DEFAULTS, levels=4, colour=1.5))
    assert np.array_equal(ppm(noisy, w, h), rgb.cpu().numpy())
    assert np.array_equal(ppm(out, w, h), exp8)
    assert not np.array_equal(ppm(out, w, h), ppm(noisy, w, h))


# ---- 6. does it denoise -------------------------------------------------------------------------------------------------------------
def quality(hip, oracle, sc, w=160, h=96, n=16):
    import torch
    cam = scenes.camera(oracle, w, h)
    with hip.HipScene(sc) as hs:
        ref = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        hs.render_device(cam, abi.default_opts(spp=1024, seed=T.SEED + 1), ref.data_ptr())
        noisy = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        res = hs.render_adaptive(cam, abi.default_opts(spp=n, seed=T.SEED), 0.0, 16, 64, noisy.data_ptr())
        assert res["samples"] == w * h * n
        nlm = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        hs.denoise(nlm.data_ptr())
        ft = features_of(hs, torch, cam, abi.default_opts(spp=n, seed=T.SEED), w, h, samples=4)
        guided, _ = handle_guided(hip, hs, torch, ft, w, h)
        hs.check()
    ref, noisy, nlm = (t.cpu().numpy() for t in (ref, noisy, nlm))
    r = SimpleNamespace(noisy=GC.rmse(noisy, ref), nlm=GC.rmse(nlm, ref), guided=GC.rmse(guided, ref))
    print(f"RMSE noisy {r.noisy:.5f}, guided {r.guided:.5f} (ratio {r.guided / r.noisy:.3f}), NLM {r.nlm:.5f} (ratio {r.nlm / r.noisy:.3f})")
    assert np.isfinite(guided).all()
    return r


def test_the_filtered_spheres_are_closer_to_a_converged_render(hip, oracle):
    """The NLM test's case: spheres, 160 x 96, 16 spp in one round, the defaults, features at 4 samples; the reference is the
    fixed path at 1024 spp with another seed. Measured on one MI355X: RMSE of the noisy image 0.01562, of the guided filter's
    0.01136 (0.728 of it), of the NLM's from the same render 0.00895 (0.573) (reported, not asserted)."""
    r = quality(hip, oracle, scenes.spheres_scene())
    assert r.guided < r.noisy, (r.guided, r.noisy)


def test_the_filtered_mesh_scene_is_closer_to_a_converged_render(hip, oracle):
    """The same on the spheres with the stand-in mesh of 1203 triangles, whose facets are feature edges the NLM has to find in
    the noise. Measured on one MI355X: RMSE of the noisy image 0.01696, of the guided filter's 0.01196 (0.705), of the NLM's 0.01064 (0.627)
    (reported, not asserted)."""
    r = quality(hip, oracle, scenes.example_scene(oracle, 1203))
    assert r.guided < r.noisy, (r.guided, r.noisy)
