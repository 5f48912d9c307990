"""The frame pipeline's stages together on the GPU against their composition in numpy (np_pipeline.py), bit for bit, on the frozen
rows of pipeline_cases.py.

a. The library calls, stage by stage, on one handle: render_adaptive (one round), the handle's halves, despike_halves,
   render_features, upsample_halves, temporal_accumulate, one of the three ends, glare, tonemap and compare_images, into buffers
   full of sentinels. Every intermediate equals numpy's; the numpy side is fed the per-sample radiance of render_pass (pinned to
   the oracle by test_adaptive_gpu.py) and the oracle's features, and takes its order from the header, not from the host.
b. The command line, with every output asked for at once, against the same composition; then against the library calls of (a),
   so that a mismatch shows on which side the fault lies.

The rows' conditions (pipeline_cases.check_conditions) are asserted on the numpy side before anything is compared."""
from __future__ import annotations

import json
import math
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import np_features
import np_lens
import np_pipeline as P
import np_tonemap
import np_upsample
import pipeline_cases as PC
import scenes
import test_adaptive_gpu as TA
import test_guided_gpu as TG
from rbrt_amd import abi
from test_compare_gpu import read_grey_pfm
from test_despike_gpu import ppm, read_pfm, same

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
YAML = ROOT / "scenes" / "emissive_spheres.yaml"
f32 = np.float32
CAMERA_FIELDS = ("position", "right", "up", "img_center_point", "mm_per_pix_hor", "mm_per_pix_vert", "img_width_pix", "img_height_pix")


def field(cam, name):
    v = getattr(cam, name)
    return list(v) if hasattr(v, "__len__") else v


def planted(x):
    """A reference for the comparison: x with one pixel not a number, which the stage skips, and one negative, which it does not."""
    ref = np.array(x, f32)
    ref[1, 2, 0], ref[ref.shape[0] // 2, ref.shape[1] // 2] = np.nan, (-0.25, 0.5, 0.125)
    return ref


def numpy_inputs(hs, torch, r, cam0, lens, opts_of, seed, features):
    """The frames np_pipeline is fed: the per-sample radiance of render_pass with the traced camera and seed + k, and the features
    `features(full camera, options)` gives."""
    frames = []
    for k in range(r.frames):
        full, traced = PC.cameras(r, cam0, k)
        s = P.frame_seed(seed, k)
        samples = TA.extract_samples(hs, torch, traced, lens, lambda spp: opts_of(spp, s), r.n)
        assert np.isfinite(samples).all()
        frames.append(P.frame(samples, *features(full, opts_of(r.n, s)), full))
    hs.check()
    return frames


def handle_features(hs, torch, r, lens):
    def features(full, o):
        ft = TG.features_of(hs, torch, full, o, r.w, r.h, lens, PC.FEATURE_SAMPLES)
        return tuple(t.cpu().numpy() for t in (ft.albedo, ft.normal, ft.depth, ft.coverage))
    return features


def chain(hip, torch, hs, r, cam0, lens, opts_of, seed, reference):
    """The library calls of a render with the row's options, into sentinel-filled buffers. -> namespace like np_pipeline's."""
    W, H, n = r.w, r.h, r.n
    f = r.f if r.f else 1
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    new8 = lambda *shape: torch.full(shape, 0x77, dtype=torch.uint8, device="cuda")
    host = lambda t: t.cpu().numpy()
    before = new(H, W, 3)
    hs.render_device(cam0, opts_of(4, 9), before.data_ptr(), lens=lens)
    wa = torch.full((H, W), float(P.mix_weight(n)), dtype=torch.float32, device="cuda")
    two = [new8(hip.temporal_history_bytes(W, H)) for _ in range(2)]
    out = SimpleNamespace(frames=[], cameras=[])
    prev = None
    for k in range(r.frames):
        full = P.frame_camera(cam0, r.step, k)
        traced = hip.upsample_camera(full, f) if f > 1 else full
        w, h = traced.img_width_pix, traced.img_height_pix
        o = opts_of(n, P.frame_seed(seed, k))
        s = SimpleNamespace()
        own, own8, ra, rb = new(h, w, 3), new8(h, w, 3), new(h, w, 3), new(h, w, 3)
        assert hs.render_adaptive(traced, o, 0.0, n, n, own.data_ptr(), own8.data_ptr(), lens=lens)["rounds"] == 1
        hs.denoise(None, None, ra.data_ptr(), rb.data_ptr())
        s.own, s.own8, s.raw_a, s.raw_b = host(own), host(own8), host(ra), host(rb)
        a, b = ra, rb
        if r.despike is not None:
            a, b, mask, res = new(h, w, 3), new(h, w, 3), new8(h, w), torch.full((4,), -1, dtype=torch.int32, device="cuda")
            hip.despike_halves(0, ra.data_ptr(), rb.data_ptr(), w, h, a.data_ptr(), b.data_ptr(), mask.data_ptr(), res.data_ptr(), hip.despike_opts(**r.despike))
            words = host(res).view(np.uint32)
            s.spike_a, s.spike_b, s.mask, s.spikes = host(a), host(b), host(mask), (int(words[0]), int(words[1]))
            assert not words[2:].any()
        alb, nor, dep, cov = new(H, W, 3), new(H, W, 3), new(H, W), new(H, W)
        hs.render_features(full, o, PC.FEATURE_SAMPLES, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), lens=lens)
        s.features = tuple(host(t) for t in (alb, nor, dep, cov))
        s.noisy, s.noisy8 = s.own, s.own8
        if f > 1:
            ws = new8(hip.upsample_workspace_bytes(W, H, f))
            ua, ub, noisy, noisy8 = new(H, W, 3), new(H, W, 3), new(H, W, 3), new8(H, W, 3)
            hip.upsample_halves(0, a.data_ptr(), b.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H, ws.data_ptr(),
                                ua.data_ptr(), ub.data_ptr(), None, hip.upsample_opts(factor=f))
            hip.denoise_halves(0, ua.data_ptr(), ub.data_ptr(), wa.data_ptr(), W, H, noisy.data_ptr(), noisy8.data_ptr(), window_radius=0)
            a, b = ua, ub
            s.up_a, s.up_b, s.noisy, s.noisy8 = host(a), host(b), host(noisy), host(noisy8)
        oa, ob, ol = new(H, W, 3), new(H, W, 3), new(H, W)
        hip.temporal_accumulate(0, a.data_ptr(), b.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), full, prev,
                                two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), oa.data_ptr(), ob.data_ptr(), ol.data_ptr())
        torch.cuda.synchronize()
        s.acc_a, s.acc_b, s.length, s.history = host(oa), host(ob), host(ol), host(two[k & 1]).view(f32).reshape(3, H, W, 4).copy()
        a, b, prev = oa, ob, full
        out.frames.append(s)
        out.cameras.append((full, traced))
    rad, rgb = new(H, W, 3), new8(H, W, 3)
    if r.end == "guided":
        gws = new8(hip.guided_workspace_bytes(W, H))
        hip.denoise_guided(0, a.data_ptr(), b.data_ptr(), wa.data_ptr(), alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H, gws.data_ptr(),
                           rad.data_ptr(), rgb.data_ptr(), hip.guided_opts(**(r.guided or {})))
    else:
        kw = dict(window_radius=0) if r.end == "mix" else dict(r.nlm or {})
        hip.denoise_halves(0, a.data_ptr(), b.data_ptr(), wa.data_ptr(), W, H, rad.data_ptr(), rgb.data_ptr(), **kw)
    torch.cuda.synchronize()
    out.filtered, out.filtered8 = host(rad), host(rgb)

    def display(src, exposure=None, white=None):
        """glare, then the display transform -> (glared or None, rgb8 or None, what the transform chose or None)"""
        glared, rgb8, chosen = None, None, None
        if r.glare is not None:
            g = hip.glare_opts(**r.glare)
            gws, glared, rgb8 = new8(hip.glare_workspace_bytes(W, H, g.levels)), new(H, W, 3), new8(H, W, 3)
            hip.glare(0, src.data_ptr(), W, H, g, gws.data_ptr(), glared.data_ptr(), rgb8.data_ptr())
            src = glared
        if r.tonemap is not None:
            t = dict(r.tonemap)
            if exposure is not None:
                t["exposure"], t["white"] = float(exposure), float(white)
            tws, mapped, rgb8 = new8(abi.TONEMAP_WORKSPACE_BYTES), new(H, W, 3), new8(H, W, 3)
            hip.tonemap(0, src.data_ptr(), W * H, hip.tonemap_opts(**t), tws.data_ptr(), mapped.data_ptr(), rgb8.data_ptr())
            torch.cuda.synchronize()
            chosen = abi.TonemapResult.from_buffer_copy(host(tws)[abi.TONEMAP_RESULT_OFFSET:].tobytes())
        torch.cuda.synchronize()
        return None if glared is None else host(glared), None if rgb8 is None else host(rgb8), chosen

    out.glared, final8, chosen = display(rad)
    out.final8 = out.filtered8 if final8 is None else final8
    out.exposure = None if chosen is None else f32(chosen.exposure)
    out.white = None if chosen is None else f32(chosen.white)
    noisy = torch.from_numpy(out.frames[-1].noisy.copy()).cuda()
    _, noisy8, _ = display(noisy, out.exposure, out.white)
    out.noisy_final8 = out.frames[-1].noisy8 if noisy8 is None else noisy8
    cws, rel, ssim = new8(hip.compare_workspace_bytes(W, H)), new(H, W), new(H, W)
    res = new8(64)
    ref = torch.from_numpy(np.ascontiguousarray(reference, f32)).cuda()
    hip.compare_images(0, rad.data_ptr(), ref.data_ptr(), W, H, cws.data_ptr(), rel.data_ptr(), ssim.data_ptr(), res.data_ptr(), hip.compare_opts(epsilon=0.5))
    torch.cuda.synchronize()
    out.compare = SimpleNamespace(result=host(res).tobytes(), rel_map=host(rel), ssim_map=host(ssim))
    after = new(H, W, 3)
    hs.render_device(cam0, opts_of(4, 9), after.data_ptr(), lens=lens)
    torch.cuda.synchronize()
    out.before, out.after = host(before), host(after)
    hs.check()
    return out


def differences(g, res, r):
    """The names of everything in the library's chain `g` that is not np_pipeline's `res` bit for bit, in the order of the stages."""
    bad = []

    def eq(name, got, exp):
        ok = np.array_equal(got, exp) if np.asarray(exp).dtype == np.uint8 else same(got, exp)
        if not ok:
            bad.append(name)

    for k, (s, e) in enumerate(zip(g.frames, res.frames)):
        eq(f"frame {k}: the render's own image", s.own, e.own), eq(f"frame {k}: its 8-bit image", s.own8, e.own8)
        eq(f"frame {k}: raw half A", s.raw_a, e.raw_a), eq(f"frame {k}: raw half B", s.raw_b, e.raw_b)
        if r.despike is not None:
            eq(f"frame {k}: despiked A", s.spike_a, e.spike_a), eq(f"frame {k}: despiked B", s.spike_b, e.spike_b)
            eq(f"frame {k}: spike mask", s.mask, e.mask)
            if tuple(s.spikes) != tuple(e.spikes):
                bad.append(f"frame {k}: spike counts {s.spikes} != {e.spikes}")
        if r.f:
            eq(f"frame {k}: upsampled A", s.up_a, e.up_a), eq(f"frame {k}: upsampled B", s.up_b, e.up_b)
        eq(f"frame {k}: unfiltered image", s.noisy, e.noisy), eq(f"frame {k}: unfiltered 8-bit image", s.noisy8, e.noisy8)
        eq(f"frame {k}: accumulated A", s.acc_a, e.acc_a), eq(f"frame {k}: accumulated B", s.acc_b, e.acc_b)
        eq(f"frame {k}: history length", s.length, e.length), eq(f"frame {k}: history", s.history, e.history)
    eq("filtered radiance", g.filtered, res.filtered), eq("filtered 8-bit image", g.filtered8, res.filtered8)
    if r.glare is not None:
        eq("glared radiance", g.glared, res.glared)
    if r.tonemap is not None and (g.exposure != res.exposure or g.white != res.white):
        bad.append(f"chosen exposure and white {g.exposure}, {g.white} != {res.exposure}, {res.white}")
    eq("final 8-bit image", g.final8, res.final8), eq("final unfiltered 8-bit image", g.noisy_final8, res.noisy_final8)
    if g.compare.result != res.compare.result:
        bad.append("comparison result")
    eq("error map", g.compare.rel_map, res.compare.rel_map), eq("ssim map", g.compare.ssim_map, res.compare.ssim_map)
    return bad


# ---- a. the library calls, stage by stage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.ROWS))
def test_the_library_calls_stage_by_stage(hip, oracle, name):
    import torch
    r = PC.ROWS[name]
    sc = PC.scene_of(oracle, r)
    cam0 = scenes.camera(oracle, r.w, r.h)
    lens = PC.lens_of(r, cam0)
    opts_of = lambda spp, seed: PC.opts_of(r, spp, seed)
    with hip.HipScene(sc) as hs:
        if r.scene == "mesh":  # (np_features is pinned on scenes without smooth meshes: this scene's features are the handle's own, as in test_guided_gpu.py)
            features = handle_features(hs, torch, r, lens)
        else:
            features = lambda full, o: tuple(np_features.features(oracle, full, sc, o, PC.FEATURE_SAMPLES, lens))[:4]
        frames = numpy_inputs(hs, torch, r, cam0, lens, opts_of, r.seed, features)
        rough = P.pipeline(frames, PC.options(r))
        res = P.pipeline(frames, PC.options(r), planted(rough.noisy))
        PC.check_conditions(name, r, res, frames)
        assert res.compare.skipped == 1 and res.compare.usable == r.w * r.h - 1
        g = chain(hip, torch, hs, r, cam0, lens, opts_of, r.seed, planted(rough.noisy))
    for k, ((full, traced), fr, s) in enumerate(zip(g.cameras, frames, g.frames)):
        low = np_upsample.low_camera(full, r.f) if r.f else full
        for name_ in CAMERA_FIELDS:
            assert field(traced, name_) == field(low, name_), (name, k, name_)
        assert (traced.img_width_pix, traced.img_height_pix) == (res.render_width, res.render_height)
        for what, got, exp in zip(("albedo", "normal", "depth", "coverage"), s.features, (fr.albedo, fr.normal, fr.depth, fr.coverage)):
            assert same(got, exp), (name, k, what)
    bad = differences(g, res, r)
    assert not bad, (name, bad)
    assert same(g.after, g.before)


# ---- b. the command line ------------------------------------------------------------------------------------------------------------------
def cli_arguments(r, tmp):
    a = ["--frames", str(r.frames), "--camera-step", ",".join(str(x) for x in r.step), "--history-map", str(tmp / "h.ppm"),
         "--feature-samples", str(PC.FEATURE_SAMPLES), "--features", str(tmp / "ft")]
    if r.lens:
        a += ["--aperture", str(PC.APERTURE_MM), "--focus-distance", str(PC.FOCUS_DISTANCE)]
    if r.despike is not None:
        a += ["--despike", "--despike-radius", str(r.despike["radius"]), "--despike-rank", str(r.despike["rank"]), "--despike-threshold",
              str(r.despike["threshold"]), "--spike-map", str(tmp / "m.ppm")]
    if r.f:
        a += ["--upscale", str(r.f)]
    if r.end == "nlm":
        a += ["--denoise", "--denoise-radius", str(r.nlm["window_radius"]), "--denoise-patch", str(r.nlm["patch_radius"])]
    if r.end == "guided":
        a += ["--denoise-guided"] + (["--guided-no-demodulation"] if (r.guided or {}).get("flags") else [])
    if r.glare is not None:
        g = dict(P.GLARE_DEFAULTS, **r.glare)
        a += ["--glare", str(g["intensity"]), "--glare-threshold", str(g["threshold"]), "--glare-levels", str(g["levels"])]
    if r.tonemap is not None:
        t = r.tonemap
        a += ["--tonemap", {np_tonemap.LINEAR: "none", np_tonemap.REINHARD: "reinhard", np_tonemap.ACES: "aces"}[t["curve"]],
              "--exposure", "auto" if t["exposure"] == 0.0 else str(math.log2(t["exposure"]))]
        if t["curve"] == np_tonemap.REINHARD:
            a += ["--white", "auto" if t["white"] == 0.0 else str(t["white"])]
    return a


@pytest.mark.parametrize("name", PC.CLI_ROWS)
def test_the_command_line_against_numpy(hip, tmp_path, name):
    """Every output of one run at once. The scene is the YAML's, under a black sky: much noisier than the rows' own, so of the
    rows' conditions the share of flagged pixels is not asked here (few_spikes=False); the features are render_features' on the
    handle (pinned by test_features_gpu.py)."""
    import torch
    r = PC.ROWS[name]
    W, H = r.w, r.h
    hsn = abi.HostScene(YAML, H, W)
    assert hsn.lens is None
    cam0 = hsn.camera
    lens = np_lens.lens_for(cam0, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], PC.APERTURE_MM, PC.FOCUS_DISTANCE) if r.lens else None
    opts_of = lambda spp, seed: abi.default_opts(spp=spp, seed=seed, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    with hip.HipScene(hsn) as hs:
        features = handle_features(hs, torch, r, lens)
        other = numpy_inputs(hs, torch, r, cam0, lens, opts_of, r.cli_seed + 100, features)
        reference = planted(P.pipeline(other, PC.options(r)).filtered)  # the row with another seed
        frames = numpy_inputs(hs, torch, r, cam0, lens, opts_of, r.cli_seed, features)
        res = P.pipeline(frames, PC.options(r), reference)
        PC.check_conditions(name, r, res, frames, few_spikes=False)
        assert res.compare.skipped == 1 and res.compare.sum_se > 0
        ref_file, out, pfm, noisy, rep = tmp_path / "ref.pfm", tmp_path / "a.ppm", tmp_path / "out.pfm", tmp_path / "n.ppm", tmp_path / "rep.json"
        abi.write_pfm(ref_file, reference)
        run = subprocess.run([str(EXE), "-c", str(YAML), "--height", str(H), "-w", str(W), "-s", str(r.n), "--seed", str(r.cli_seed), "--background", "0,0,0",
                              *cli_arguments(r, tmp_path), "--radiance", str(pfm), "--noisy", str(noisy), "--compare", str(ref_file), "--compare-epsilon", "0.5",
                              "--error-map", str(tmp_path / "e.pfm"), "--ssim-map", str(tmp_path / "s.pfm"), "--report", str(rep), "-t", str(out)],
                             capture_output=True, text=True, timeout=300)
        assert run.returncode == 0, run.stderr[-2000:]
        js = json.loads(rep.read_text())
        files = SimpleNamespace(filtered=read_pfm(pfm), final8=ppm(out, W, H), noisy_final8=ppm(noisy, W, H), history=ppm(tmp_path / "h.ppm", W, H),
                                spikes=ppm(tmp_path / "m.ppm", res.render_width, res.render_height), error=read_grey_pfm(tmp_path / "e.pfm"),
                                ssim=read_grey_pfm(tmp_path / "s.pfm"), albedo=read_pfm(tmp_path / "ft.albedo.pfm"), normal=read_pfm(tmp_path / "ft.normal.pfm"),
                                depth=read_grey_pfm(tmp_path / "ft.depth.pfm"), coverage=read_grey_pfm(tmp_path / "ft.coverage.pfm"))
        grey = lambda m: np.repeat(m[..., None], 3, -1)
        last = frames[-1]
        bad = [what for what, ok in (
            ("--radiance", same(files.filtered, res.filtered)), ("the target", np.array_equal(files.final8, res.final8)),
            ("--noisy", np.array_equal(files.noisy_final8, res.noisy_final8)), ("--spike-map", np.array_equal(files.spikes, grey(res.spike_map))),
            ("--history-map", np.array_equal(files.history, grey(res.history_map))), ("--features albedo", same(files.albedo, last.albedo)),
            ("--features normal", same(files.normal, last.normal)), ("--features depth", same(files.depth, last.depth)),
            ("--features coverage", same(files.coverage, last.coverage)), ("--error-map", same(files.error, res.compare.rel_map)),
            ("--ssim-map", same(files.ssim, res.compare.ssim_map))) if not ok]
        assert not bad, (name, bad)
        for k in ("mse", "mae", "relmse", "psnr_db", "ssim"):
            assert js[f"compare_{k}"] == res.summary[k], (name, k, js[f"compare_{k}"], res.summary[k])  # (%.17g round-trips a double)
        assert (js["compare_max_abs"], js["compare_usable"], js["compare_skipped"]) == (float(res.compare.max_abs), W * H - 1, 1)
        assert (js["spikes_a"], js["spikes_b"]) == (float(f"{res.spikes_a:.9g}"), float(f"{res.spikes_b:.9g}")), (name, js["spikes_a"], js["spikes_b"])
        if r.tonemap is not None:
            assert (f32(js["exposure"]), f32(js["white"])) == (res.exposure, res.white), (name, js["exposure"], js["white"])
        if r.f:
            assert (js["render_width"], js["render_height"]) == (res.render_width, res.render_height)
        assert (js["width"], js["height"], js["frames"]) == (W, H, r.frames)
        # the same row through the library calls: they equal numpy, and so the files
        g = chain(hip, torch, hs, r, cam0, lens, opts_of, r.cli_seed, reference)
        assert not differences(g, res, r), (name, differences(g, res, r))
        assert same(g.filtered, files.filtered) and np.array_equal(g.final8, files.final8) and np.array_equal(g.noisy_final8, files.noisy_final8)
        assert same(g.after, g.before)
