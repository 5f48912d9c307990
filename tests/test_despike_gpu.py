"""Spike removal on the GPU (rbrt_hip_despike_halves) against its numpy restatement (np_despike.py), bit for bit.

The frozen cases of despike_cases.py go through despike_halves into buffers full of sentinels: sizes of one pixel, ragged
ones, one row and one column, sizes one below, at and one above the kernel's tile (RBRT_DESPIKE_TILE_W x RBRT_DESPIKE_TILE_H),
twice it, and three times it and a little, where an interior workgroup has halos on all four sides; every radius with the
ranks at both ends; a threshold of 1 without a floor and one that limits nothing. Through a handle the halves are a render's
own and the guided filter runs on the despiked ones, and the command line is compared with the same library calls made from
here."""
from __future__ import annotations

import functools
import json
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import despike_cases as DC
import np_despike as ND
import np_guided
import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
TW, TH = DC.TW, DC.TH

PARAMS = {"defaults": {}, "R1 k1": dict(radius=1, rank=1), "R2 k4": dict(radius=2, rank=4), "R1 k4": dict(radius=1, rank=4),
          "t1 f0": dict(threshold=1.0, floor=0.0), "t1e6": dict(threshold=1e6)}
DIRTY = 0xCD  # what the result buffer holds before a call


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


@functools.lru_cache(maxsize=None)
def expected(w, h, row="defaults", nonfinite=True):
    """The restatement's result for a frozen case: made once, shared, never changed. -> (A', B', mask, (spikes_a, spikes_b))"""
    c = DC.case(w, h, nonfinite)
    oa, ob, mask, counts, _ = ND.despike(c.a, c.b, **dict(ND.DEFAULTS, **PARAMS[row]))
    for x in (oa, ob, mask):
        x.flags.writeable = False
    return oa, ob, mask, counts


def run_despike(hip, torch, a, b, p=None, want=("a", "b", "mask", "result"), offset=0):
    """One despike_halves call into buffers full of sentinels; with `offset` every image starts that many bytes (a multiple of 4)
    into its allocation. -> namespace(a, b, mask: numpy; counts: (spikes_a, spikes_b); words: the result's four words)"""
    H, W, _ = a.shape
    n = H * W * 3

    def image(src=None):
        t = torch.full((n + offset // 4,), float("nan"), dtype=torch.float32, device="cuda")
        if src is not None:
            t[offset // 4:] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).copy()).cuda()
        return t

    da, db, oa, ob = image(a), image(b), image(), image()
    mask = torch.full((H * W + 1,), 0x77, dtype=torch.uint8, device="cuda")
    res = torch.full((16,), DIRTY, dtype=torch.uint8, device="cuda")
    m_off = 1 if offset else 0
    hip.despike_halves(0, da.data_ptr() + offset, db.data_ptr() + offset, W, H, oa.data_ptr() + offset if "a" in want else None,
                       ob.data_ptr() + offset if "b" in want else None, mask.data_ptr() + m_off if "mask" in want else None,
                       res.data_ptr() if "result" in want else None, hip.despike_opts(**(p or {})))
    torch.cuda.synchronize()
    words = res.cpu().numpy().view(np.uint32)
    out = lambda t: t.cpu().numpy()[offset // 4:].reshape(H, W, 3)
    assert offset == 0 or (np.isnan(oa.cpu().numpy()[:offset // 4]).all() and np.isnan(ob.cpu().numpy()[:offset // 4]).all())
    return SimpleNamespace(a=out(oa), b=out(ob), mask=mask.cpu().numpy()[m_off:m_off + H * W].reshape(H, W), mask_all=mask.cpu().numpy(),
                           counts=(int(words[0]), int(words[1])), words=words)


def check_case(hip, w, h, row="defaults", nonfinite=True, **kw):
    import torch
    c = DC.case(w, h, nonfinite)
    ea, eb, em, ec = expected(w, h, row, nonfinite)
    g = run_despike(hip, torch, c.a, c.b, PARAMS[row], **kw)
    assert same(g.a, ea) and same(g.b, eb), (w, h, row, int((bits(g.a) != bits(ea)).sum()), int((bits(g.b) != bits(eb)).sum()))
    assert np.array_equal(g.mask, em) and g.counts == ec and g.words[2] == 0 and g.words[3] == 0, (w, h, row, g.counts, ec)
    return c, g


# ---- 1. the frozen cases against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("row", list(PARAMS))
@pytest.mark.parametrize("w,h", DC.SIZES, ids=[f"{w}x{h}" for w, h in DC.SIZES])
def test_sizes_and_parameters(hip, w, h, row):
    clean = row == "t1e6"  # (what is not finite is limited whatever the threshold)
    c, g = check_case(hip, w, h, row, nonfinite=not clean)
    if clean:  # the identity, and both counts 0
        assert same(g.a, c.a) and same(g.b, c.b) and g.counts == (0, 0) and not g.mask.any()


def test_the_parameters_matter_and_the_cases_hold_what_they_should():
    """(conditions on the inputs) every row of PARAMS gives another result on the main case; it limits pixels of both halves, for
    both reasons, either side of a tile edge."""
    w, h = DC.MAIN
    base = expected(w, h)
    for row in PARAMS:
        if row != "defaults":
            assert not same(expected(w, h, row)[0], base[0]) or not np.array_equal(expected(w, h, row)[2], base[2]), row
    c, mask = DC.case(w, h, True), base[2]
    assert base[3][0] > 20 and base[3][1] > 20 and (mask == 3).any()
    assert mask[:, TW - 1].any() and mask[:, TW].any() and mask[TH - 1].any() and mask[TH].any()
    assert (c.bad & (mask != 0)).sum() >= 5


# ---- 2. outputs, the result buffer, alignment ------------------------------------------------------------------------------------
def test_each_output_alone_and_nothing_asked_for(hip):
    import torch
    w, h = DC.MAIN
    c = DC.case(w, h, True)
    ea, eb, em, ec = expected(w, h)
    untouched = dict(a=lambda g: np.isnan(g.a).all(), b=lambda g: np.isnan(g.b).all(), mask=lambda g: (g.mask_all == 0x77).all(),
                     result=lambda g: (g.words == np.uint32(0xCDCDCDCD)).all())
    right = dict(a=lambda g: same(g.a, ea), b=lambda g: same(g.b, eb), mask=lambda g: np.array_equal(g.mask, em) and g.mask_all[-1] == 0x77,
                 result=lambda g: g.counts == ec and not g.words[2:].any())
    for only in ("a", "b", "mask", "result"):
        g = run_despike(hip, torch, c.a, c.b, want=(only,))
        assert right[only](g), only
        assert all(check(g) for name, check in untouched.items() if name != only), only
    g = run_despike(hip, torch, c.a, c.b, want=())  # nothing asked for: nothing launched
    assert all(check(g) for check in untouched.values())


def test_a_dirty_result_buffer_is_zeroed_by_every_call(hip):
    """The same result buffer through three calls in a row without a synchronisation between them: each call's counts are its
    own (the last one flags nothing and leaves zeros)."""
    import torch
    w, h = DC.MAIN
    c = DC.case(w, h, False)
    da, db = torch.from_numpy(c.a.copy()).cuda(), torch.from_numpy(c.b.copy()).cuda()
    res = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    seen = []
    for row in ("defaults", "R1 k4", "t1e6"):
        hip.despike_halves(0, da.data_ptr(), db.data_ptr(), w, h, None, None, None, res.data_ptr(), hip.despike_opts(**PARAMS[row]))
        seen.append(res.clone())
    torch.cuda.synchronize()
    for row, t in zip(("defaults", "R1 k4", "t1e6"), seen):
        assert tuple(t.cpu().numpy().view(np.uint32)) == (*expected(w, h, row, False)[3], 0, 0), row
    assert expected(w, h, "t1e6", False)[3] == (0, 0) and expected(w, h, "defaults", False)[3] != expected(w, h, "R1 k4", False)[3]


@pytest.mark.parametrize("offset", [4, 8, 12])
def test_unaligned_image_pointers(hip, offset):
    check_case(hip, 2 * TW + 1, TH + 3, offset=offset)
    check_case(hip, 5, 3, "R1 k1", offset=offset)


def test_what_is_not_finite_comes_out_finite(hip):
    """NaN, +inf and -inf as centres and as neighbours: every output pixel is finite, the planted ones are flagged, and images that
    are nothing but NaN or infinities come out as the floor everywhere."""
    import torch
    w, h = DC.MAIN
    c, g = check_case(hip, w, h)
    assert c.bad.sum() >= 8 and np.isfinite(g.a).all() and np.isfinite(g.b).all() and (g.mask[c.bad] != 0).all()
    for v in (np.nan, np.inf, -np.inf):
        x = np.full((TH + 1, TW + 1, 3), v, f32)
        g = run_despike(hip, torch, x, x.copy(), dict(radius=1, rank=1))
        assert (g.a == f32(0.01)).all() and (g.b == f32(0.01)).all() and (g.mask == 3).all() and g.counts == (x.shape[0] * x.shape[1],) * 2


def test_refusals_write_nothing(hip):
    import torch
    c = DC.case(5, 3)
    g = None
    for p in (dict(radius=0), dict(radius=3), dict(rank=0), dict(rank=5), dict(threshold=0.5), dict(threshold=float("nan")), dict(floor=-1.0),
              dict(floor=float("inf")), dict(flags=1), dict(reserved=(0, 1, 0))):
        with pytest.raises(abi.RbrtError) as e:
            g = run_despike(hip, torch, c.a, c.b, p)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG, p
    x = torch.full((5 * 3 * 3,), 2.0, dtype=torch.float32, device="cuda")
    y = torch.full((5 * 3 * 3,), 3.0, dtype=torch.float32, device="cuda")
    for kw in (dict(d_out_a=x.data_ptr()), dict(d_out_b=y.data_ptr()), dict(d_mask=x.data_ptr()), dict(d_result=y.data_ptr())):
        with pytest.raises(abi.RbrtError) as e:   # an output that is an input
            hip.despike_halves(0, x.data_ptr(), y.data_ptr(), 5, 3, **kw)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG, kw
    torch.cuda.synchronize()
    assert g is None and bool((x == 2.0).all()) and bool((y == 3.0).all())
    assert (TW, TH) == (abi.DESPIKE_TILE_W, abi.DESPIKE_TILE_H)


# ---- 3. through a handle -----------------------------------------------------------------------------------------------------------
def test_a_handle_despikes_its_own_halves_and_the_guided_filter_takes_them(hip, oracle):
    """A 64 x 48 render of the spheres scene with a small, very bright emitter: the halves of render_adaptive (one round), the
    stage, then the guided filter on the despiked halves equal the restatements fed the downloaded halves and features; the
    handle's later render is what it was."""
    import torch
    W, H, n, fs = 64, 48, 64, 3
    light = ((2.0, 6.0, -8.0), 0.08, abi.material(abi.MAT_EMISSIVE, (3000.0, 2700.0, 2100.0)))
    sc = scenes.spheres_scene(scenes.EXAMPLE_SPHERES + [light])
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    cam = scenes.camera(oracle, W, H)
    with hip.HipScene(sc) as hs:
        before = new(H, W, 3)
        hs.render_device(cam, abi.default_opts(spp=4, seed=9), before.data_ptr())
        o = abi.default_opts(spp=n, seed=31)
        rad, ra, rb, ha, hb, out = new(H, W, 3), new(H, W, 3), new(H, W, 3), new(H, W, 3), new(H, W, 3), new(H, W, 3)
        alb, nor, dep, cov = new(H, W, 3), new(H, W, 3), new(H, W), new(H, W)
        mask = torch.full((H, W), 0x77, dtype=torch.uint8, device="cuda")
        res = torch.full((4,), -1, dtype=torch.int32, device="cuda")
        assert hs.render_adaptive(cam, o, 0.0, n, n, rad.data_ptr())["rounds"] == 1
        hs.denoise(None, None, ra.data_ptr(), rb.data_ptr())
        hip.despike_halves(0, ra.data_ptr(), rb.data_ptr(), W, H, ha.data_ptr(), hb.data_ptr(), mask.data_ptr(), res.data_ptr())
        hs.render_features(cam, o, fs, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
        ws = torch.zeros((hip.guided_workspace_bytes(W, H),), dtype=torch.uint8, device="cuda")
        hip.denoise_guided(0, ha.data_ptr(), hb.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H, ws.data_ptr(),
                           out.data_ptr())
        torch.cuda.synchronize()
        a, b, rho, N, z, c = (t.cpu().numpy() for t in (ra, rb, alb, nor, dep, cov))
        assert np.isfinite(a).all() and np.isfinite(b).all() and not same(a, b)
        ea, eb, em, ec, _ = ND.despike(a, b)
        assert same(ha.cpu().numpy(), ea) and same(hb.cpu().numpy(), eb) and np.array_equal(mask.cpu().numpy(), em)
        assert tuple(res.cpu().numpy().view(np.uint32)) == (*ec, 0, 0)
        print(f"flagged {ec[0]} in A, {ec[1]} in B of {W * H} pixels")
        assert 0 < ec[0] + ec[1] < 0.02 * W * H            # the emitter leaves fireflies, and few
        assert same(out.cpu().numpy(), np_guided.denoise(ea, eb, None, rho, N, z, c)[0])
        after = new(H, W, 3)
        hs.render_device(cam, abi.default_opts(spp=4, seed=9), after.data_ptr())
        torch.cuda.synchronize()
        assert same(after.cpu().numpy(), before.cpu().numpy())
        hs.check()


# ---- 4. the command line --------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    """A colour PFM in numpy: float32 (H, W, 3), top row first."""
    raw = Path(path).read_bytes()
    magic, size, scale, body = raw.split(b"\n", 3)
    assert magic == b"PF" and float(scale) < 0  # colour, little-endian
    w, h = (int(x) for x in size.split())
    assert len(body) == w * h * 12
    return np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1].copy()


def ppm(p, w, h):
    raw = p.read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(head)
    return np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)


@pytest.mark.parametrize("mode", ["alone", "upscale", "frames guided"])
def test_cli_despike_equals_the_library_calls(hip, tmp_path, mode):
    """--despike --despike-threshold 1.5 --despike-rank 3 --despike-radius 1 --spike-map m.ppm --radiance out.pfm --noisy n.ppm at 64 x 48 (alone: the plain mix of the despiked halves; with
    --upscale 2: the stage on the low halves, in front of upsampling; with --frames 3 --denoise-guided: in front of the accumulation
    and the filter) equal what the same library calls give from here; the report has despike_ms, spikes_a and spikes_b, the means
    per frame."""
    import torch
    W, H, n, fs, step, seed, thr, rank, radius = 64, 48, 6, 3, 0.01, 3, 1.5, 3, 1
    f = 2 if mode == "upscale" else 1
    frames = 3 if mode == "frames guided" else 1
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    out, pfm, noisy, rep, smap = tmp_path / "a.ppm", tmp_path / "out.pfm", tmp_path / "n.ppm", tmp_path / "rep.json", tmp_path / "m.ppm"
    extra = {"alone": [], "upscale": ["--upscale", "2", "--feature-samples", str(fs)],
             "frames guided": ["--frames", "3", "--camera-step", f"{step},0,0", "--denoise-guided", "--feature-samples", str(fs)]}[mode]
    r = subprocess.run([str(EXE), "-c", str(cfg), "--height", str(H), "-w", str(W), "-s", str(n), "--seed", str(seed), "--background", "0,0,0",
                        "--despike", "--despike-threshold", str(thr), "--despike-rank", str(rank), "--despike-radius", str(radius), "--spike-map", str(smap), *extra, "--radiance", str(pfm), "--noisy", str(noisy),
                        "--report", str(rep), "-t", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(rep.read_text())
    assert (js["despike_threshold"], js["despike_rank"], js["despike_radius"], js["width"], js["height"]) == (thr, rank, radius, W, H)
    assert 0.0 < js["despike_ms"] < 1000.0 and ("upsample_ms" in js) == (f > 1) and ("temporal_ms" in js) == (frames > 1)
    hsn = abi.HostScene(cfg, H, W)
    assert hsn.lens is None
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    w, h = W // f, H // f
    ra, rb, la, lb, ha, hb, ol = new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w, 3), new(H, W, 3), new(H, W, 3), new(H, W)
    alb, nor, dep, cov, rad, first = new(H, W, 3), new(H, W, 3), new(H, W), new(H, W), new(H, W, 3), new(H, W, 3)
    rgb, first8 = (torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    mask = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
    res = torch.zeros((4,), dtype=torch.int32, device="cuda")
    two = [torch.zeros((hip.temporal_history_bytes(W, H),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    wa = torch.full((H, W), float(f32((n + 1) // 2) * (f32(1) / f32(n))), dtype=torch.float32, device="cuda")
    so = hip.despike_opts(threshold=thr, rank=rank, radius=radius)
    counts = []
    with hip.HipScene(hsn) as hs:
        prev = None
        for k in range(frames):
            cam = type(hsn.camera).from_buffer_copy(hsn.camera)
            shift = f32(k) * f32(step)
            cam.position[0] = f32(hsn.camera.position[0]) + shift
            cam.img_center_point[0] = f32(hsn.camera.img_center_point[0]) + shift
            traced = hip.upsample_camera(cam, f) if f > 1 else cam
            o = abi.default_opts(spp=n, seed=seed + k, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
            # (the render's own image is the unfiltered one of a render without --upscale: in front of the stage)
            assert hs.render_adaptive(traced, o, 0.0, n, n, first.data_ptr() if f == 1 else None, first8.data_ptr() if f == 1 else None)["rounds"] == 1
            hs.denoise(None, None, ra.data_ptr(), rb.data_ptr())
            da, db = (la, lb) if f > 1 else (ha, hb)
            hip.despike_halves(0, ra.data_ptr(), rb.data_ptr(), w, h, da.data_ptr(), db.data_ptr(), mask.data_ptr(), res.data_ptr(), so)
            if mode != "alone":
                hs.render_features(cam, o, fs, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
            if f > 1:
                ws = torch.zeros((hip.upsample_workspace_bytes(W, H, f),), dtype=torch.uint8, device="cuda")
                hip.upsample_halves(0, la.data_ptr(), lb.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H,
                                    ws.data_ptr(), ha.data_ptr(), hb.data_ptr(), None, hip.upsample_opts(factor=f))
                hip.denoise_halves(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), W, H, first.data_ptr(), first8.data_ptr(), window_radius=0)
            if frames > 1:
                hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, prev,
                                        two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr())
            torch.cuda.synchronize()
            counts.append(res.cpu().numpy().view(np.uint32)[:2].astype(np.float64))
            prev = cam
        hs.check()
    if frames > 1:
        gws = torch.zeros((hip.guided_workspace_bytes(W, H),), dtype=torch.uint8, device="cuda")
        hip.denoise_guided(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H,
                           gws.data_ptr(), rad.data_ptr(), rgb.data_ptr())
    else:
        hip.denoise_halves(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), W, H, rad.data_ptr(), rgb.data_ptr(), window_radius=0)
    torch.cuda.synchronize()
    mean = np.mean(counts, axis=0)
    assert js["spikes_a"] == pytest.approx(mean[0], rel=1e-7) and js["spikes_b"] == pytest.approx(mean[1], rel=1e-7) and mean.sum() > 0, (js, counts)
    assert same(read_pfm(pfm), rad.cpu().numpy())
    assert np.array_equal(ppm(out, W, H), rgb.cpu().numpy())
    assert np.array_equal(ppm(noisy, W, H), first8.cpu().numpy())
    grey = ppm(smap, w, h)   # the last frame's mask, at the size that was traced
    m = mask.cpu().numpy()
    assert np.array_equal(grey, np.repeat(ND.spike_map(m)[..., None], 3, -1)) and m.any()
    if mode == "alone":  # the stage changed the image: the target is not the unfiltered one
        assert not same(first.cpu().numpy(), rad.cpu().numpy())
