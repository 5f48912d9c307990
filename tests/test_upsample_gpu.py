"""Guided upsampling on the GPU (rbrt_hip_upsample_halves) against its numpy restatement (np_upsample.py), bit for bit.

The frozen cases of upsample_cases.py go through upsample_halves into buffers full of sentinels, for every factor 1..4: sizes of
one pixel, ragged ones, one row and one column, widths and heights that are no multiple of the factor, and sizes one below, at
and one above the gather kernel's tile (RBRT_UPSAMPLE_TILE_W x RBRT_UPSAMPLE_TILE_H) and twice it, where an interior workgroup
exists. The packed low records in the workspace are compared too. Through a handle the halves and features are a render's own,
and the command line is compared with the same library calls made from here."""
from __future__ import annotations

import functools
import json
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import np_upsample as NU
import scenes
import upsample_cases as UC
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
_debug = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
TW, TH = (int(re.search(rf"#define RBRT_UPSAMPLE_TILE_{k} (\d+)u", _debug).group(1)) for k in "WH")

#         W   H
SIZES = [(1, 1), (2, 2), (5, 3), (37, 21), (50, 47), (67, 1), (1, 23),                                 # ragged; one row; one column
         (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW, 2 * TH), (3 * TW + 1, 3 * TH + 2),   # around a tile; an interior workgroup
         (TW + 3, 2 * TH - 1)]                                                                       # no multiple of 2, 3 or 4
PARAMS = {"defaults": {}, "flag": dict(flags=1), "tight": dict(normal=0.2, depth=0.03, albedo=0.6), "tight flag": dict(normal=0.2, depth=0.03, albedo=0.6, flags=1)}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


@functools.lru_cache(maxsize=None)
def expected(w, h, f, row="defaults", wa=True):
    """The restatement's result for a frozen case: made once, shared, never changed. -> (A, B, wa, packed records, info)"""
    c = UC.case(w, h, f)
    A, B, wo, info = NU.upsample(c.a, c.b, c.wa if wa else None, c.rho, c.N, c.z, c.cov, factor=f, **dict({k: v for k, v in NU.DEFAULTS.items() if k != "factor"}, **PARAMS[row]))
    packed = NU.pack(info.low)
    for x in (A, B, wo, packed):
        x.flags.writeable = False
    return A, B, wo, packed, info


def up(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def run_upsample(hip, torch, c, p=None, want=("a", "b", "wa"), a=None, b=None, wa="case", workspace=None, offset=0):
    """One upsample_halves call into buffers full of sentinels. -> namespace(a, b, wa: numpy; ws: the workspace's records)"""
    H, W = c.z.shape
    f = c.f
    dev = SimpleNamespace(a=up(torch, c.a if a is None else a), b=up(torch, c.b if b is None else b), rho=up(torch, c.rho), N=up(torch, c.N),
                          z=up(torch, c.z), cov=up(torch, c.cov))
    d_wa = up(torch, c.wa) if isinstance(wa, str) else None if wa is None else up(torch, wa)
    n_ws = hip.upsample_workspace_bytes(W, H, f)
    assert n_ws == c.w * c.h * 64
    ws = workspace if workspace is not None else torch.full((n_ws + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    assert (ws.data_ptr() + offset) % 16 == 0 and ws.numel() >= n_ws + offset
    oa = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    ob = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
    ow = torch.full((H, W), -7.0, dtype=torch.float32, device="cuda")
    hip.upsample_halves(0, dev.a.data_ptr(), dev.b.data_ptr(), d_wa.data_ptr() if d_wa is not None else None, dev.rho.data_ptr(), dev.N.data_ptr(),
                        dev.z.data_ptr(), dev.cov.data_ptr(), W, H, ws.data_ptr() + offset, oa.data_ptr() if "a" in want else None,
                        ob.data_ptr() if "b" in want else None, ow.data_ptr() if "wa" in want else None, hip.upsample_opts(factor=f, **(p or {})))
    torch.cuda.synchronize()
    return SimpleNamespace(a=oa.cpu().numpy(), b=ob.cpu().numpy(), wa=ow.cpu().numpy(), ws_t=ws,
                           ws=ws.cpu().numpy()[offset:offset + n_ws].view(f32).reshape(4, c.h, c.w, 4))


def check_case(hip, w, h, f, row="defaults"):
    import torch
    c = UC.case(w, h, f)
    ea, eb, ew, eh, _ = expected(w, h, f, row)
    g = run_upsample(hip, torch, c, PARAMS[row])
    assert same(g.ws, eh), (w, h, f, row, "records", int((bits(g.ws) != bits(eh)).sum()))
    assert same(g.a, ea) and same(g.b, eb) and same(g.wa, ew), (w, h, f, row, int((bits(g.a) != bits(ea)).sum()), int((bits(g.wa) != bits(ew)).sum()))


# ---- 1. the frozen cases against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes(hip, w, h, f):
    check_case(hip, w, h, f)


@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("row", [r for r in PARAMS if r != "defaults"])
def test_flag_and_sigmas(hip, row, f):
    check_case(hip, 37, 21, f, row)
    check_case(hip, 2 * TW + 5, 2 * TH + 3, f, row)


def test_the_options_matter():
    """(conditions on the inputs) every row of PARAMS gives another result somewhere."""
    for f in (2, 3, 4):
        base = expected(37, 21, f)
        for row in PARAMS:
            if row != "defaults":
                assert not same(expected(37, 21, f, row)[0], base[0]), (f, row)


# ---- 2. outputs, the mix, the workspace -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 3])
def test_each_output_alone_and_nothing_asked_for(hip, f):
    import torch
    w, h = 50, 47
    c = UC.case(w, h, f)
    ea, eb, ew, eh, _ = expected(w, h, f)
    untouched = dict(a=lambda g: np.isnan(g.a).all(), b=lambda g: np.isnan(g.b).all(), wa=lambda g: (g.wa == -7).all())
    exp = dict(a=ea, b=eb, wa=ew)
    for only in ("a", "b", "wa"):
        g = run_upsample(hip, torch, c, want=(only,))
        assert same(getattr(g, only), exp[only]), only
        assert all(check(g) for name, check in untouched.items() if name != only), only
    g = run_upsample(hip, torch, c, want=())  # nothing asked for: nothing launched, the workspace included
    assert all(check(g) for check in untouched.values()) and bool((g.ws_t == 0xAB).all())


@pytest.mark.parametrize("f", [1, 2, 4])
def test_no_mix_is_a_plane_of_one_half(hip, f):
    import torch
    w, h = 37, 21
    c = UC.case(w, h, f)
    ea, eb, ew, eh, _ = expected(w, h, f, wa=False)
    g0 = run_upsample(hip, torch, c, wa=None)
    g1 = run_upsample(hip, torch, c, wa=np.full((c.h, c.w), 0.5, f32))
    for g in (g0, g1):
        assert same(g.a, ea) and same(g.b, eb) and same(g.wa, ew) and same(g.ws, eh)
    assert not same(ew, expected(w, h, f)[2])


def test_any_aligned_workspace_dirty_or_reused(hip):
    """The workspace at every 16-byte offset of a buffer full of garbage, then the same buffer again for another size and factor."""
    import torch
    rng = np.random.default_rng(5)
    big = hip.upsample_workspace_bytes(50, 47, 1) + 64
    ws = torch.from_numpy(rng.integers(0, 256, big, dtype=np.uint8)).cuda()
    base = (-ws.data_ptr()) % 16
    for k, (w, h, f) in enumerate([(50, 47, 1), (50, 47, 3), (37, 21, 2), (50, 47, 2), (5, 3, 4)]):
        c = UC.case(w, h, f)
        ea, eb, ew, eh, _ = expected(w, h, f)
        g = run_upsample(hip, torch, c, workspace=ws, offset=base + 16 * (k % 4))
        assert same(g.a, ea) and same(g.b, eb) and same(g.wa, ew) and same(g.ws, eh), (w, h, f)


# ---- 3. the rule's consequences on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (37, 21), (2 * TW + 1, 2 * TH + 1)])
def test_factor_one_without_demodulation_is_the_identity(hip, w, h):
    import torch
    c = UC.case(w, h, 1)
    g = run_upsample(hip, torch, c, dict(flags=1))
    assert same(g.a, c.a) and same(g.b, c.b) and same(g.wa, c.wa)


@pytest.mark.parametrize("f", [2, 3, 4])
def test_non_finite_low_pixels_stay_within_their_reach(hip, f):
    """NaN and infinities in low pixels that no accepted tap reaches: the run ends without a fault, and the pixels outside the
    listed ones (the fallback pixels whose own low pixel is planted) hold the bits of the run without them."""
    import torch
    w, h = 50, 47
    c = UC.case(w, h, f)
    ea, eb, ew, eh, info = expected(w, h, f)
    a2, b2, w2, bad, listed = UC.planted(c, info)
    assert bad.sum() >= 2 and 0 < listed.sum() < 0.05 * listed.size
    g = run_upsample(hip, torch, c, a=a2, b=b2, wa=w2)
    keep = ~listed
    assert same(g.a[keep], ea[keep]) and same(g.b[keep], eb[keep]) and same(g.wa[keep], ew[keep])
    xa, xb, xw, _ = NU.upsample(a2, b2, w2, c.rho, c.N, c.z, c.cov, factor=f)
    nan_eq = lambda x, y: np.array_equal(np.isnan(x), np.isnan(y)) and same(np.where(np.isnan(x), 0, x), np.where(np.isnan(y), 0, y))
    assert nan_eq(g.a, xa) and nan_eq(g.b, xb) and nan_eq(g.wa, xw)   # the listed pixels too, up to a NaN's payload
    # ... and low halves that are nothing but NaN, or nothing but infinities: every pixel holds something, no fault
    for v in (np.nan, np.inf, -np.inf):
        g = run_upsample(hip, torch, c, a=np.full_like(c.a, v), b=np.full_like(c.b, v), wa=np.full_like(c.wa, v))
        assert (g.wa != -7).all()


# ---- 4. through a handle --------------------------------------------------------------------------------------------------------------------
def test_a_handle_upsamples_its_low_render_and_renders_on_as_before(hip, oracle):
    """The low camera from the helper, render_adaptive (one round) with it, its halves, render_features with the full camera on
    the same handle and upsample_halves equal the restatement fed the downloaded halves and features; the helper's camera is
    the restatement's bit for bit; the handle's later render is what it was."""
    import torch
    W, H, f, n, fs = 48, 32, 2, 6, 3
    sc = scenes.spheres_scene()
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    cam = scenes.camera(oracle, W, H)
    low = hip.upsample_camera(cam, f)
    assert bytes(low) == bytes(NU.low_camera(cam, f)) and (low.img_width_pix, low.img_height_pix) == (24, 16)
    w, h = low.img_width_pix, low.img_height_pix
    with hip.HipScene(sc) as hs:
        before = new(H, W, 3)
        hs.render_device(cam, abi.default_opts(spp=4, seed=9), before.data_ptr())
        o = abi.default_opts(spp=n, seed=11)
        rad, ha, hb = new(h, w, 3), new(h, w, 3), new(h, w, 3)
        alb, nor, dep, cov = new(H, W, 3), new(H, W, 3), new(H, W), new(H, W)
        assert hs.render_adaptive(low, o, 0.0, n, n, rad.data_ptr())["rounds"] == 1
        hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
        hs.render_features(cam, o, fs, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
        ws = torch.full((hip.upsample_workspace_bytes(W, H, f),), 0xAB, dtype=torch.uint8, device="cuda")
        oa, ob, ow = new(H, W, 3), new(H, W, 3), new(H, W)
        hip.upsample_halves(0, ha.data_ptr(), hb.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H,
                            ws.data_ptr(), oa.data_ptr(), ob.data_ptr(), ow.data_ptr(), hip.upsample_opts(factor=f))
        torch.cuda.synchronize()
        a, b, rho, N, z, c = (t.cpu().numpy() for t in (ha, hb, alb, nor, dep, cov))
        assert np.isfinite(a).all() and np.isfinite(b).all() and not same(a, b)
        ea, eb, ew, info = NU.upsample(a, b, None, rho, N, z, c, factor=f)
        assert same(oa.cpu().numpy(), ea) and same(ob.cpu().numpy(), eb) and same(ow.cpu().numpy(), ew)
        assert 0 < info.fallback.mean() < 0.2 and (info.count == 4).any()
        after = new(H, W, 3)
        hs.render_device(cam, abi.default_opts(spp=4, seed=9), after.data_ptr())
        torch.cuda.synchronize()
        assert same(after.cpu().numpy(), before.cpu().numpy())
        hs.check()


# ---- 5. refusals with device pointers ---------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip):
    import torch
    c = UC.case(37, 21, 2)
    g = None
    ws = torch.full((hip.upsample_workspace_bytes(37, 21, 2) + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    for p in (dict(normal=0.0), dict(depth=-1.0), dict(albedo=float("nan")), dict(flags=2), dict(reserved=(0, 0, 1))):
        with pytest.raises(abi.RbrtError) as e:
            g = run_upsample(hip, torch, c, p, workspace=ws)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG, p
    out = torch.full((21, 37, 3), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(abi.RbrtError) as e:   # a workspace that is not 16-byte aligned (every other pointer is a valid one)
        hip.upsample_halves(0, ws.data_ptr(), ws.data_ptr(), None, ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), ws.data_ptr(), 37, 21,
                            ws.data_ptr() + 4, out.data_ptr(), None, None)
    assert e.value.code == abi.RBRT_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert g is None and bool((ws == 0xAB).all()) and bool(torch.isnan(out).all())
    assert (TW, TH) == (abi.UPSAMPLE_TILE_W, abi.UPSAMPLE_TILE_H)


# ---- 6. the command line --------------------------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("mode", ["alone", "frames guided"])
def test_cli_upscale_equals_the_library_calls(hip, tmp_path, mode):
    """--upscale 2 (alone: the plain mix of the upsampled halves; with --frames 3 --denoise-guided: accumulated and filtered at full
    size) --radiance out.pfm --noisy n.ppm --features PREFIX equal what the same library calls give from here; the report has
    upscale, render_width, render_height and upsample_ms."""
    import torch
    W, H, f, n, fs, step, seed = 48, 32, 2, 6, 3, 0.01, 3
    frames = 3 if mode != "alone" else 1
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    out, pfm, noisy, rep, feat = tmp_path / "a.ppm", tmp_path / "out.pfm", tmp_path / "n.ppm", tmp_path / "rep.json", tmp_path / "ft"
    extra = ["--frames", str(frames), "--camera-step", f"{step},0,0", "--denoise-guided", "--history-map", str(tmp_path / "h.ppm")] if frames > 1 else []
    r = subprocess.run([str(EXE), "-c", str(cfg), "--height", str(H), "-w", str(W), "-s", str(n), "--seed", str(seed), "--background", "0,0,0",
                        "--feature-samples", str(fs), "--upscale", str(f), *extra, "--radiance", str(pfm), "--noisy", str(noisy), "--features", str(feat),
                        "--report", str(rep), "-t", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(rep.read_text())
    assert (js["upscale"], js["render_width"], js["render_height"], js["width"], js["height"]) == (f, W // f, H // f, W, H)
    assert 0.0 < js["upsample_ms"] < 1000.0 and js["upscale_normal"] == 0.5 and ("temporal_ms" in js) == (frames > 1)
    hsn = abi.HostScene(cfg, H, W)
    assert hsn.lens is None
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    w, h = W // f, H // f
    la, lb, ha, hb, ol = new(h, w, 3), new(h, w, 3), new(H, W, 3), new(H, W, 3), new(H, W)
    alb, nor, dep, cov, rad, plain = new(H, W, 3), new(H, W, 3), new(H, W), new(H, W), new(H, W, 3), new(H, W, 3)
    rgb, plain8 = (torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda") for _ in range(2))
    ws = torch.zeros((hip.upsample_workspace_bytes(W, H, f),), dtype=torch.uint8, device="cuda")
    two = [torch.zeros((hip.temporal_history_bytes(W, H),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    wa = torch.full((H, W), float(f32((n + 1) // 2) * (f32(1) / f32(n))), dtype=torch.float32, device="cuda")
    with hip.HipScene(hsn) as hs:
        prev = None
        for k in range(frames):
            cam = type(hsn.camera).from_buffer_copy(hsn.camera)
            shift = f32(k) * f32(step)
            cam.position[0] = f32(hsn.camera.position[0]) + shift
            cam.img_center_point[0] = f32(hsn.camera.img_center_point[0]) + shift
            low = hip.upsample_camera(cam, f)
            o = abi.default_opts(spp=n, seed=seed + k, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
            assert hs.render_adaptive(low, o, 0.0, n, n)["rounds"] == 1
            hs.denoise(None, None, la.data_ptr(), lb.data_ptr())
            hs.render_features(cam, o, fs, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
            hip.upsample_halves(0, la.data_ptr(), lb.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H,
                                ws.data_ptr(), ha.data_ptr(), hb.data_ptr(), None, hip.upsample_opts(factor=f))
            if k + 1 == frames:  # --noisy: the plain mix of the last frame's upsampled halves, before the accumulation
                hip.denoise_halves(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), W, H, plain.data_ptr(), plain8.data_ptr(), window_radius=0)
            if frames > 1:
                hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, prev,
                                        two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr())
            torch.cuda.synchronize()
            prev = cam
        hs.check()
    if frames > 1:
        gws = torch.zeros((hip.guided_workspace_bytes(W, H),), dtype=torch.uint8, device="cuda")
        hip.denoise_guided(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H,
                           gws.data_ptr(), rad.data_ptr(), rgb.data_ptr())
    else:
        hip.denoise_halves(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), W, H, rad.data_ptr(), rgb.data_ptr(), window_radius=0)
    torch.cuda.synchronize()
    assert same(read_pfm(pfm), rad.cpu().numpy())
    assert np.array_equal(ppm(out, W, H), rgb.cpu().numpy())
    assert np.array_equal(ppm(noisy, W, H), plain8.cpu().numpy())
    if frames == 1:
        assert same(plain.cpu().numpy(), rad.cpu().numpy())
    else:
        assert not same(plain.cpu().numpy(), rad.cpu().numpy()) and ppm(tmp_path / "h.ppm", W, H).shape == (H, W, 3)
    # --features: full size, the full camera's (of the last frame)
    assert same(read_pfm(f"{feat}.albedo.pfm"), alb.cpu().numpy()) and same(read_pfm(f"{feat}.normal.pfm"), nor.cpu().numpy())
    assert same(read_pfm(f"{feat}.depth.pfm")[..., 0], dep.cpu().numpy()) and read_pfm(f"{feat}.coverage.pfm").shape == (H, W, 3)
