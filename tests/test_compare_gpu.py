"""Image comparison on the GPU (rbrt_hip_compare_images) against its numpy restatement (np_compare.py), bit for bit: the 64
bytes of the result and both maps.

The frozen cases of compare_cases.py go through compare_images into buffers full of sentinels: one pixel, one row, one column,
sizes one below, at and one above the tile of 16 x 16, a size whose interior workgroup has halos on all four sides, and sizes of
289 and 513 tiles, where the reduce kernel's lanes take a second and a third tile. Through a handle the images are a render and
its guided-denoised version, and the command line is compared with the restatement on the files it wrote."""
from __future__ import annotations

import ctypes as C
import functools
import json
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import compare_cases as CC
import np_compare as NC
import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
DIRTY = 0xCD  # what the workspace and the result buffer hold before a call


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


@functools.lru_cache(maxsize=None)
def expected(w, h, kind="mixed", epsilon=0.01):
    """The restatement's result for a frozen case: made once, shared, never changed."""
    c = CC.case(w, h, kind)
    e = NC.compare(c.x, c.r, epsilon)
    for a in (e.rel_map, e.ssim_map):
        a.flags.writeable = False
    return e


def run_compare(hip, torch, x, r, epsilon=None, want=("rel", "ssim", "result"), offset=0, one_pointer=False, dirty=DIRTY, stream=None):
    """One compare_images call into buffers full of sentinels; with `offset` both images start that many bytes (a multiple of 4)
    into their allocations. -> namespace(rel, ssim: numpy [H, W]; result: the 64 bytes; ...)"""
    H, W, _ = x.shape

    def image(src):
        t = torch.full((H * W * 3 + offset // 4,), float("nan"), dtype=torch.float32, device="cuda")
        t[offset // 4:] = torch.from_numpy(np.ascontiguousarray(src).reshape(-1).copy()).cuda()
        return t

    dx = image(x)
    dr = dx if one_pointer else image(r)
    rel = torch.full((H * W + 1,), -7.0, dtype=torch.float32, device="cuda")
    ssim = torch.full((H * W + 1,), -7.0, dtype=torch.float32, device="cuda")
    nws = hip.compare_workspace_bytes(W, H)
    assert nws == 48 * (-(-W // CC.TW)) * (-(-H // CC.TH))
    ws = torch.full((nws + 8,), dirty, dtype=torch.uint8, device="cuda")
    res = torch.full((64 + 8,), dirty, dtype=torch.uint8, device="cuda")
    hip.compare_images(0, dx.data_ptr() + offset, dr.data_ptr() + offset, W, H, ws.data_ptr() if "result" in want else None,
                       rel.data_ptr() if "rel" in want else None, ssim.data_ptr() if "ssim" in want else None,
                       res.data_ptr() if "result" in want else None, hip.compare_opts(epsilon=epsilon), stream)
    torch.cuda.synchronize()
    rel_all, ssim_all, res_all, ws_all = rel.cpu().numpy(), ssim.cpu().numpy(), res.cpu().numpy(), ws.cpu().numpy()
    return SimpleNamespace(rel=rel_all[:H * W].reshape(H, W), ssim=ssim_all[:H * W].reshape(H, W), result=res_all[:64].tobytes(), rel_all=rel_all,
                           ssim_all=ssim_all, res_all=res_all, ws_all=ws_all)


def check(g, e, what=""):
    assert g.result == e.result, (what, abi.CompareResult.from_buffer_copy(g.result).sum_ssim, e.sum_ssim, g.result.hex(), e.result.hex())
    assert same(g.rel, e.rel_map) and same(g.ssim, e.ssim_map), (what, int((bits(g.rel) != bits(e.rel_map)).sum()), int((bits(g.ssim) != bits(e.ssim_map)).sum()))
    # nothing behind the buffers' ends was written
    assert g.rel_all[-1] == -7.0 and g.ssim_all[-1] == -7.0 and (g.res_all[64:] == g.res_all[-1]).all() and (g.ws_all[-8:] == g.ws_all[-1]).all(), what


# ---- 1. sizes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", CC.SIZES + CC.MANY_TILES, ids=[f"{w}x{h}" for w, h in CC.SIZES + CC.MANY_TILES])
def test_sizes(hip, w, h):
    import torch
    c = CC.case(w, h)
    check(run_compare(hip, torch, c.x, c.r), expected(w, h), (w, h))


def test_the_cases_hold_what_they_should():
    """(conditions on the inputs) the main case has unusable pixels as centres and within the window's reach of a tile's edge, in
    X and in R, and negative channels; the sizes with many tiles make the reduce kernel's lanes wrap once and twice."""
    w, h = CC.MAIN
    c, e = CC.case(w, h), expected(w, h)
    assert e.skipped == int(c.bad.sum()) > 20 and e.usable + e.skipped == w * h
    assert c.bad[:, CC.TW - 1].any() and c.bad[:, CC.TW].any() and c.bad[CC.TH - 1].any() and c.bad[CC.TH].any()
    assert c.bad[:, CC.TW + 4].any() and c.bad[:, CC.TW + 5].any() and c.bad[:, CC.TW - 5].any() and c.bad[:, CC.TW - 6].any()
    assert (~np.isfinite(c.x)).any() and (~np.isfinite(c.r)).any() and (c.x[np.isfinite(c.x)] < 0).any() and (c.r[np.isfinite(c.r)] < 0).any()
    assert (e.rel_map[c.bad] == 0).all() and not np.signbit(e.rel_map[c.bad]).any() and np.isfinite(e.ssim_map).all()
    assert all(np.isfinite(v) for v in (e.sum_se, e.sum_ae, e.sum_rel, e.sum_ssim))
    tiles = [(-(-w // CC.TW)) * (-(-h // CC.TH)) for w, h in CC.MANY_TILES]
    assert 256 < tiles[0] <= 512 < tiles[1]
    assert (3 * CC.TW < 49 < 4 * CC.TW) and (3 * CC.TH < 50 < 4 * CC.TH) and (49, 50) in CC.SIZES


# ---- 2. inputs at the main size ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("one_pointer", [False, True])
def test_an_image_against_itself(hip, one_pointer):
    import torch
    w, h = CC.MAIN
    c = CC.case(w, h, "clean")
    g = run_compare(hip, torch, c.x, c.x.copy(), one_pointer=one_pointer)
    r = abi.CompareResult.from_buffer_copy(g.result)
    assert (r.sum_se, r.sum_ae, r.sum_rel, r.max_abs, r.usable, r.skipped, list(r.reserved)) == (0.0, 0.0, 0.0, 0.0, w * h, 0, [0] * 5)
    assert r.sum_ssim == float(w * h) and (g.ssim == f32(1)).all() and (g.rel == 0).all()
    check(g, NC.compare(c.x, c.x))
    # ... and with what is not finite in it: skipped, and still 1 everywhere
    m = CC.case(w, h, "mixed")
    g = run_compare(hip, torch, m.x, m.x.copy(), one_pointer=one_pointer)
    r = abi.CompareResult.from_buffer_copy(g.result)
    assert (r.sum_se, r.max_abs, r.sum_ssim) == (0.0, 0.0, float(w * h)) and r.skipped > 0 and (g.ssim == f32(1)).all()
    check(g, NC.compare(m.x, m.x))


def test_a_square_that_overflows_is_not_hidden(hip):
    import torch
    w, h = CC.MAIN
    c, e = CC.case(w, h, "overflow"), expected(w, h, "overflow")
    g = run_compare(hip, torch, c.x, c.r)
    check(g, e)
    assert e.sum_se == np.inf and e.sum_rel == np.inf and np.isfinite(e.sum_ae) and e.max_abs == f32(1e25) and e.skipped == 0
    assert np.isinf(g.rel).sum() == 1


@pytest.mark.parametrize("epsilon", [1e-6, 100.0])
def test_epsilon(hip, epsilon):
    import torch
    w, h = CC.MAIN
    c, e = CC.case(w, h), expected(w, h, "mixed", epsilon)
    check(run_compare(hip, torch, c.x, c.r, epsilon), e)
    d = expected(w, h)
    assert e.sum_rel != d.sum_rel and e.result[:16] == d.result[:16] and e.result[24:] == d.result[24:]  # only rel reads epsilon


# ---- 3. outputs, dirty buffers, alignment --------------------------------------------------------------------------------------------
def test_each_output_alone_and_nothing_asked_for(hip):
    import torch
    w, h = CC.MAIN
    c, e = CC.case(w, h), expected(w, h)
    untouched = dict(rel=lambda g: (g.rel_all == -7.0).all(), ssim=lambda g: (g.ssim_all == -7.0).all(),
                     result=lambda g: (g.res_all == DIRTY).all() and (g.ws_all == DIRTY).all())
    right = dict(rel=lambda g: same(g.rel, e.rel_map) and g.rel_all[-1] == -7.0, ssim=lambda g: same(g.ssim, e.ssim_map) and g.ssim_all[-1] == -7.0,
                 result=lambda g: g.result == e.result and (g.res_all[64:] == DIRTY).all())
    for only in ("rel", "ssim", "result"):
        g = run_compare(hip, torch, c.x, c.r, want=(only,))
        assert right[only](g), only
        assert all(ok(g) for name, ok in untouched.items() if name != only), only
    g = run_compare(hip, torch, c.x, c.r, want=())  # nothing asked for: nothing launched
    assert all(ok(g) for ok in untouched.values())


@pytest.mark.parametrize("dirty", [0x00, 0xFF, 0x7F])
def test_a_dirty_workspace_and_result_do_not_matter(hip, dirty):
    """0xFF bytes are NaN as doubles and floats and the largest count; 0x7F7F... is a huge finite double."""
    import torch
    for w, h in (CC.MAIN, (1, 1)):
        c = CC.case(w, h)
        check(run_compare(hip, torch, c.x, c.r, dirty=dirty), expected(w, h), (w, h, dirty))


def test_images_offset_by_one_float(hip):
    import torch
    for w, h in (CC.MAIN, (3, 3)):
        c = CC.case(w, h)
        check(run_compare(hip, torch, c.x, c.r, offset=4), expected(w, h), (w, h))


def test_two_calls_on_one_stream_and_a_third_on_another_give_equal_bytes(hip):
    import torch
    w, h = CC.MANY_TILES[0]
    c, e = CC.case(w, h), expected(w, h)
    other = torch.cuda.Stream()
    a = run_compare(hip, torch, c.x, c.r)
    b = run_compare(hip, torch, c.x, c.r)
    with torch.cuda.stream(other):
        t = run_compare(hip, torch, c.x, c.r, stream=other.cuda_stream)
    for g in (a, b, t):
        check(g, e)
    assert a.result == b.result == t.result and same(a.ssim, t.ssim) and same(a.rel, b.rel)


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip):
    import torch
    w, h = 5, 3
    x = torch.full((w * h * 3,), 2.0, dtype=torch.float32, device="cuda")
    r = torch.full((w * h * 3,), 3.0, dtype=torch.float32, device="cuda")
    m1 = torch.full((w * h,), -7.0, dtype=torch.float32, device="cuda")
    m2 = torch.full((w * h,), -7.0, dtype=torch.float32, device="cuda")
    ws = torch.full((hip.compare_workspace_bytes(w, h) + 8,), DIRTY, dtype=torch.uint8, device="cuda")
    res = torch.full((64 + 8,), DIRTY, dtype=torch.uint8, device="cuda")
    ok = dict(d_x=x.data_ptr(), d_ref=r.data_ptr(), width=w, height=h, d_workspace=ws.data_ptr(), d_rel_map=m1.data_ptr(), d_ssim_map=m2.data_ptr(),
              d_result=res.data_ptr())
    nan, inf = float("nan"), float("inf")
    O = hip.compare_opts
    rows = [dict(d_x=0), dict(d_ref=0), dict(d_workspace=0), dict(width=0), dict(height=0), dict(d_workspace=ws.data_ptr() + 4), dict(d_result=res.data_ptr() + 4),
            dict(opts=O(epsilon=0.0)), dict(opts=O(epsilon=-0.01)), dict(opts=O(epsilon=nan)), dict(opts=O(epsilon=inf)), dict(opts=O(flags=1)),
            dict(opts=O(reserved=(1, 0))), dict(opts=O(reserved=(0, 1))),
            dict(d_rel_map=x.data_ptr()), dict(d_rel_map=r.data_ptr()), dict(d_ssim_map=x.data_ptr()), dict(d_ssim_map=r.data_ptr()),
            dict(d_result=x.data_ptr()), dict(d_result=r.data_ptr()), dict(d_workspace=x.data_ptr()), dict(d_workspace=r.data_ptr()),
            dict(d_ssim_map=m1.data_ptr()), dict(d_result=m1.data_ptr()), dict(d_result=m2.data_ptr()), dict(d_workspace=m1.data_ptr()),
            dict(d_workspace=res.data_ptr())]
    for kw in rows:
        with pytest.raises(abi.RbrtError) as e:
            hip.compare_images(0, **dict(ok, **kw))
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG, kw
    with pytest.raises(abi.RbrtError) as e:
        hip.compare_images(0, **dict(ok, width=1 << 16, height=1 << 15))
    assert e.value.code == abi.RBRT_ERR_UNSUPPORTED
    assert hip.compare_workspace_bytes(1 << 16, 1 << 15) == 0 and hip.compare_workspace_bytes(0, 4) == 0
    torch.cuda.synchronize()
    assert bool((x == 2.0).all()) and bool((r == 3.0).all()) and bool((m1 == -7.0).all()) and bool((m2 == -7.0).all())
    assert bool((ws == DIRTY).all()) and bool((res == DIRTY).all())
    hip.compare_images(0, **ok)  # and the same arguments unchanged are taken
    torch.cuda.synchronize()
    assert res.cpu().numpy()[:64].tobytes() == NC.compare(np.full((h, w, 3), 2.0, f32), np.full((h, w, 3), 3.0, f32)).result


# ---- 5. through a handle -------------------------------------------------------------------------------------------------------------
def test_a_render_against_its_guided_denoised_image(hip, oracle):
    """A 64 x 48 render of the example spheres at 4 samples and what the guided filter makes of it: the stage on the two device
    images equals the restatement on the arrays read back, either way round."""
    import torch
    W, H, n = 64, 48, 4
    sc = scenes.spheres_scene(scenes.EXAMPLE_SPHERES)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    cam = scenes.camera(oracle, W, H)
    with hip.HipScene(sc) as hs:
        o = abi.default_opts(spp=n, seed=5)
        rad, ha, hb, out = new(H, W, 3), new(H, W, 3), new(H, W, 3), new(H, W, 3)
        alb, nor, dep, cov = new(H, W, 3), new(H, W, 3), new(H, W), new(H, W)
        assert hs.render_adaptive(cam, o, 0.0, n, n, rad.data_ptr())["rounds"] == 1
        hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
        hs.render_features(cam, o, 2, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
        ws = torch.zeros((hip.guided_workspace_bytes(W, H),), dtype=torch.uint8, device="cuda")
        hip.denoise_guided(0, ha.data_ptr(), hb.data_ptr(), None, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), W, H, ws.data_ptr(),
                           out.data_ptr())
        cws = torch.full((hip.compare_workspace_bytes(W, H),), DIRTY, dtype=torch.uint8, device="cuda")
        rel, ssim = new(H, W), new(H, W)
        res = torch.full((64,), DIRTY, dtype=torch.uint8, device="cuda")
        noisy, clean = rad.cpu().numpy(), None
        for dx, dr in ((out, rad), (rad, out)):
            hip.compare_images(0, dx.data_ptr(), dr.data_ptr(), W, H, cws.data_ptr(), rel.data_ptr(), ssim.data_ptr(), res.data_ptr())
            torch.cuda.synchronize()
            clean = out.cpu().numpy()
            e = NC.compare(dx.cpu().numpy(), dr.cpu().numpy())
            assert res.cpu().numpy().tobytes() == e.result and same(rel.cpu().numpy(), e.rel_map) and same(ssim.cpu().numpy(), e.ssim_map)
            assert e.skipped == 0 and e.sum_se > 0 and 0.0 < e.sum_ssim < W * H
        assert np.isfinite(noisy).all() and np.isfinite(clean).all() and not same(noisy, clean)
        hs.check()


# ---- 6. the command line ---------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    """A colour PFM in numpy: float32 (H, W, 3), top row first."""
    raw = Path(path).read_bytes()
    magic, size, scale, body = raw.split(b"\n", 3)
    assert magic == b"PF" and float(scale) < 0  # colour, little-endian
    w, h = (int(x) for x in size.split())
    assert len(body) == w * h * 12
    return np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1].copy()


def read_grey_pfm(path):
    """A map's PFM: three equal channels -> float32 (H, W)."""
    a = read_pfm(path)
    assert same(a[..., 0], a[..., 1]) and same(a[..., 0], a[..., 2])
    return a[..., 0].copy()


def rbrt(*argv):
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    r = subprocess.run([str(EXE), "-c", str(cfg), "--height", "48", "-w", "64", "-s", "4", *map(str, argv)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return r


def pgm(p, w, h):
    """The grey image a .ppm target holds: three equal channels."""
    raw = Path(p).read_bytes()
    head = f"P6\n{w} {h}\n255\n".encode()
    assert raw.startswith(head)
    a = np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)
    assert (a[..., 0] == a[..., 1]).all() and (a[..., 0] == a[..., 2]).all()
    return a[..., 0]


def test_cli_compare(hip, tmp_path):
    W, H = 64, 48
    ref, rep, out = tmp_path / "ref.pfm", tmp_path / "rep.json", tmp_path / "x.ppm"
    rbrt("--seed", 1, "--radiance", ref, "-t", out)
    # the same frame against itself
    r = rbrt("--seed", 1, "--compare", ref, "--report", rep, "-t", out)
    js = json.loads(rep.read_text())
    assert (js["compare_mse"], js["compare_mae"], js["compare_relmse"], js["compare_ssim"], js["compare_max_abs"]) == (0, 0, 0, 1, 0)
    assert (js["compare_skipped"], js["compare_usable"], js["compare_file"]) == (0, W * H, str(ref)) and 0.0 < js["compare_ms"] < 1000.0
    assert js["compare_psnr_db"] == "inf"  # (what is not finite is a string)
    assert "compare" in r.stdout and "ssim" in r.stdout.lower()
    # another seed: every number is the restatement's on the two files
    xp, em, sm, em8, sm8 = tmp_path / "x.pfm", tmp_path / "err.pfm", tmp_path / "ssim.pfm", tmp_path / "err.ppm", tmp_path / "ssim.ppm"
    rbrt("--seed", 2, "--compare", ref, "--compare-epsilon", 0.5, "--error-map", em, "--ssim-map", sm, "--radiance", xp, "--report", rep, "-t", out)
    js = json.loads(rep.read_text())
    X, R = read_pfm(xp), read_pfm(ref)
    e = NC.compare(X, R, 0.5)
    s = NC.summary(e, W, H, 1.0)
    assert e.sum_se > 0 and e.skipped == 0
    for k in ("mse", "mae", "relmse", "psnr_db", "ssim"):
        assert js[f"compare_{k}"] == s[k], (k, js[f"compare_{k}"], s[k])  # (%.17g round-trips a double)
    assert (js["compare_max_abs"], js["compare_usable"], js["compare_skipped"], js["compare_epsilon"]) == (float(e.max_abs), W * H, 0, 0.5)
    assert same(read_grey_pfm(em), e.rel_map) and same(read_grey_pfm(sm), e.ssim_map)
    # 8-bit maps: the documented scaling
    rbrt("--seed", 2, "--compare", ref, "--compare-epsilon", 0.5, "--error-map", em8, "--ssim-map", sm8, "-t", out)
    assert np.array_equal(pgm(em8, W, H), NC.grey8(e.rel_map, 0.0, 1.0)) and np.array_equal(pgm(sm8, W, H), NC.grey8(e.ssim_map, 0.0, 1.0))
    # the last of two frames, and an upscaled frame: the reference's size is the image's
    for extra in (["--frames", 2], ["--upscale", 2], ["--gpus", 1, "--denoise"]):
        rbrt("--seed", 1, *extra, "--compare", ref, "--radiance", xp, "--report", rep, "-t", out)
        js = json.loads(rep.read_text())
        e = NC.compare(read_pfm(xp), R)
        s = NC.summary(e, W, H, 1.0)
        assert js["compare_usable"] + js["compare_skipped"] == W * H and js["compare_mse"] == s["mse"] > 0 and js["compare_ssim"] == s["ssim"], extra
        assert js["compare_relmse"] == s["relmse"] and f32(js["compare_epsilon"]) == f32(0.01) and js["compare_skipped"] == e.skipped == 0, extra  # (the default epsilon)
