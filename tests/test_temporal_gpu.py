"""Temporal accumulation on the GPU (rbrt_hip_temporal_accumulate) against its numpy restatement (np_temporal.py), bit for bit.

The frozen cases of temporal_cases.py go through temporal_accumulate into buffers full of sentinels: every camera pair; sizes of
one pixel, ragged ones, rows and columns of one pixel, and pixel counts one below, at and one above what a workgroup takes
(RBRT_TEMPORAL_BLOCK: the kernel has no tile), as one row and as one column. A chain of frames alternates two histories, which
is what checks the packed history from frame to frame. Through a handle the halves and features are a render's own, and the
command line is compared with the same library calls made from here."""
from __future__ import annotations

import functools
import json
import re
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import np_temporal as NT
import scenes
import temporal_cases as TC
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
BLOCK = int(re.search(r"#define RBRT_TEMPORAL_BLOCK (\d+)u", (ROOT / "include" / "rbrt_hip_debug.h").read_text()).group(1))

#         W   H
SIZES = [(1, 1), (5, 3), (8, 8), (37, 21), (50, 47), (80, 17), (17, 80),
         (BLOCK - 1, 1), (BLOCK, 1), (BLOCK + 1, 1), (1, BLOCK - 1), (1, BLOCK), (1, BLOCK + 1),   # around a workgroup's pixels
         (BLOCK // 2, 2), (BLOCK // 2 + 1, 2), (2, BLOCK // 2), (3, BLOCK // 2 + 1)]                # ... in two rows and two columns
PARAMS = {"defaults": {}, "M1": dict(max_history=1.0), "M1000": dict(max_history=1000.0), "k0": dict(depth=0.0, normal=0.0)}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def expected(pair, w, h, row="defaults"):
    """The restatement's result for a frozen case: made once, shared, never changed. -> (A', B', len, packed next history, info)"""
    c = TC.case(pair, w, h)
    oa, ob, ln, nxt, info = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, **dict(NT.DEFAULTS, **PARAMS[row]))
    packed = NT.pack(nxt)
    for a in (oa, ob, ln, packed):
        a.flags.writeable = False
    return oa, ob, ln, packed, info


def up(torch, x):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()


def run_temporal(hip, torch, c, hist_packed, p=None, want=("hist", "a", "b", "len"), in_place=False, hist_out=None, cam_prev="case"):
    """One temporal_accumulate call into buffers full of sentinels. hist_packed: a packed history in numpy, a device tensor, or
    None for the first frame. -> namespace(a, b, len, hist: numpy; hist_t: the history written, on the device)"""
    h, w = c.z.shape
    dev = SimpleNamespace(**{k: up(torch, getattr(c, k)) for k in ("A", "B", "N", "z", "c")})
    hin = None if hist_packed is None else hist_packed if torch.is_tensor(hist_packed) else up(torch, hist_packed)
    n_hist = hip.temporal_history_bytes(w, h)
    assert n_hist == w * h * 48
    hout = hist_out if hist_out is not None else torch.full((n_hist,), 0xAB, dtype=torch.uint8, device="cuda")
    assert hout.data_ptr() % 16 == 0 and hout.numel() * hout.element_size() >= n_hist and (hin is None or hin.data_ptr() % 16 == 0)
    oa = dev.A if in_place else torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    ob = dev.B if in_place else torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    ol = torch.full((h, w), -7.0, dtype=torch.float32, device="cuda")
    prev = (c.cam_prev if hin is not None else None) if isinstance(cam_prev, str) else cam_prev
    hip.temporal_accumulate(0, dev.A.data_ptr(), dev.B.data_ptr(), dev.N.data_ptr(), dev.z.data_ptr(), dev.c.data_ptr(), c.cam, prev,
                            hin.data_ptr() if hin is not None else None, hout.data_ptr() if "hist" in want else None,
                            oa.data_ptr() if "a" in want else None, ob.data_ptr() if "b" in want else None,
                            ol.data_ptr() if "len" in want else None, hip.temporal_opts(**(p or {})))
    torch.cuda.synchronize()
    return SimpleNamespace(a=oa.cpu().numpy(), b=ob.cpu().numpy(), len=ol.cpu().numpy(),
                           hist=hout.cpu().numpy()[:n_hist].view(f32).reshape(3, h, w, 4), hist_t=hout)


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


def check_case(hip, pair, w, h, row="defaults"):
    import torch
    c = TC.case(pair, w, h)
    ea, eb, el, eh, _ = expected(pair, w, h, row)
    g = run_temporal(hip, torch, c, NT.pack(c.hist), PARAMS[row])
    assert same(g.a, ea) and same(g.b, eb) and same(g.len, el), (pair, w, h, row, int((bits(g.a) != bits(ea)).sum()), int((bits(g.len) != bits(el)).sum()))
    assert same(g.hist, eh), (pair, w, h, row)


# ---- 1. the frozen cases against the restatement -------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_sizes(hip, w, h):
    check_case(hip, "turn", w, h)
    check_case(hip, "drift_0.2", w, h)


@pytest.mark.parametrize("row", list(PARAMS))
@pytest.mark.parametrize("pair", list(TC.PAIRS))
def test_camera_pairs_and_options(hip, pair, row):
    check_case(hip, pair, 37, 21, row)
    check_case(hip, pair, 50, 47, row)


def test_the_options_matter():
    """(conditions on the inputs) every row of PARAMS gives another result somewhere."""
    base = expected("turn", 50, 47)
    for row in ("M1", "M1000", "k0"):
        other = expected("turn", 50, 47, row)
        assert not same(other[0], base[0]) or not same(other[2], base[2]), row
    assert expected("turn", 50, 47, "M1")[2].max() == 1 and expected("turn", 50, 47, "M1000")[2].max() == 41
    assert 0 < expected("turn", 50, 47, "k0")[4].valid.sum() < base[4].valid.sum()


# ---- 2. outputs, in place, the first frame ----------------------------------------------------------------------------------------
def test_each_output_alone_in_place_and_nothing_asked_for(hip):
    import torch
    pair, w, h = "turn", 50, 47
    c = TC.case(pair, w, h)
    ea, eb, el, eh, _ = expected(pair, w, h)
    packed = NT.pack(c.hist)
    untouched = dict(a=lambda g: np.isnan(g.a).all(), b=lambda g: np.isnan(g.b).all(), len=lambda g: (g.len == -7).all(),
                     hist=lambda g: (g.hist_t == 0xAB).all())
    exp = dict(a=ea, b=eb, len=el, hist=eh)
    for only in ("a", "b", "len", "hist"):
        g = run_temporal(hip, torch, c, packed, want=(only,))
        assert same(getattr(g, only), exp[only]), only
        assert all(check(g) for name, check in untouched.items() if name != only), only
    g = run_temporal(hip, torch, c, packed, want=())  # nothing asked for: nothing written
    assert all(check(g) for check in untouched.values())
    g = run_temporal(hip, torch, c, packed, in_place=True)  # the outputs exactly on d_a and d_b
    assert same(g.a, ea) and same(g.b, eb) and same(g.len, el) and same(g.hist, eh)
    g = run_temporal(hip, torch, c, packed, want=("a", "len"), in_place=True)  # ... and only one of them
    assert same(g.a, ea) and same(g.b, c.B) and same(g.len, el)


@pytest.mark.parametrize("w,h", [(1, 1), (37, 21), (BLOCK + 1, 1), (50, 47)])
def test_the_first_frame_is_the_identity(hip, w, h):
    import torch
    c = TC.case("turn", w, h)
    ea, eb, el, nxt, info = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam)
    assert info is None and same(ea, c.A) and (el == 1).all()
    for prev in (None, c.cam_prev):  # (cam_prev is not read without a history)
        g = run_temporal(hip, torch, c, None, cam_prev=prev)
        assert same(g.a, c.A) and same(g.b, c.B) and (g.len == 1).all() and same(g.hist, NT.pack(nxt))


# ---- 3. a chain of frames over two alternating histories ---------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(37, 21), (50, 47), (BLOCK + 1, 3)])
def test_a_chain_of_three_frames_alternates_two_histories(hip, w, h):
    """Frame 0 has no history; frames 1 and 2 read what the frame before wrote, through the packed history on the device alone.
    The two histories start dirty, and the second round of the chain reuses them as the first left them."""
    import torch
    pairs = ("static", "drift_0.2", "turn")   # frame k is the case's K' for k = 0 and K after, so the cameras differ
    cams = [TC.camera(w, h, **TC.PAIRS["turn"]), TC.camera(w, h, **TC.PAIRS["drift_0.2"]), TC.camera(w, h)]
    rng = np.random.default_rng(w * 100 + h)
    frames = []
    for k, cam in enumerate(cams):
        N, z, c = TC.features(cam)
        t = TC.truth(N, c)
        frames.append(SimpleNamespace(A=TC.noisy(t, rng), B=TC.noisy(t, rng), N=N, z=z, c=c, cam=cam, cam_prev=cams[k - 1] if k else None))
    hist, exp = None, []
    for fr in frames:
        oa, ob, ln, hist, info = NT.accumulate(fr.A, fr.B, fr.N, fr.z, fr.c, fr.cam, fr.cam_prev, hist, **NT.DEFAULTS)
        exp.append((oa, ob, ln, NT.pack(hist), info))
    assert exp[2][4].valid.any() and not exp[2][4].valid.all() and exp[2][2].max() > 2  # the third frame has histories of length 2
    n_hist = hip.temporal_history_bytes(w, h)
    two = [torch.full((n_hist,), v, dtype=torch.uint8, device="cuda") for v in (0xAB, 0x7F)]
    for round_ in range(2):  # (the second round: the workspace reused dirty)
        hin = None
        for k, fr in enumerate(frames):
            g = run_temporal(hip, torch, fr, hin, hist_out=two[k & 1])
            hin = two[k & 1].view(torch.float32)
            oa, ob, ln, packed, _ = exp[k]
            assert same(g.a, oa) and same(g.b, ob) and same(g.len, ln) and same(g.hist, packed), (round_, k)


# ---- 4. NaN and infinities ---------------------------------------------------------------------------------------------------------------
def test_non_finite_inputs_stay_within_their_taps_reach(hip):
    """A NaN and an infinity planted in this frame's features and in every field of the history: the run ends without a fault,
    and the pixels out of the planted values' reach -- the planted pixels themselves for the features, the pixels whose four taps
    touch a planted history pixel for the history -- hold the bits of the run without them."""
    import torch
    pair, w, h = "turn", 50, 47
    c = TC.case(pair, w, h)
    ea, eb, el, eh, info = expected(pair, w, h)
    nan, inf = f32(np.nan), f32(np.inf)
    feat = {(5, 7): ("N", nan), (20, 30): ("z", inf), (21, 31): ("z", nan), (40, 10): ("c", nan), (41, 11): ("c", inf), (30, 5): ("N", -inf)}
    planted = SimpleNamespace(**{k: getattr(c, k).copy() for k in ("A", "B", "N", "z", "c")}, cam=c.cam, cam_prev=c.cam_prev)
    reached = np.zeros((h, w), bool)
    for (y, x), (name, v) in feat.items():
        getattr(planted, name)[y, x] = v
        reached[y, x] = True
    hist = NT.History(*(getattr(c.hist, k).copy() for k in ("a", "b", "length", "n", "z", "c")))
    bad = np.zeros((h, w), bool)
    for (y, x), (name, v) in {(10, 10): ("a", nan), (12, 25): ("b", inf), (25, 12): ("length", nan), (33, 40): ("n", nan), (8, 44): ("z", inf),
                              (44, 8): ("c", nan), (15, 15): ("length", inf), (36, 22): ("z", nan), (2, 2): ("c", inf)}.items():
        getattr(hist, name)[y, x] = v
        bad[y, x] = True
    for dj, di in ((0, 0), (0, 1), (1, 0), (1, 1)):
        qy, qx = info.j + dj, info.i + di
        ins = info.projects & (qy >= 0) & (qy < h) & (qx >= 0) & (qx < w)
        reached |= ins & bad[np.where(ins, qy, 0), np.where(ins, qx, 0)]
    assert 15 <= reached.sum() <= 60 and (~reached).sum() > 2000
    g = run_temporal(hip, torch, planted, NT.pack(hist))
    keep = ~reached
    assert same(g.a[keep], ea[keep]) and same(g.b[keep], eb[keep]) and same(g.len[keep], el[keep])
    assert same(g.hist[:, keep], eh[:, keep])
    # ... and a history that is nothing but NaN, or nothing but infinities: every pixel passes through or holds something, no fault
    for v in (nan, inf, -inf):
        full = np.full((3, h, w, 4), v, f32)
        g = run_temporal(hip, torch, c, full)
        assert (g.len != -7).all()


# ---- 5. through a handle --------------------------------------------------------------------------------------------------------------------
def test_a_handle_accumulates_its_renders_and_renders_on_as_before(hip, oracle):
    """render_adaptive (one round), its halves, render_features and temporal_accumulate over three seeds and a drifting camera
    equal the restatement fed the same halves and features; the handle's later renders are what they were."""
    import torch
    w, h, n, fs = 45, 27, 6, 3
    sc = scenes.spheres_scene()
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    n_hist = hip.temporal_history_bytes(w, h)
    two = [torch.full((n_hist,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(2)]
    with hip.HipScene(sc) as hs:
        cam0 = scenes.camera(oracle, w, h)
        before = new(h, w, 3)
        hs.render_device(cam0, abi.default_opts(spp=4, seed=9), before.data_ptr())
        hist, prev, seen = None, None, []
        for k in range(3):
            cam = scenes.camera(oracle, w, h, position=(0.05 * k, 5.0, 4.0))
            o = abi.default_opts(spp=n, seed=11 + k)
            rad, ha, hb, alb, nor, dep, cov = new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w), new(h, w)
            assert hs.render_adaptive(cam, o, 0.0, n, n, rad.data_ptr())["rounds"] == 1
            hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
            hs.render_features(cam, o, fs, alb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
            torch.cuda.synchronize()
            A, B, N, z, c = (t.cpu().numpy() for t in (ha, hb, nor, dep, cov))
            oa, ob, ol = new(h, w, 3), new(h, w, 3), new(h, w)
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, prev,
                                    two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), oa.data_ptr(), ob.data_ptr(), ol.data_ptr())
            torch.cuda.synchronize()
            ea, eb, el, hist, info = NT.accumulate(A, B, N, z, c, cam, prev, hist, **NT.DEFAULTS)
            assert same(oa.cpu().numpy(), ea) and same(ob.cpu().numpy(), eb) and same(ol.cpu().numpy(), el), k
            assert same(two[k & 1].cpu().numpy().view(f32).reshape(3, h, w, 4), NT.pack(hist)), k
            if info is not None:
                seen.append(float(info.valid.mean()))
                assert not same(ea, A)
            prev = cam
        assert all(0.5 < s <= 1.0 for s in seen) and el.max() == 3, (seen, el.max())
        after = new(h, w, 3)
        hs.render_device(cam0, abi.default_opts(spp=4, seed=9), after.data_ptr())
        torch.cuda.synchronize()
        assert same(after.cpu().numpy(), before.cpu().numpy())
        hs.check()


# ---- 6. refusals with device pointers ---------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip):
    import torch
    c = TC.case("turn", 37, 21)
    packed = up(torch, NT.pack(c.hist))
    g = None
    for kw in (dict(p=dict(max_history=0.5)), dict(p=dict(depth=-1.0)), dict(p=dict(flags=1)), dict(p=dict(reserved=(0, 0, 0, 1))),
               dict(cam_prev=None), dict(cam_prev=TC.camera(36, 21)), dict(hist_out=packed.view(torch.uint8))):
        with pytest.raises(abi.RbrtError) as e:
            g = run_temporal(hip, torch, c, packed, **kw)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG, kw
    assert g is None and same(packed.cpu().numpy(), NT.pack(c.hist))
    t = hip.temporal_opts()
    assert (t.max_history, t.depth, t.normal, t.flags, list(t.reserved)) == (f32(32), f32(0.05), f32(0.35), 0, [0, 0, 0, 0])
    assert BLOCK == abi.TEMPORAL_BLOCK and BLOCK % 64 == 0


# ---- 7. the command line --------------------------------------------------------------------------------------------------------------
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


def test_cli_frames_equal_the_library_calls(hip, tmp_path):
    """--frames 3 --camera-step 0.01,0,0 --radiance out.pfm equals what the same library calls give from here; --history-map
    and the report's temporal_ms exist."""
    import torch
    w, h, n, fs, frames, step, seed = 64, 48, 6, 3, 3, 0.01, 3
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    out, pfm, hmap, rep = tmp_path / "a.ppm", tmp_path / "out.pfm", tmp_path / "h.ppm", tmp_path / "rep.json"
    r = subprocess.run([str(EXE), "-c", str(cfg), "--height", str(h), "-w", str(w), "-s", str(n), "--seed", str(seed), "--background", "0,0,0",
                        "--feature-samples", str(fs), "--frames", str(frames), "--camera-step", f"{step},0,0", "--radiance", str(pfm),
                        "--history-map", str(hmap), "--report", str(rep), "-t", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(rep.read_text())
    assert js["frames"] == frames and 0.0 < js["temporal_ms"] < 1000.0 and js["temporal_max_history"] == 32
    assert js["camera_step"] == pytest.approx([step, 0, 0], rel=1e-6) and "denoise_ms" not in js and "guided_ms" not in js
    hsn = abi.HostScene(cfg, h, w)
    assert hsn.lens is None
    new = lambda *shape: torch.zeros(shape, dtype=torch.float32, device="cuda")
    ha, hb, nor, dep, cov, ol, rad = new(h, w, 3), new(h, w, 3), new(h, w, 3), new(h, w), new(h, w), new(h, w), new(h, w, 3)
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    two = [torch.zeros((hip.temporal_history_bytes(w, h),), dtype=torch.uint8, device="cuda") for _ in range(2)]
    with hip.HipScene(hsn) as hs:
        prev = None
        for k in range(frames):
            cam = type(hsn.camera).from_buffer_copy(hsn.camera)
            shift = f32(k) * f32(step)
            cam.position[0] = f32(hsn.camera.position[0]) + shift
            cam.img_center_point[0] = f32(hsn.camera.img_center_point[0]) + shift
            o = abi.default_opts(spp=n, seed=seed + k, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
            assert hs.render_adaptive(cam, o, 0.0, n, n)["rounds"] == 1
            hs.denoise(None, None, ha.data_ptr(), hb.data_ptr())
            hs.render_features(cam, o, fs, None, nor.data_ptr(), dep.data_ptr(), cov.data_ptr())
            hip.temporal_accumulate(0, ha.data_ptr(), hb.data_ptr(), nor.data_ptr(), dep.data_ptr(), cov.data_ptr(), cam, prev,
                                    two[(k - 1) & 1].data_ptr() if k else None, two[k & 1].data_ptr(), ha.data_ptr(), hb.data_ptr(), ol.data_ptr())
            torch.cuda.synchronize()
            prev = cam
        hs.check()
    wa = torch.full((h, w), float(f32((n + 1) // 2) * (f32(1) / f32(n))), dtype=torch.float32, device="cuda")
    hip.denoise_halves(0, ha.data_ptr(), hb.data_ptr(), wa.data_ptr(), w, h, rad.data_ptr(), rgb.data_ptr(), window_radius=0)
    torch.cuda.synchronize()
    assert same(read_pfm(pfm), rad.cpu().numpy())
    assert np.array_equal(ppm(out, w, h), rgb.cpu().numpy())
    length = ol.cpu().numpy()
    assert length.max() == 3 and length.min() >= 1
    grey = ppm(hmap, w, h)
    assert np.array_equal(grey[..., 0], ((length / f32(32)) * f32(255)).astype(np.uint8)) and (grey[..., 0] == grey[..., 2]).all()
