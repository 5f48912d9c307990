"""The display transform on the GPU (rbrt_hip_tonemap) against its numpy restatement (np_tonemap.py), bit for bit: the float
output, the rgb8 output and the workspace (the 4096 histogram words and the result struct). NaN pixels are compared as
NaN-ness; there is no tolerance anywhere.

Sizes around the kernels' group of four pixels, around a wave, around the pixels one workgroup takes per stride
(RBRT_TONEMAP_BLOCK_PIXELS, B) and around the capped grid's reach (RBRT_TONEMAP_MAX_BLOCKS, G): from G * B + 1 pixels on a
workgroup strides a second time. Contents (a) to (e) are described at `content`."""
from __future__ import annotations

import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

import np_tonemap as N
import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32, u32 = np.float32, np.uint32
_dbg = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
B = int(re.search(r"#define RBRT_TONEMAP_BLOCK_PIXELS (\d+)u", _dbg).group(1))
G = int(re.search(r"#define RBRT_TONEMAP_MAX_BLOCKS (\d+)u", _dbg).group(1))
assert G * B <= 4 << 20, "lower the grid cap rather than growing the test"
SIZES = [1, 3, 4, 5, 63, 64, 65, B - 1, B, B + 1, 3 * B + 1, G * B - 1, G * B + 1, 2 * G * B + 5]
CONTENTS = ["a_log_uniform", "b_flat", "c_nothing_counted", "d_bin_edges", "e_rank_at_a_lane_boundary"]
CURVES = [N.LINEAR, N.REINHARD, N.ACES]
LANE_LAST, LANE_FIRST = 31 * 64 + 63, 32 * 64  # bins 2047 and 2048: the last of lane 31's 64 and the first of lane 32's


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def from_bits(u):
    return np.array([u], u32).view(f32)[0]


def pixel_with_luminance(target_bits: int) -> np.ndarray:
    """A pixel whose luminance has exactly these bits (a positive float). Starts from the grey of that value and moves the
    green and, if green's steps jump over the target, the blue component by single steps."""
    t = from_bits(target_bits)
    v = min(t, np.finfo(f32).max)

    def lum(p):
        return N.luminance(np.array(p, f32))

    for db in range(0, 200):
        for sign in ((1,) if db == 0 else (1, -1)):
            b = from_bits(int(bits([v])[0]) + sign * db) if 0 < int(bits([v])[0]) + sign * db <= 0x7F7FFFFF else v
            lo, hi = 0, 0x7F7FFFFF  # the smallest green whose luminance reaches t (the luminance does not fall as green grows)
            while lo < hi:
                mid = (lo + hi) // 2
                y = lum([v, from_bits(mid), b])
                if y >= t:  # (inf included)
                    hi = mid
                else:
                    lo = mid + 1
            p = np.array([v, from_bits(lo), b], f32)
            if int(bits([lum(p)])[0]) == target_bits:
                return p
    raise AssertionError(f"no pixel found for luminance bits {target_bits:#x}")


@functools.lru_cache(maxsize=None)
def edge_pixels() -> np.ndarray:
    """(d): luminances on both edges of bins -- the low 19 bits all 0 and all 1 -- in bins low, middle and high (15 is the last
    bin of the denormals, which are not counted), next to a lane boundary of the select kernel, and the two ends of what is counted: the smallest normal float and FLT_MAX."""
    targets = [0x00800000, 0x7F7FFFFF]
    for b in (15, 16, 17, 63, 64, 65, 1000, LANE_LAST, LANE_FIRST, 2100, 4000, 4078, 4079):
        targets += [b << 19, (b << 19) | 0x7FFFF]
    px = np.stack([pixel_with_luminance(t) for t in targets])
    assert np.array_equal(bits(N.luminance(px)), np.array(targets, u32))  # a condition on the inputs
    px.flags.writeable = False
    return px


def in_bin(b: int, n: int, rng) -> np.ndarray:
    """n green pixels whose luminances lie in bin b, away from its edges."""
    lo, hi = from_bits((b << 19) + 0x10000), from_bits((b << 19) + 0x70000)
    y = rng.uniform(lo, hi, n).astype(f32)
    px = np.zeros((n, 3), f32)
    px[:, 1] = y / f32(0.7152)
    return px


@functools.lru_cache(maxsize=None)
def content(kind: str, n: int) -> np.ndarray:
    """n pixels, made once, shared, never changed.
    (a) luminances log-uniform over 2^-20 .. 2^20 with random chroma, one pixel in 7 zero
    (b) every pixel equal: one bin, the contended case
    (c) nothing counted: +0, -0, denormals, negatives, +-inf and NaN
    (d) edge_pixels(), repeated
    (e) with M = n: exactly k_500 + 1 pixels in bins up to 2047, the last bin of lane 31 of the select kernel, at least one of
        them in 2047 itself, and the rest in bin 2048, the first of lane 32: rank k_500 is the last pixel of the one lane and
        rank k_990 (n >= 4) a pixel of the next lane's first bin"""
    rng = np.random.default_rng(7919 * CONTENTS.index(kind) + n)
    if kind == "a_log_uniform":
        chroma = rng.uniform(0.05, 1.0, (n, 3)).astype(f32)
        target = (2.0 ** rng.uniform(-20.0, 20.0, n)).astype(f32)
        x = (chroma * (target / N.luminance(chroma))[:, None]).astype(f32)
        x[rng.integers(0, 7, n) == 0] = 0
    elif kind == "b_flat":
        x = np.tile(np.array([0.25, 0.5, 0.125], f32), (n, 1))
    elif kind == "c_nothing_counted":
        tiny = np.finfo(f32).tiny
        rows = np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [1e-42, 3e-43, 0], [tiny / 4, tiny / 4, tiny / 4], [-1, -2, -3], [-1e30, 0, 1],
                         [np.inf, 1, 1], [-np.inf, 1, 1], [np.nan, 1, 1], [np.inf, -np.inf, 0], [0, np.nan, -np.inf]], f32)
        x = rows[rng.integers(0, len(rows), n)]
    elif kind == "d_bin_edges":
        e = edge_pixels()
        x = e[(np.arange(n) + n) % len(e)] if n < len(e) else e[rng.permutation(np.arange(n) % len(e))]
    else:
        k500 = ((n - 1) * 500) // 1000
        low = in_bin(LANE_LAST, k500 + 1, rng)
        other = np.arange(k500 + 1) % 3 == 1  # (index 0 stays in 2047)
        low[other] = in_bin(1000, int(other.sum()), rng)
        x = np.concatenate([low, in_bin(LANE_FIRST, n - (k500 + 1), rng)])[rng.permutation(n)]
    x = np.ascontiguousarray(x, f32)
    assert x.shape == (n, 3)
    x.flags.writeable = False
    return x


def test_the_contents_are_what_they_claim():
    """Conditions on the inputs, checked with the restatement."""
    n = 3 * B + 1
    assert len(np.unique(N.counted_bins(content("a_log_uniform", n)))) > 500
    assert len(np.unique(N.counted_bins(content("b_flat", n)))) == 1 and N.counted_bins(content("b_flat", n)).size == n
    assert N.counted_bins(content("c_nothing_counted", n)).size == 0 and np.isnan(content("c_nothing_counted", n)).any()
    assert set(N.counted_bins(content("d_bin_edges", n))) >= {16, 17, 63, 64, LANE_LAST, LANE_FIRST, 4079, 0x7F7FFFFF >> 19}
    assert 15 not in set(N.counted_bins(content("d_bin_edges", n)))
    for m in [s for s in SIZES if s >= 4]:
        h = N.histogram(content("e_rank_at_a_lane_boundary", m))
        assert h.sum() == m and N.rank_bin(h, 500) == LANE_LAST and N.rank_bin(h, 990) == LANE_FIRST, m
        k = ((m - 1) * 500) // 1000
        assert int(h[:LANE_LAST + 1].sum()) == k + 1  # rank k is the LAST pixel of lane 31's bins


class Run:
    """One rbrt_hip_tonemap call into buffers full of sentinels, one pixel longer than needed."""

    def __init__(self, hip, torch, x, opts, want_rad=True, want_rgb=True, workspace=True, in_place=False, d_in=None, ws=None):
        n = x.shape[0]
        self.d_in = torch.from_numpy(np.ascontiguousarray(x).copy()).cuda() if d_in is None else d_in
        if in_place:
            rad = self.d_in
        else:
            rad = torch.full((n + 1, 3), -7.0, dtype=torch.float32, device="cuda")
        rgb = torch.full((n + 1, 3), 77, dtype=torch.uint8, device="cuda")
        if ws is None:
            ws = torch.full((abi.TONEMAP_WORKSPACE_BYTES,), 0xAB, dtype=torch.uint8, device="cuda")
        hip.tonemap(0, self.d_in.data_ptr(), n, opts, ws.data_ptr() if workspace else None, rad.data_ptr() if want_rad else None,
                    rgb.data_ptr() if want_rgb else None)
        torch.cuda.synchronize()
        rad_h, rgb_h, raw = rad.cpu().numpy(), rgb.cpu().numpy(), ws.cpu().numpy()
        if not in_place:
            assert (rad_h[n:] == -7.0).all(), "wrote beyond the last pixel"
        assert (rgb_h[n:] == 77).all(), "wrote beyond the last pixel"
        self.rad, self.rgb = rad_h[:n], rgb_h[:n]
        self.hist = raw[:abi.TONEMAP_RESULT_OFFSET].view(u32)
        self.result = abi.TonemapResult.from_buffer_copy(raw[abi.TONEMAP_RESULT_OFFSET:].tobytes())
        self.ws = ws


def same_pixels(got, exp, what=""):
    got, exp = np.asarray(got, f32), np.asarray(exp, f32)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), (what, "NaN-ness", np.argwhere(gn != en)[:5])
    diff = (bits(got) != bits(exp)) & ~en
    assert not diff.any(), (what, np.argwhere(diff)[:5], got[diff][:5], exp[diff][:5])


def same_workspace(run: Run, ch, what=""):
    assert np.array_equal(run.hist, ch.hist), (what, np.argwhere(run.hist != ch.hist)[:5])
    r = run.result
    got = [bits([r.exposure])[0], bits([r.white])[0], bits([r.l_key])[0], bits([r.l_white])[0], r.counted, r.reserved, r.pixels]
    exp = [bits([ch.exposure])[0], bits([ch.white])[0], bits([ch.l_key])[0], bits([ch.l_white])[0], ch.counted, 0, ch.pixels]
    assert got == exp, (what, got, exp)


def opts_of(hip, curve, **kw):
    return hip.tonemap_opts(curve=curve, **kw)


def check_call(hip, torch, x, curve, what="", d_in=None, **kw):
    exp_rad, exp_rgb, ch = N.tonemap(x, curve, **kw)
    run = Run(hip, torch, x, opts_of(hip, curve, **kw), d_in=d_in)
    same_workspace(run, ch, what)
    same_pixels(run.rad, exp_rad, what)
    assert np.array_equal(run.rgb, exp_rgb), (what, np.argwhere(run.rgb != exp_rgb)[:5])
    return run, ch


# ---- 1. every size, every content, every curve: both automatic ---------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("n", SIZES)
def test_bit_identical_to_the_restatement(hip, n, kind):
    import torch
    x = content(kind, n)
    d_in = torch.from_numpy(x.copy()).cuda()
    for curve in CURVES:
        _, ch = check_call(hip, torch, x, curve, (n, kind, curve), d_in=d_in, exposure=0.0, white=0.0)
        if kind == "c_nothing_counted":
            assert ch.counted == 0 and ch.exposure == 1 and ch.white == 1
        if kind == "b_flat":
            assert ch.counted == n and ch.hist.max() == n


# ---- 2. manual and automatic, in every combination ---------------------------------------------------------------------------
@pytest.mark.parametrize("white", [0.0, 2.5])
@pytest.mark.parametrize("exposure", [0.0, 1.7])
@pytest.mark.parametrize("curve", CURVES)
def test_manual_and_automatic_in_every_combination(hip, curve, exposure, white):
    import torch
    x = content("a_log_uniform", 3 * B + 1)
    run, ch = check_call(hip, torch, x, curve, exposure=exposure, white=white, key=0.25, key_permille=400, white_permille=950)
    if exposure and white:  # nothing automatic: the result is written all the same, over zeroed histogram words
        assert not run.hist.any() and run.result.counted == 0 and run.result.exposure == f32(1.7) and run.result.white == 2.5
        bare = Run(hip, torch, x, opts_of(hip, curve, exposure=exposure, white=white), workspace=False)
        same_pixels(bare.rad, run.rad)
        assert np.array_equal(bare.rgb, run.rgb) and (bare.ws.cpu().numpy() == 0xAB).all()


@pytest.mark.parametrize("q", [0, 1, 999, 1000])
def test_the_extreme_ranks(hip, q):
    import torch
    x = content("a_log_uniform", B + 1)
    check_call(hip, torch, x, N.REINHARD, exposure=0.0, white=0.0, key_permille=q, white_permille=1000 - q)


# ---- 3. the buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", CURVES)
def test_in_place_equals_out_of_place(hip, curve):
    import torch
    x = content("a_log_uniform", 3 * B + 1)
    o = opts_of(hip, curve, exposure=0.0, white=0.0)
    apart = Run(hip, torch, x, o)
    inpl = Run(hip, torch, x, o, in_place=True)
    same_pixels(inpl.rad, apart.rad)
    assert np.array_equal(inpl.rgb, apart.rgb) and np.array_equal(inpl.hist, apart.hist)


def test_each_output_alone(hip):
    import torch
    x = content("a_log_uniform", B + 1)
    o = opts_of(hip, N.ACES, exposure=0.0, white=0.0)
    both = Run(hip, torch, x, o)
    rad_only = Run(hip, torch, x, o, want_rgb=False)
    rgb_only = Run(hip, torch, x, o, want_rad=False)
    neither = Run(hip, torch, x, o, want_rad=False, want_rgb=False)
    same_pixels(rad_only.rad, both.rad)
    assert (rad_only.rgb == 77).all() and (rgb_only.rad == -7.0).all() and np.array_equal(rgb_only.rgb, both.rgb)
    assert (neither.rgb == 77).all() and (neither.rad == -7.0).all()
    for r in (rad_only, rgb_only, neither):  # the choice is made whatever is written
        assert np.array_equal(r.hist, both.hist) and bytes(r.result) == bytes(both.result)


def test_pointers_that_are_not_16_byte_aligned_give_the_same_bits(hip):
    """The scalar form of the kernels: the same pixels one float into an allocation, and outputs one pixel in."""
    import torch
    n = 3 * B + 1
    x = content("a_log_uniform", n)
    o = opts_of(hip, N.REINHARD, exposure=0.0, white=0.0)
    ref = Run(hip, torch, x, o)
    shifted = torch.zeros(n * 3 + 1, dtype=torch.float32, device="cuda")
    shifted[1:] = torch.from_numpy(x.copy()).cuda().reshape(-1)
    rad = torch.full((n * 3 + 7,), -7.0, dtype=torch.float32, device="cuda")
    rgb = torch.full((n * 3 + 7,), 77, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(abi.TONEMAP_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
    hip.tonemap(0, shifted.data_ptr() + 4, n, o, ws.data_ptr(), rad.data_ptr() + 12, rgb.data_ptr() + 3)
    torch.cuda.synchronize()
    rad_h, rgb_h = rad.cpu().numpy(), rgb.cpu().numpy()
    same_pixels(rad_h[3:3 + 3 * n].reshape(n, 3), ref.rad)
    assert np.array_equal(rgb_h[3:3 + 3 * n].reshape(n, 3), ref.rgb)
    assert (rad_h[:3] == -7).all() and (rad_h[3 + 3 * n:] == -7).all() and (rgb_h[:3] == 77).all() and (rgb_h[3 + 3 * n:] == 77).all()
    assert np.array_equal(ws.cpu().numpy()[:abi.TONEMAP_RESULT_OFFSET].view(u32), ref.hist)


def test_a_second_call_on_one_workspace_forgets_the_first(hip):
    import torch
    x1, x2 = content("b_flat", 3 * B + 1), content("a_log_uniform", B + 1)
    o = opts_of(hip, N.ACES, exposure=0.0, white=0.0)
    first = Run(hip, torch, x1, o)
    assert first.hist.max() == 3 * B + 1
    second = Run(hip, torch, x2, o, ws=first.ws)
    same_workspace(second, N.choose(x2, exposure=0.0, white=0.0))


# ---- 4. a rendered image -----------------------------------------------------------------------------------------------------
W, H = 64, 48


def lamp_scene():
    """The example spheres with a lamp: radiance well above 1 next to the black sky of the constant background."""
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(abi.MAT_EMISSIVE, (12.0, 9.0, 4.0)))]
    return abi.SceneData(spheres=sph)


def test_a_rendered_image(hip, oracle):
    import torch
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=4, seed=6, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    with hip.HipScene(lamp_scene()) as hs:
        rad = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        rgb = torch.full((H, W, 3), 0, dtype=torch.uint8, device="cuda")
        hs.render_device(cam, opts, rad.data_ptr(), rgb.data_ptr())
        torch.cuda.synchronize()
        hs.check()
        x = rad.cpu().numpy().reshape(-1, 3)
        assert (x > 1.0).any() and (x == 0).all(axis=1).any()
        # LINEAR with e = 1: the render's own radiance and rgb8
        same = Run(hip, torch, x, opts_of(hip, N.LINEAR, exposure=1.0, white=1.0), d_in=rad.reshape(-1, 3))
        assert np.array_equal(bits(same.rad), bits(x)) and np.array_equal(same.rgb, rgb.cpu().numpy().reshape(-1, 3))
        # automatic exposure and ACES
        _, ch = check_call(hip, torch, x, N.ACES, d_in=rad.reshape(-1, 3), exposure=0.0, white=0.0)
        assert 0 < ch.counted < W * H
        # the same image as packed tiles: a rank's buffer is transformed as it is, and the three ranks' counts add up to the image's
        for (w, h) in ((W, H), (W - 4, H - 3)):  # (the second: ragged edge tiles, whose padding is zero and not counted)
            cam2 = scenes.camera(oracle, w, h)
            whole = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            hs.render_device(cam2, opts, whole.data_ptr())
            torch.cuda.synchronize()
            total = N.choose(whole.cpu().numpy(), exposure=0.0)
            hists = []
            for r in range(3):
                n = hip.packed_pixels(w, h, r, 3)
                packed = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
                o = abi.default_opts(spp=4, seed=6, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0), tile_rank=r, tile_world=3)
                hs.render_device(cam2, o, packed.data_ptr())
                torch.cuda.synchronize()
                run, _ = check_call(hip, torch, packed.cpu().numpy(), N.ACES, (w, h, r), d_in=packed, exposure=0.0, white=0.0)
                hists.append(run.hist.astype(np.int64))
            assert np.array_equal(sum(hists), total.hist.astype(np.int64)) and total.counted > 0
            assert sum(hip.packed_pixels(w, h, r, 3) for r in range(3)) > w * h or (w % 8 == 0 and h % 8 == 0)
        hs.check()


# ---- 5. what is refused ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(hip):
    import torch
    lib = abi.load_hip()
    n = 100
    x = torch.ones((n, 3), dtype=torch.float32, device="cuda")
    rad = torch.full((n, 3), -7.0, dtype=torch.float32, device="cuda")
    rgb = torch.full((n, 3), 77, dtype=torch.uint8, device="cuda")
    ws = torch.full((abi.TONEMAP_WORKSPACE_BYTES + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    T = hip.tonemap_opts
    nan, inf = float("nan"), float("inf")
    INVALID, UNSUPPORTED = abi.RBRT_ERR_INVALID_ARG, abi.RBRT_ERR_UNSUPPORTED
    # name: (input, n, opts, workspace, expected status)
    rows = {
        "null radiance": (0, n, T(), ws.data_ptr(), INVALID),
        "null opts": (x.data_ptr(), n, None, ws.data_ptr(), INVALID),
        "no pixels": (x.data_ptr(), 0, T(), ws.data_ptr(), INVALID),
        "unknown curve": (x.data_ptr(), n, T(curve=3), ws.data_ptr(), INVALID),
        "reserved[0]": (x.data_ptr(), n, T(reserved=(1, 0)), ws.data_ptr(), INVALID),
        "reserved[1]": (x.data_ptr(), n, T(reserved=(0, 1)), ws.data_ptr(), INVALID),
        "exposure nan": (x.data_ptr(), n, T(exposure=nan), ws.data_ptr(), INVALID),
        "exposure inf": (x.data_ptr(), n, T(exposure=inf), ws.data_ptr(), INVALID),
        "exposure negative": (x.data_ptr(), n, T(exposure=-1.0), ws.data_ptr(), INVALID),
        "key nan": (x.data_ptr(), n, T(key=nan), ws.data_ptr(), INVALID),
        "key inf, manual exposure": (x.data_ptr(), n, T(key=inf), ws.data_ptr(), INVALID),
        "white nan": (x.data_ptr(), n, T(white=nan), ws.data_ptr(), INVALID),
        "white inf": (x.data_ptr(), n, T(white=inf), ws.data_ptr(), INVALID),
        "white negative": (x.data_ptr(), n, T(white=-0.5), ws.data_ptr(), INVALID),
        "key 0, automatic exposure": (x.data_ptr(), n, T(exposure=0.0, key=0.0), ws.data_ptr(), INVALID),
        "key negative, automatic exposure": (x.data_ptr(), n, T(exposure=0.0, key=-0.18), ws.data_ptr(), INVALID),
        "key permille 1001": (x.data_ptr(), n, T(key_permille=1001), ws.data_ptr(), INVALID),
        "white permille 1001": (x.data_ptr(), n, T(white_permille=1001), ws.data_ptr(), INVALID),
        "automatic exposure, no workspace": (x.data_ptr(), n, T(exposure=0.0, white=1.0), 0, INVALID),
        "automatic white, no workspace": (x.data_ptr(), n, T(exposure=1.0, white=0.0), 0, INVALID),
        "workspace not aligned": (x.data_ptr(), n, T(), ws.data_ptr() + 8, INVALID),
        "2^32 pixels": (x.data_ptr(), 1 << 32, T(), ws.data_ptr(), UNSUPPORTED),
        "more than 2^32 pixels": (x.data_ptr(), (1 << 32) + 5, T(white=1.0), 0, UNSUPPORTED),
    }
    for name, (d_in, count, o, d_ws, status) in rows.items():
        rc = lib.rbrt_hip_tonemap(0, None, C.c_void_p(d_in), count, C.byref(o) if o is not None else None, C.c_void_p(d_ws),
                                  C.c_void_p(rad.data_ptr()), C.c_void_p(rgb.data_ptr()))
        assert rc == status, (name, rc, lib.rbrt_hip_last_error())
        assert lib.rbrt_hip_last_error(), name
    torch.cuda.synchronize()
    assert (rad.cpu().numpy() == -7.0).all() and (rgb.cpu().numpy() == 77).all() and (ws.cpu().numpy() == 0xAB).all()
    # a negative key is nobody's business while the exposure is manual, and the defaults are what the header says
    d = T()
    assert (d.curve, d.exposure, d.key_permille, d.white, d.white_permille, list(d.reserved)) == (0, 1.0, 500, 0.0, 990, [0, 0])
    assert d.key == f32(0.18)
    hip.tonemap(0, x.data_ptr(), n, T(key=-1.0, white=1.0), None, rad.data_ptr(), rgb.data_ptr())
    torch.cuda.synchronize()
    assert (rad.cpu().numpy() == 1.0).all() and (rgb.cpu().numpy() == 255).all()
