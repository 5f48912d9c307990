"""The glare stage on the GPU (rbrt_hip_glare) against its numpy restatement (np_glare.py), bit for bit: the float output, the
rgb8 output and the output in place. NaN pixels are compared as NaN-ness; there is no tolerance anywhere. Every device buffer
has a canary behind it (a row for the images, 64 bytes for the workspace) that must survive.

Sizes, with TW x TH = RBRT_GLARE_TILE_W x RBRT_GLARE_TILE_H, the tile of a level one REDUCE workgroup makes from 2 TW x 2 TH
pixels of the level above plus a halo: the smallest images; the corners (and the centre) of 2 TW - 1 .. 2 TW + 1 by
2 TH - 1 .. 2 TH + 1, around one workgroup's reach; and 6 TW + 1 by 6 TH + 1, three full workgroups and a ragged one per
direction at level 1, one of them with its whole halo inside the image, with ragged levels below. Contents are described at
`content`."""
from __future__ import annotations

import functools
import json
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_glare as G
import np_tonemap as N
import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
SCENE = ROOT / "scenes" / "emissive_spheres.yaml"
f32, u32 = np.float32, np.uint32
_dbg = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
TW = int(re.search(r"#define RBRT_GLARE_TILE_W (\d+)u", _dbg).group(1))
TH = int(re.search(r"#define RBRT_GLARE_TILE_H (\d+)u", _dbg).group(1))
assert (6 * TW + 1) * (6 * TH + 1) <= 200 * 100, "shrink the tile rather than growing the test"
SMALL = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5)]  # (W, H)
AROUND = [(2 * TW - 1, 2 * TH - 1), (2 * TW + 1, 2 * TH - 1), (2 * TW, 2 * TH), (2 * TW - 1, 2 * TH + 1), (2 * TW + 1, 2 * TH + 1)]
BIG = (6 * TW + 1, 6 * TH + 1)
SIZES = SMALL + AROUND + [BIG]
CONTENTS = ["a_log_uniform", "b_impulses", "c_flat", "d_nothing_bright", "e_salted"]
ALL_LEVELS = [1, 2, 3, 5, 8]


def bits(a):
    return np.ascontiguousarray(a, f32).view(u32)


def impulse_positions(w, h):
    """(y, x): the four corners, the middle of the top and the left edge, and both sides of the boundaries between the tiles of
    a REDUCE workgroup at level 1 (2 TW, 2 TH pixels of the image) and of the composite's workgroup (4 TW x TH pixels)."""
    pos = {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, w // 2), (h // 2, 0)}
    for bx in (2 * TW, 4 * TW):
        for by in (TH, 2 * TH):
            pos |= {(min(y, h - 1), min(x, w - 1)) for y in (by - 1, by) for x in (bx - 1, bx)}
    return sorted(pos)


@functools.lru_cache(maxsize=None)
def content(kind: str, w: int, h: int) -> np.ndarray:
    """An (h, w, 3) image, made once, shared, never changed.
    (a) luminances log-uniform over 2^-10 .. 2^10 with random chroma
    (b) impulses at impulse_positions over a dim background (0.01)
    (c) every pixel (0.75, 3.0, 0.5): bright for T = 0 and for T = 1
    (d) nothing bright for T = 1: luminances below 0.9, some pixels zero
    (e) (a) salted with NaN, +-inf, negative, denormal and -0 pixels, one pixel in 9"""
    rng = np.random.default_rng(104729 * CONTENTS.index(kind) + 1000 * w + h)
    if kind in ("a_log_uniform", "e_salted"):
        chroma = rng.uniform(0.05, 1.0, (h, w, 3)).astype(f32)
        target = (2.0 ** rng.uniform(-10.0, 10.0, (h, w))).astype(f32)
        x = (chroma * (target / N.luminance(chroma))[..., None]).astype(f32)
        if kind == "e_salted":
            tiny = np.finfo(f32).tiny
            salt = np.array([[np.nan, 1, 1], [1, np.nan, 400], [np.inf, 1, 1], [-np.inf, 1, 1], [np.inf, -np.inf, 0], [-1, -2, -3], [-50, 90, 2],
                             [40, -1, 3], [1e-42, 3e-43, 0], [tiny / 4, tiny / 4, tiny / 4], [-0.0, -0.0, -0.0], [0, 0, 0], [1e30, 1e30, 1e30]], f32)
            pick = rng.integers(0, 9, (h, w)) == 0
            x[pick] = salt[rng.integers(0, len(salt), int(pick.sum()))]
    elif kind == "b_impulses":
        x = np.full((h, w, 3), 0.01, f32)
        for k, (py, px) in enumerate(impulse_positions(w, h)):
            x[py, px] = (64.0 + k, 32.0, 16.0 + 3 * k)
    elif kind == "c_flat":
        x = np.tile(np.array([0.75, 3.0, 0.5], f32), (h, w, 1))
    else:
        chroma = rng.uniform(0.05, 1.0, (h, w, 3)).astype(f32)
        target = rng.uniform(0.0, 0.9, (h, w)).astype(f32)
        x = (chroma * (target / N.luminance(chroma))[..., None]).astype(f32)
        x[rng.integers(0, 5, (h, w)) == 0] = 0
    x = np.ascontiguousarray(x, f32)
    assert x.shape == (h, w, 3)
    x.flags.writeable = False
    return x


def test_the_contents_are_what_they_claim():
    """Conditions on the inputs, checked with the restatement."""
    w, h = BIG
    a = G.bright_mask(content("a_log_uniform", w, h), 1.0)
    assert a.any() and not a.all()
    assert G.bright_mask(content("c_flat", w, h), 1.0).all()
    assert not G.bright_mask(content("d_nothing_bright", w, h), 1.0).any() and G.bright_mask(content("d_nothing_bright", w, h), 0.0).any()
    e = content("e_salted", w, h)
    assert np.isnan(e).any() and np.isinf(e).any() and (e < 0).any() and (bits(e) == 0x80000000).any()
    assert ((e > 0) & (e < np.finfo(f32).tiny)).any()
    pos = impulse_positions(w, h)
    assert {(0, 0), (h - 1, w - 1), (2 * TH - 1, 2 * TW - 1), (2 * TH, 2 * TW), (TH - 1, 4 * TW - 1), (TH, 4 * TW)} <= set(pos)
    assert int(G.bright_mask(content("b_impulses", w, h), 1.0).sum()) == len(pos)
    assert G.sizes(w, h, 3)[1:] == [(3 * TW + 1, 3 * TH + 1), ((3 * TW + 2) // 2, (3 * TH + 2) // 2), ((3 * TW + 4) // 4, (3 * TH + 4) // 4)]


WS_CANARY = 64


class Run:
    """One rbrt_hip_glare call into buffers full of sentinels, one row longer than the image; the workspace is full of 0xAB
    before the call (the call may assume nothing about it) and 64 bytes longer than asked for."""

    def __init__(self, hip, torch, x, opts, want_rad=True, want_rgb=True, in_place=False, ws=None):
        h, w, _ = x.shape
        self.d_in = torch.full((h + 1, w, 3), -3.0, dtype=torch.float32, device="cuda")
        self.d_in[:h] = torch.from_numpy(np.ascontiguousarray(x).copy()).cuda()
        rad = self.d_in if in_place else torch.full((h + 1, w, 3), -7.0, dtype=torch.float32, device="cuda")
        rgb = torch.full((h + 1, w, 3), 77, dtype=torch.uint8, device="cuda")
        need = hip.glare_workspace_bytes(w, h, opts.levels)
        assert need > 0
        if ws is None:
            ws = torch.full((need + WS_CANARY,), 0xAB, dtype=torch.uint8, device="cuda")
        assert ws.numel() >= need + WS_CANARY and ws.data_ptr() % 16 == 0
        ws[need:] = 0xAB
        hip.glare(0, self.d_in.data_ptr(), w, h, opts, ws.data_ptr(), rad.data_ptr() if want_rad else None,
                  rgb.data_ptr() if want_rgb else None)
        torch.cuda.synchronize()
        rad_h, rgb_h = rad.cpu().numpy(), rgb.cpu().numpy()
        assert (rad_h[h:] == (-3.0 if in_place else -7.0)).all(), "wrote beyond the last row"
        assert (rgb_h[h:] == 77).all(), "wrote beyond the last row"
        assert (ws[need:].cpu().numpy() == 0xAB).all(), "wrote beyond the workspace"
        if not in_place:
            assert np.array_equal(bits(self.d_in.cpu().numpy()[:h]), bits(x)) and (self.d_in.cpu().numpy()[h:] == -3.0).all(), "the input changed"
        self.rad, self.rgb, self.ws = rad_h[:h], rgb_h[:h], ws


def same_pixels(got, exp, what=""):
    got, exp = np.asarray(got, f32), np.asarray(exp, f32)
    gn, en = np.isnan(got), np.isnan(exp)
    assert np.array_equal(gn, en), (what, "NaN-ness", np.argwhere(gn != en)[:5])
    diff = (bits(got) != bits(exp)) & ~en
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:5], got[diff][:5], exp[diff][:5])


def check_call(hip, torch, x, what="", **kw):
    exp_rad, exp_rgb = G.glare(x, **kw)
    run = Run(hip, torch, x, hip.glare_opts(**kw))
    same_pixels(run.rad, exp_rad, what)
    assert np.array_equal(run.rgb, exp_rgb), (what, np.argwhere(run.rgb != exp_rgb)[:5])
    return run, exp_rad


# ---- 1. every size, every content; every number of levels at the small and the large sizes -----------------------------------
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_identical_to_the_restatement(hip, size, kind):
    import torch
    w, h = size
    x = content(kind, w, h)
    for levels in (ALL_LEVELS if size in SMALL or size == BIG else [1, 3, 8]):
        _, exp = check_call(hip, torch, x, (size, kind, levels), threshold=1.0, intensity=0.1, levels=levels, spread=0.5)
        if kind == "d_nothing_bright":
            assert np.array_equal(exp, x)
        if kind == "e_salted":  # a defect stays in its own pixel
            assert np.array_equal(np.isfinite(exp), np.isfinite(x))


# ---- 2. the options ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("intensity", [0.1, 1.0])
@pytest.mark.parametrize("threshold", [0.0, 1.0])
@pytest.mark.parametrize("spread", [0.0, 0.5, 1.0])
def test_spread_threshold_and_intensity(hip, spread, threshold, intensity):
    import torch
    for size in ((3, 5), BIG):
        for kind in ("a_log_uniform", "b_impulses"):
            for levels in (1, 5):
                check_call(hip, torch, content(kind, *size), (size, kind, levels), threshold=threshold, intensity=intensity, levels=levels,
                           spread=spread)


def test_a_flat_image_with_threshold_0_comes_back_bit_for_bit(hip):
    """The header's consequence: T = 0, s = 1 gives out == X (0.75, 3.0 and 0.5 times 5 are exact)."""
    import torch
    x = np.tile(np.array([0.75, 3.0, 0.5], f32), (37, 53, 1))
    run = Run(hip, torch, x, hip.glare_opts(threshold=0.0, intensity=0.5, levels=5, spread=1.0))
    assert np.array_equal(bits(run.rad), bits(x)) and np.array_equal(run.rgb, N.quantise(x))


# ---- 3. the buffers ----------------------------------------------------------------------------------------------------------
VEC = (6 * TW + 4, 2 * TH + 1)  # a width that is a multiple of 4: aligned pointers take the 16-byte form


@pytest.mark.parametrize("size", [BIG, VEC, (3, 5)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_in_place_equals_out_of_place(hip, size):
    import torch
    x = content("e_salted", *size)
    o = hip.glare_opts(threshold=1.0, intensity=0.3, levels=5, spread=1.0)
    apart = Run(hip, torch, x, o)
    inpl = Run(hip, torch, x, o, in_place=True)
    same_pixels(inpl.rad, apart.rad)
    same_pixels(apart.rad, G.glare(x, 1.0, 0.3, 5, 1.0)[0])
    assert np.array_equal(inpl.rgb, apart.rgb)


@pytest.mark.parametrize("size", [BIG, VEC], ids=lambda s: f"{s[0]}x{s[1]}")
def test_each_output_alone(hip, size):
    import torch
    x = content("a_log_uniform", *size)
    o = hip.glare_opts(threshold=0.5, intensity=0.2, levels=3, spread=1.0)
    both = Run(hip, torch, x, o)
    rad_only = Run(hip, torch, x, o, want_rgb=False)
    rgb_only = Run(hip, torch, x, o, want_rad=False)
    neither = Run(hip, torch, x, o, want_rad=False, want_rgb=False)
    same_pixels(rad_only.rad, both.rad)
    assert (rad_only.rgb == 77).all() and (rgb_only.rad == -7.0).all() and np.array_equal(rgb_only.rgb, both.rgb)
    assert (neither.rgb == 77).all() and (neither.rad == -7.0).all()


def test_pointers_that_are_not_16_byte_aligned_give_the_same_bits(hip):
    """The scalar form of the composite: the same image one float into an allocation, and outputs one pixel in."""
    import torch
    w, h = VEC
    assert w % 4 == 0
    x = content("e_salted", w, h)
    o = hip.glare_opts(threshold=1.0, intensity=0.2, levels=4, spread=0.5)
    ref = Run(hip, torch, x, o)
    same_pixels(ref.rad, G.glare(x, 1.0, 0.2, 4, 0.5)[0])
    n = w * h * 3
    shifted = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    shifted[1:] = torch.from_numpy(x.copy()).cuda().reshape(-1)
    rad = torch.full((n + 7,), -7.0, dtype=torch.float32, device="cuda")
    rgb = torch.full((n + 7,), 77, dtype=torch.uint8, device="cuda")
    need = hip.glare_workspace_bytes(w, h, o.levels)
    ws = torch.full((need + WS_CANARY,), 0xAB, dtype=torch.uint8, device="cuda")
    hip.glare(0, shifted.data_ptr() + 4, w, h, o, ws.data_ptr(), rad.data_ptr() + 12, rgb.data_ptr() + 3)
    torch.cuda.synchronize()
    rad_h, rgb_h = rad.cpu().numpy(), rgb.cpu().numpy()
    same_pixels(rad_h[3:3 + n].reshape(h, w, 3), ref.rad)
    assert np.array_equal(rgb_h[3:3 + n].reshape(h, w, 3), ref.rgb)
    assert (rad_h[:3] == -7).all() and (rad_h[3 + n:] == -7).all() and (rgb_h[:3] == 77).all() and (rgb_h[3 + n:] == 77).all()
    assert (ws[need:].cpu().numpy() == 0xAB).all()
    # each pointer alone off its alignment
    for d_in, d_rad, d_rgb in ((4, 0, 0), (0, 12, 0), (0, 0, 3)):
        rad.fill_(-7.0), rgb.fill_(77)
        src = shifted.data_ptr() + 4
        if d_in == 0:
            aligned_in = torch.from_numpy(x.copy()).cuda()
            src = aligned_in.data_ptr()
        hip.glare(0, src, w, h, o, ws.data_ptr(), rad.data_ptr() + d_rad, rgb.data_ptr() + d_rgb)
        torch.cuda.synchronize()
        same_pixels(rad.cpu().numpy()[d_rad // 4:d_rad // 4 + n].reshape(h, w, 3), ref.rad, (d_in, d_rad, d_rgb))
        assert np.array_equal(rgb.cpu().numpy()[d_rgb:d_rgb + n].reshape(h, w, 3), ref.rgb), (d_in, d_rad, d_rgb)


def test_a_second_call_on_one_workspace_forgets_the_first(hip):
    import torch
    w, h = BIG
    o = hip.glare_opts(threshold=0.0, intensity=1.0, levels=8, spread=1.0)
    first = Run(hip, torch, content("c_flat", w, h), o)
    x2 = content("b_impulses", w - 5, h - 3)  # smaller: the first call's pyramid lies under and behind the second's
    o2 = hip.glare_opts(threshold=1.0, intensity=0.1, levels=3, spread=0.5)
    second = Run(hip, torch, x2, o2, ws=first.ws)
    exp_rad, exp_rgb = G.glare(x2, 1.0, 0.1, 3, 0.5)
    same_pixels(second.rad, exp_rad)
    assert np.array_equal(second.rgb, exp_rgb)


# ---- 4. a rendered image -----------------------------------------------------------------------------------------------------
W, H = 64, 48


def lamp_scene():
    """The example spheres with a lamp: radiance well above 1 next to the black sky of the constant background."""
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(abi.MAT_EMISSIVE, (12.0, 9.0, 4.0)))]
    return abi.SceneData(spheres=sph)


def test_a_rendered_frame_through_glare_and_the_display_transform(hip, oracle):
    import torch
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=4, seed=6, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    with hip.HipScene(lamp_scene()) as hs:
        rad = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(cam, opts, rad.data_ptr())
        torch.cuda.synchronize()
        hs.check()
        x = rad.cpu().numpy()
        assert G.bright_mask(x, 1.0).any() and not G.bright_mask(x, 1.0).all()
        g = hip.glare_opts(threshold=1.0, intensity=0.25, levels=4, spread=1.0)
        ws = torch.full((hip.glare_workspace_bytes(W, H, 4),), 0xAB, dtype=torch.uint8, device="cuda")
        glared = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        hip.glare(0, rad.data_ptr(), W, H, g, ws.data_ptr(), glared.data_ptr())
        t = hip.tonemap_opts(curve=N.ACES, exposure=0.0, white=1.0)
        tws = torch.zeros(abi.TONEMAP_WORKSPACE_BYTES, dtype=torch.uint8, device="cuda")
        out = torch.full((H, W, 3), float("nan"), dtype=torch.float32, device="cuda")
        rgb = torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        hip.tonemap(0, glared.data_ptr(), W * H, t, tws.data_ptr(), out.data_ptr(), rgb.data_ptr())
        torch.cuda.synchronize()
        exp_glared, _ = G.glare(x, 1.0, 0.25, 4, 1.0)
        same_pixels(glared.cpu().numpy(), exp_glared)
        exp_out, exp_rgb, ch = N.tonemap(exp_glared.reshape(-1, 3), N.ACES, exposure=0.0, white=1.0)
        same_pixels(out.cpu().numpy().reshape(-1, 3), exp_out)
        assert np.array_equal(rgb.cpu().numpy().reshape(-1, 3), exp_rgb) and ch.counted > 0
        dark = (x == 0).all(axis=2)
        assert dark.any() and (exp_glared[dark] > 0).any()  # the lamp's light has reached the black sky around it
        hs.check()


# ---- 5. the command line -----------------------------------------------------------------------------------------------------
CW, CHT, SPP = 72, 40, 8


def png(p, w=CW, h=CHT):
    from PIL import Image
    a = np.asarray(Image.open(p).convert("RGB"))
    assert a.shape == (h, w, 3)
    return a


def cli(tmp_path, name, *extra):
    """One run on the emissive spheres under a black sky; returns (target, report)."""
    out, rep = tmp_path / f"{name}.png", tmp_path / f"{name}.json"
    argv = [str(EXE), "-c", str(SCENE), "-t", str(out), "--height", str(CHT), "-w", str(CW), "-s", str(SPP), "--seed", "3", "--background", "0,0,0",
            "--report", str(rep), *extra]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return out, json.loads(rep.read_text())


def test_cli_glare_alone_and_in_front_of_the_display_transform(hip, tmp_path):
    pfm = tmp_path / "r.pfm"
    plain, js0 = cli(tmp_path, "plain", "--radiance", str(pfm))
    assert not [k for k in ("glare", "glare_levels", "glare_ms") if k in js0]
    rad = abi.read_pfm(pfm, any_value=True)
    assert G.bright_mask(rad, 1.0).any()
    assert np.array_equal(png(plain), N.quantise(rad))
    # glare alone: 0 EV, no curve -- the glare call's own rgb8; the radiance file stays without glare
    pfm1 = tmp_path / "g.pfm"
    out1, js1 = cli(tmp_path, "glare", "--glare", "0.3", "--radiance", str(pfm1))
    assert pfm1.read_bytes() == pfm.read_bytes()
    _, exp8 = G.glare(rad, 1.0, 0.3, 5, 1.0)
    assert np.array_equal(png(out1), exp8) and not np.array_equal(png(out1), png(plain))
    assert f32(js1["glare"]) == f32(0.3) and js1["glare_levels"] == 5 and 0.0 < js1["glare_ms"] < 1000.0 and "tonemap" not in js1
    # every option, and automatic exposure behind it: the exposure is chosen on the glared image
    out2, js2 = cli(tmp_path, "all", "--glare", "0.5", "--glare-threshold", "0.5", "--glare-levels", "3", "--glare-spread", "0.5",
                    "--exposure", "auto", "--tonemap", "aces")
    glared, _ = G.glare(rad, 0.5, 0.5, 3, 0.5)
    _, exp2, ch = N.tonemap(glared, N.ACES, exposure=0.0, white=1.0)
    assert np.array_equal(png(out2), exp2.reshape(CHT, CW, 3))
    assert f32(js2["exposure"]) == ch.exposure and js2["glare_levels"] == 3 and js2["glare"] == 0.5 and js2["tonemap"] == "aces"
    # two ranks on one GPU, tiles merged on the host: the same bytes
    out3, js3 = cli(tmp_path, "two", "--glare", "0.3", "--gpus", "2", "--oversubscribe", "--gather", "host")
    assert js3["gpus"] == 2 and np.array_equal(png(out3), png(out1))


def test_cli_two_ranks_glare_and_automatic_exposure_after_the_host_gather(hip, tmp_path):
    """Both display stages on the image two ranks rendered and the host merged (it goes up to rank 0's device once): the same
    bytes and the same chosen exposure as the one-rank run, where the stages work on the radiance that never left the device."""
    stages = ("--glare", "0.3", "--exposure", "auto", "--tonemap", "aces")
    one, js1 = cli(tmp_path, "one", *stages)
    two, js2 = cli(tmp_path, "two", *stages, "--gpus", "2", "--oversubscribe", "--gather", "host")
    assert js1["gpus"] == 1 and js2["gpus"] == 2 and js2["gather"] == "host"
    assert two.read_bytes() == one.read_bytes()
    assert js2["exposure"] == js1["exposure"] and js1["exposure"] > 0 and js2["tonemap"] == "aces" and f32(js2["glare"]) == f32(0.3)
    assert not np.array_equal(png(two), png(cli(tmp_path, "plain")[0]))  # (the stages did something)


def test_cli_the_noisy_file_gets_the_same_glare(hip, tmp_path):
    import torch
    pfm, noisy = tmp_path / "r.pfm", tmp_path / "noisy.png"
    out, js = cli(tmp_path, "dn", "--denoise", "--denoise-radius", "3", "--denoise-patch", "2", "--noisy", str(noisy), "--radiance", str(pfm),
                  "--glare", "0.4", "--glare-levels", "4")
    filtered = abi.read_pfm(pfm, any_value=True)
    assert np.array_equal(png(out), G.glare(filtered, 1.0, 0.4, 4, 1.0)[1])
    # the unfiltered radiance: --denoise without --adaptive is the fixed render
    hsn = abi.HostScene(SCENE, CHT, CW)
    o = abi.default_opts(spp=SPP, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    rad = torch.zeros((CHT, CW, 3), dtype=torch.float32, device="cuda")
    with hip.HipScene(hsn) as hs:
        hs.render_device(hsn.camera, o, rad.data_ptr(), lens=hsn.lens)
        torch.cuda.synchronize()
        hs.check()
    unfiltered = rad.cpu().numpy()
    assert not np.array_equal(bits(unfiltered), bits(filtered))
    assert np.array_equal(png(noisy), G.glare(unfiltered, 1.0, 0.4, 4, 1.0)[1])
    # ... and with a display transform behind both, the target's exposure for both
    out2, js2 = cli(tmp_path, "dn2", "--denoise", "--denoise-radius", "3", "--denoise-patch", "2", "--noisy", str(noisy),
                    "--glare", "0.4", "--glare-levels", "4", "--exposure", "auto", "--tonemap", "reinhard")
    g_f, g_u = G.glare(filtered, 1.0, 0.4, 4, 1.0)[0], G.glare(unfiltered, 1.0, 0.4, 4, 1.0)[0]
    ch = N.choose(g_f, exposure=0.0, white=0.0)
    assert f32(js2["exposure"]) == ch.exposure and f32(js2["white"]) == ch.white
    assert np.array_equal(png(out2), N.quantise(N.apply(g_f, N.REINHARD, ch.exposure, ch.white)))
    assert np.array_equal(png(noisy), N.quantise(N.apply(g_u, N.REINHARD, ch.exposure, ch.white)))


# ---- 6. what is refused on a machine with a device ---------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(hip):
    import ctypes as C

    import torch
    lib = abi.load_hip()
    w, h = 20, 10
    x = torch.full((h, w, 3), 5.0, dtype=torch.float32, device="cuda")
    rad = torch.full((h, w, 3), -7.0, dtype=torch.float32, device="cuda")
    rgb = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
    ws = torch.full((hip.glare_workspace_bytes(w, h, 8) + 16,), 0xAB, dtype=torch.uint8, device="cuda")
    T = hip.glare_opts
    rows = {
        "null workspace": (x.data_ptr(), w, h, T(), 0, abi.RBRT_ERR_INVALID_ARG),
        "levels 9": (x.data_ptr(), w, h, T(levels=9), ws.data_ptr(), abi.RBRT_ERR_INVALID_ARG),
        "intensity 0": (x.data_ptr(), w, h, T(intensity=0.0), ws.data_ptr(), abi.RBRT_ERR_INVALID_ARG),
        "workspace not aligned": (x.data_ptr(), w, h, T(), ws.data_ptr() + 8, abi.RBRT_ERR_INVALID_ARG),
        "2^31 pixels": (x.data_ptr(), 1 << 16, 1 << 15, T(), ws.data_ptr(), abi.RBRT_ERR_UNSUPPORTED),
    }
    for name, (d_in, ww, hh, o, d_ws, status) in rows.items():
        rc = lib.rbrt_hip_glare(0, None, C.c_void_p(d_in), ww, hh, C.byref(o), C.c_void_p(d_ws), C.c_void_p(rad.data_ptr()),
                                C.c_void_p(rgb.data_ptr()))
        assert rc == status, (name, rc, lib.rbrt_hip_last_error())
    torch.cuda.synchronize()
    assert (rad.cpu().numpy() == -7.0).all() and (rgb.cpu().numpy() == 77).all() and (ws.cpu().numpy() == 0xAB).all()
