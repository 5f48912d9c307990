"""The denoiser on the GPU (rbrt_hip_denoise_halves, rbrt_hip_scene_denoise) against its numpy restatement (np_denoise.py),
bit for bit, and against a converged render.

Synthetic halves go through denoise_halves: a smooth ramp plus noise (weights between 0 and 1), a block with A == B exactly
(V = 0) and a block of values up to 1e6; sizes below the window, ragged, several workgroups, and one below / at / one above
the kernel's tile edge (RBRT_DENOISE_TILE) in each direction; then sizes with workgroups whose halo lies wholly inside the
image and grids of three to five workgroups in a direction (INTERIOR_SIZES). Through a handle the cases are test_adaptive_gpu.py's: the
samples come from render_pass, the tile counts from np_adaptive, the thresholds from the restatement."""
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

import np_adaptive as A
import np_denoise as D
import scenes
import test_adaptive_gpu as T
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
EDGE = int(re.search(r"#define RBRT_DENOISE_TILE (\d+)u", (ROOT / "include" / "rbrt_hip_debug.h").read_text()).group(1))

#         W   H
SIZES = [(1, 1), (5, 3), (8, 8), (37, 21), (40, 24),
         (EDGE - 1, 3), (EDGE, 3), (EDGE + 1, 3), (3, EDGE - 1), (3, EDGE), (3, EDGE + 1)]
#          R  P  strength
PARAMS = [(0, 0, 0.7), (1, 0, 0.45), (0, 3, 0.7), (2, 1, 1.3), (5, 3, 0.7), (10, 4, 0.7)]
# Sizes with workgroups away from the image's edges (a workgroup is EDGE x EDGE = 16 x 16 pixels, its staged halo R + P):
INTERIOR_SIZES = [(48, 48),   # 3 x 3 workgroups: the centre one's halo is wholly inside even at R 10, P 4 (16 - 14 >= 0, 32 + 14 <= 48)
                  (50, 47),   # the same, with ragged last workgroups of 2 columns and 15 rows
                  (80, 17),   # five workgroups across; the second row of workgroups is one pixel high: the offsets it skips
                  (17, 80),   # (no q inside) differ from its neighbours'; and the same the other way round
                  (64, 33)]   # four across, a third row of one pixel
# ... at every row of PARAMS and at the two extremes of the staged edge against the edge of the delta area: the widest
# window with no patch, and the widest patch (three delta positions a thread) with the smallest window
INTERIOR_PARAMS = PARAMS + [(10, 0, 0.7), (1, 4, 0.7)]


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def synthetic(w, h, seed=None):
    """(A, B, wa): a ramp plus independent noise in each half; the top-left quarter has A == B; the bottom-right quarter
    holds values up to 1e6. No value is 0."""
    rng = np.random.default_rng(1000 * w + h if seed is None else seed)
    y, x = np.meshgrid(np.arange(h, dtype=f32), np.arange(w, dtype=f32), indexing="ij")
    ramp = (f32(0.2) + f32(0.5) * x / f32(max(w, 1)) + f32(0.2) * y / f32(max(h, 1)))[..., None] * np.array([1.0, 0.8, 0.6], f32)
    a = (ramp + rng.normal(0.0, 0.04, (h, w, 3)).astype(f32)).astype(f32)
    b = (ramp + rng.normal(0.0, 0.04, (h, w, 3)).astype(f32)).astype(f32)
    a, b = np.abs(a) + f32(1e-3), np.abs(b) + f32(1e-3)
    b[:(h + 1) // 2, :(w + 1) // 2] = a[:(h + 1) // 2, :(w + 1) // 2]
    if h >= 3 and w >= 3:
        big = (slice(h - h // 3, h), slice(w - w // 3, w))
        scale = (10.0 ** rng.uniform(3.0, 6.0, a[big].shape[:2])).astype(f32)[..., None]
        a[big], b[big] = np.minimum(a[big] * scale, f32(1e6)), np.minimum(b[big] * scale, f32(1e6))
    wa = rng.uniform(0.3, 0.7, (h, w)).astype(f32)
    assert a.dtype == f32 and b.dtype == f32 and np.isfinite(a).all() and np.isfinite(b).all() and (a != 0).all() and (b != 0).all()
    for arr in (a, b, wa):
        arr.flags.writeable = False
    return a, b, wa


@functools.lru_cache(maxsize=None)
def expected(w, h, R, P, k):
    """The restatement's filtered halves for a synthetic case: made once, shared, never changed."""
    a, b, wa = synthetic(w, h)
    ah, bh = D.filtered_halves(a, b, R, P, k)
    ah.flags.writeable = False
    bh.flags.writeable = False
    return a, b, wa, ah, bh


def run_halves(hip, torch, a, b, wa, R, P, k, want_rad=True, want_rgb=True):
    """One denoise_halves call into buffers full of sentinels."""
    h, w, _ = a.shape
    da, db = torch.from_numpy(a.copy()).cuda(), torch.from_numpy(b.copy()).cuda()
    dwa = torch.from_numpy(wa.copy()).cuda() if wa is not None else None
    rad = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    rgb = torch.full((h, w, 3), 77, dtype=torch.uint8, device="cuda")
    hip.denoise_halves(0, da.data_ptr(), db.data_ptr(), dwa.data_ptr() if dwa is not None else None, w, h,
                       rad.data_ptr() if want_rad else None, rgb.data_ptr() if want_rgb else None, R, P, k)
    torch.cuda.synchronize()
    return rad.cpu().numpy(), rgb.cpu().numpy()


# ---- 1. synthetic halves against the restatement ----------------------------------------------------------------------------
def test_the_synthetic_inputs_exercise_the_weights():
    """A condition on the inputs: at the default parameters the weights of the noisy ramp are neither all 0 nor all 1, the
    A == B block has V = 0, and the large block reaches beyond 1e5."""
    a, b, wa = synthetic(40, 24)
    V = D.variance(a, b)
    assert (V[:8, :8] == 0).all() and (V[14:, :] > 0).all() and a.max() > 1e5 and a.max() <= 1e6
    k2 = f32(0.7) * f32(0.7)
    w = D.weight(D.patch_distance(b, V, 0, 1, 3, k2))[:, :39]
    assert ((w > 0.01) & (w < 0.99)).sum() > 100 and (w == 0).any() and (w > 0.9).any(), np.histogram(w, 10, (0, 1))[0]


def check_halves(hip, w, h, R, P, k):
    """One synthetic case through denoise_halves, every way of asking for its outputs."""
    import torch
    a, b, wa, ah, bh = expected(w, h, R, P, k)
    exp = D.mix(ah, bh, wa)
    rad, rgb = run_halves(hip, torch, a, b, wa, R, P, k)
    assert np.array_equal(bits(rad), bits(exp)), (int((bits(rad) != bits(exp)).sum()), float(np.nanmax(np.abs(rad - exp))))
    assert np.array_equal(rgb, D.quantise(exp))
    # d_wa NULL is 0.5 everywhere
    exp_half = D.mix(ah, bh, None)
    rad, rgb = run_halves(hip, torch, a, b, None, R, P, k)
    assert np.array_equal(bits(rad), bits(exp_half)) and np.array_equal(rgb, D.quantise(exp_half))
    assert np.array_equal(bits(exp_half), bits(D.mix(ah, bh, np.full((h, w), 0.5, f32))))
    # one output at a time: the other buffer keeps its sentinels
    rad, rgb = run_halves(hip, torch, a, b, wa, R, P, k, want_rgb=False)
    assert np.array_equal(bits(rad), bits(exp)) and (rgb == 77).all()
    rad, rgb = run_halves(hip, torch, a, b, wa, R, P, k, want_rad=False)
    assert np.isnan(rad).all() and np.array_equal(rgb, D.quantise(exp))
    if R == 0:  # the identity: no filtering at all
        assert np.array_equal(bits(exp), bits(D.mix(a, b, wa)))


@pytest.mark.parametrize("R,P,k", PARAMS, ids=[f"R{r}_P{p}" for r, p, _ in PARAMS])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_halves_against_the_restatement(hip, w, h, R, P, k):
    check_halves(hip, w, h, R, P, k)


def test_the_centre_workgroup_of_48x48_has_weights_between_0_and_1():
    """A condition on the inputs: synthetic()'s A == B quarter and its quarter of large values move with the size. At 48 x 48
    and the default parameters the pixels of the centre workgroup (rows and columns 16..31) have weights strictly between
    0.01 and 0.99 for more than 100 (pixel, offset) pairs: the one workgroup whose staged tile is clipped nowhere is neither
    all 0 nor all 1."""
    a, b, wa = synthetic(48, 48)
    V = D.variance(a, b)
    R, P, k = (D.DEFAULTS[n] for n in ("window_radius", "patch_radius", "strength"))
    k2 = f32(k) * f32(k)
    pairs = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            w = D.weight(D.patch_distance(b, V, dy, dx, P, k2))[16:32, 16:32]
            pairs += int(((w > 0.01) & (w < 0.99)).sum())
    assert pairs > 100, pairs


@pytest.mark.parametrize("R,P,k", INTERIOR_PARAMS, ids=[f"R{r}_P{p}" for r, p, _ in INTERIOR_PARAMS])
@pytest.mark.parametrize("w,h", INTERIOR_SIZES, ids=[f"{w}x{h}" for w, h in INTERIOR_SIZES])
def test_halves_with_interior_workgroups(hip, w, h, R, P, k):
    """Workgroups whose whole halo is inside the image, and grids with a middle row and a middle column of workgroups: the
    delta, row-sum and skip logic without the clipping that could mask an error in it."""
    assert 0.45 <= k <= 1.3
    a, b, wa, ah, bh = expected(w, h, R, P, k)
    assert np.isfinite(ah).all() and np.isfinite(bh).all()  # (non-finite halves are outside the rule: fminf and np.minimum differ on NaN)
    assert (w + EDGE - 1) // EDGE >= 3 or (h + EDGE - 1) // EDGE >= 3
    check_halves(hip, w, h, R, P, k)


def test_a_tiny_strength_filters_nothing(hip):
    """Every pixel differs from every other one by at least 0.01 in every channel and the halves agree to 1e-5: at strength
    1e-6 every weight but the pixel's own is 0, and the output is (A * wa) + (B * (1 - wa)) exactly."""
    import torch
    w, h = 19, 18
    rng = np.random.default_rng(5)
    levels = np.stack([rng.permutation(w * h) for _ in range(3)], axis=-1).reshape(h, w, 3)
    a = (f32(0.5) + f32(0.01) * levels.astype(f32)).astype(f32)
    b = (a + rng.uniform(-1e-5, 1e-5, a.shape).astype(f32)).astype(f32)
    wa = rng.uniform(0.3, 0.7, (h, w)).astype(f32)
    rad, rgb = run_halves(hip, torch, a, b, wa, 5, 3, 1e-6)
    exp = D.mix(a, b, wa)
    assert np.array_equal(bits(rad), bits(exp)) and np.array_equal(rgb, D.quantise(exp))
    assert np.array_equal(bits(D.denoise(a, b, wa, 5, 3, 1e-6)[0]), bits(exp))  # (the restatement agrees)


# ---- 2. through a handle ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def data(hip, oracle):
    """Per case of test_adaptive_gpu.py: the per-sample radiance, and for the thresholds zero and median the restatement's
    tile counts, half images and denoised image at the default parameters. Made once, never changed."""
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
            S, S_even = D.halves_from_samples(samples, r.counts)
            assert np.array_equal(bits(S * (f32(1) / r.counts[np.arange(h)[:, None] // 8, np.arange(w)[None, :] // 8].astype(f32))[..., None]),
                                  bits(r.image))  # (the sums are the adaptive restatement's)
            a, b, wa = D.halves(S, S_even, r.counts)
            img, rgb8 = D.denoise(a, b, wa)
            rest[kind] = SimpleNamespace(counts=r.counts, a=a, b=b, wa=wa, image=img, rgb8=rgb8, noisy=r.image)
        samples.flags.writeable = False
        d[cid] = SimpleNamespace(cid=cid, scene=scene, w=w, h=h, n=n, mn=mn, step=step, cam=cam, lens=lens, sc=sc, opts_of=opts_of,
                                 thr=thr, rest=rest)
    return d


def run_denoise(hs, torch, c, **params):
    rad = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
    rgb = torch.full((c.h, c.w, 3), 77, dtype=torch.uint8, device="cuda")
    ha = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
    hb = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
    hs.denoise(rad.data_ptr(), rgb.data_ptr(), ha.data_ptr(), hb.data_ptr(), **params)
    torch.cuda.synchronize()
    return SimpleNamespace(rad=rad.cpu().numpy(), rgb=rgb.cpu().numpy(), a=ha.cpu().numpy(), b=hb.cpu().numpy())


def test_the_cases_have_counts_of_both_parities(data):
    seen = set()
    for c in data.values():
        assert (c.rest["zero"].counts == c.n).all()
        assert len(np.unique(c.rest["median"].counts)) >= 2, (c.cid, c.rest["median"].counts)
        seen |= set(int(v) for v in np.unique(c.rest["median"].counts))
    assert any(v % 2 for v in seen) and any(v % 2 == 0 for v in seen), seen


@pytest.mark.parametrize("kind", ["zero", "median"])
@pytest.mark.parametrize("cid", T.IDS)
def test_a_handle_denoises_its_last_adaptive_render(hip, data, cid, kind):
    import torch
    c = data[cid]
    r = c.rest[kind]
    with hip.HipScene(c.sc) as hs:
        before = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(c.cam, c.opts_of(c.n), before.data_ptr(), lens=c.lens)
        torch.cuda.synchronize()
        g = T.run_adaptive(hs, torch, c, c.thr[kind])
        assert np.array_equal(g.counts, A.per_rank(r.counts)) and np.array_equal(bits(g.rad), bits(r.noisy)), (cid, kind)
        d1 = run_denoise(hs, torch, c)
        assert np.array_equal(bits(d1.a), bits(r.a)) and np.array_equal(bits(d1.b), bits(r.b)), (cid, kind)
        assert np.array_equal(bits(d1.rad), bits(r.image)), (cid, kind, int((bits(d1.rad) != bits(r.image)).sum()))
        assert np.array_equal(d1.rgb, r.rgb8)
        d2 = run_denoise(hs, torch, c)  # a second call: the same bits
        for x, y in ((d1.rad, d2.rad), (d1.a, d2.a), (d1.b, d2.b)):
            assert np.array_equal(bits(x), bits(y))
        assert np.array_equal(d1.rgb, d2.rgb)
        after = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(c.cam, c.opts_of(c.n), after.data_ptr(), lens=c.lens)  # a fixed render is what it was
        torch.cuda.synchronize()
        assert np.array_equal(bits(after.cpu().numpy()), bits(before.cpu().numpy()))
        d3 = run_denoise(hs, torch, c)  # ... and leaves the adaptive image to denoise
        assert np.array_equal(bits(d3.rad), bits(r.image))
        hs.check()


def test_other_parameters_and_null_outputs_through_a_handle(hip, data):
    import torch
    c = data["spheres_37x21_odd"]
    r = c.rest["median"]
    with hip.HipScene(c.sc) as hs:
        T.run_adaptive(hs, torch, c, c.thr["median"])
        g = run_denoise(hs, torch, c, window_radius=2, patch_radius=1, strength=1.0)
        exp, exp8 = D.denoise(r.a, r.b, r.wa, 2, 1, 1.0)
        assert np.array_equal(bits(g.rad), bits(exp)) and np.array_equal(g.rgb, exp8)
        hs.denoise()  # every output NULL
        rgb = torch.full((c.h, c.w, 3), 77, dtype=torch.uint8, device="cuda")
        hs.denoise(None, rgb.data_ptr())
        torch.cuda.synchronize()
        assert np.array_equal(rgb.cpu().numpy(), r.rgb8)
        hs.check()


# ---- 3. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(hip, data):
    import torch
    c = data["spheres_40x24"]
    lib = hip.load_hip()
    ok = abi.DenoiseOpts(5, 3, 0.7, 0)
    bad_opts = {"reserved": abi.DenoiseOpts(5, 3, 0.7, 1), "R 11": abi.DenoiseOpts(11, 3, 0.7, 0), "P 5": abi.DenoiseOpts(5, 5, 0.7, 0),
                "nan strength": abi.DenoiseOpts(5, 3, float("nan"), 0), "inf strength": abi.DenoiseOpts(5, 3, float("inf"), 0),
                "strength 0": abi.DenoiseOpts(5, 3, 0.0, 0), "negative strength": abi.DenoiseOpts(5, 3, -0.7, 0)}
    buf = torch.full((c.h, c.w, 3), 0.25, dtype=torch.float32, device="cuda")
    out = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
    p = C.c_void_p(buf.data_ptr())

    def halves(a=p, b=p, opts=ok, w=c.w, h=c.h):
        rc = lib.rbrt_hip_denoise_halves(0, None, a, b, None, w, h, C.byref(opts) if opts is not None else None,
                                         C.c_void_p(out.data_ptr()), None)
        return rc, lib.rbrt_hip_last_error().decode()

    rows = {"null a": dict(a=None), "null b": dict(b=None), "null opts": dict(opts=None), "width 0": dict(w=0), "height 0": dict(h=0)}
    rows.update({k: dict(opts=v) for k, v in bad_opts.items()})
    for what, kw in rows.items():
        rc, msg = halves(**kw)
        assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (what, rc, msg)
    torch.cuda.synchronize()
    assert np.isnan(out.cpu().numpy()).all()  # nothing ran
    assert halves()[0] == abi.RBRT_OK

    def scene_call(hs, scene=True, opts=ok):
        rc = lib.rbrt_hip_scene_denoise(hs._h if scene else None, C.byref(opts) if opts is not None else None, None,
                                        C.c_void_p(out.data_ptr()), None, None, None)
        return rc, lib.rbrt_hip_last_error().decode()

    out.fill_(float("nan"))
    with hip.HipScene(c.sc) as hs:
        rc, msg = scene_call(hs)  # no adaptive render on the handle yet
        assert rc == abi.RBRT_ERR_INVALID_ARG and "adaptive" in msg, (rc, msg)
        hs.render_adaptive(c.cam, c.opts_of(c.n), T.HUGE, c.mn, c.step)
        for what, kw in {"null scene": dict(scene=False), "null opts": dict(opts=None), **{k: dict(opts=v) for k, v in bad_opts.items()}}.items():
            rc, msg = scene_call(hs, **kw)
            assert rc == abi.RBRT_ERR_INVALID_ARG and msg, (what, rc, msg)
        hs.render_adaptive(c.cam, c.opts_of(1), T.HUGE, c.mn, c.step)  # spp 1: a half would be empty
        rc, msg = scene_call(hs)
        assert rc == abi.RBRT_ERR_INVALID_ARG and "spp" in msg, (rc, msg)
        hs.render_adaptive(c.cam, c.opts_of(c.n, tile_rank=0, tile_world=2), T.HUGE, c.mn, c.step)
        rc, msg = scene_call(hs)
        assert rc == abi.RBRT_ERR_UNSUPPORTED and "tile_world" in msg, (rc, msg)
        torch.cuda.synchronize()
        assert np.isnan(out.cpu().numpy()).all()
        # ... and the handle still renders and denoises
        T.run_adaptive(hs, torch, c, c.thr["median"])
        assert np.array_equal(bits(run_denoise(hs, torch, c).rad), bits(c.rest["median"].image))
        hs.check()


def test_defaults_and_tile_constant(hip):
    d = hip.denoise_opts()
    assert (d.window_radius, d.patch_radius, d.reserved) == (5, 3, 0) and d.strength == f32(0.7)
    assert D.DEFAULTS == dict(window_radius=5, patch_radius=3, strength=0.7) and EDGE >= 8


# ---- 4. the command line ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("adaptive", [False, True], ids=["fixed", "adaptive"])
def test_cli_denoises_and_reports(hip, tmp_path, adaptive):
    """--denoise alone is the fixed render, filtered; with --adaptive the adaptive one. -t gets the filtered image, --noisy the
    unfiltered one, both equal to the library's own calls on the same scene."""
    import torch
    w, h, n, R, P, k = 72, 40, 24, 3, 2, 0.9
    mn, step, thr = (4, 8, 0.02) if adaptive else (n, n, 0.0)
    cfg = ROOT / "scenes" / "emissive_spheres.yaml"
    png, noisy, rep = tmp_path / "a.ppm", tmp_path / "noisy.ppm", tmp_path / "rep.json"
    argv = [str(EXE), "-c", str(cfg), "-t", str(png), "--height", str(h), "-w", str(w), "-s", str(n), "--seed", "3", "--background", "0,0,0",
            "--denoise", "--denoise-radius", str(R), "--denoise-patch", str(P), "--denoise-strength", str(k), "--noisy", str(noisy), "--report", str(rep)]
    if adaptive:
        argv += ["--adaptive", str(thr), "--min-samples", str(mn), "--adaptive-step", str(step)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(rep.read_text())
    assert (js["denoise_window_radius"], js["denoise_patch_radius"]) == (R, P) and js["denoise_strength"] == pytest.approx(k, rel=1e-6)
    assert 0.0 < js["denoise_ms"] < 1000.0 and js["denoise_ms"] / 1e3 < js["render_s"]
    assert ("adaptive_rounds" in js) == adaptive
    hsn = abi.HostScene(cfg, h, w)
    o = abi.default_opts(spp=n, seed=3, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0))
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    den = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    fixed = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    with hip.HipScene(hsn) as hs:
        hs.render_device(hsn.camera, o, None, fixed.data_ptr(), lens=hsn.lens)
        res = hs.render_adaptive(hsn.camera, o, thr, mn, step, None, rgb.data_ptr(), lens=hsn.lens)
        hs.denoise(None, den.data_ptr(), window_radius=R, patch_radius=P, strength=k)
        torch.cuda.synchronize()
        hs.check()
    if adaptive:
        assert js["adaptive_rounds"] == res["rounds"] and js["samples_traced"] == res["samples"] < res["samples_fixed"]
    else:
        assert res["rounds"] == 1 and np.array_equal(rgb.cpu().numpy(), fixed.cpu().numpy())  # one round: the fixed render

    def ppm(p):
        raw = p.read_bytes()
        head = f"P6\n{w} {h}\n255\n".encode()
        assert raw.startswith(head)
        return np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)
    assert np.array_equal(ppm(noisy), rgb.cpu().numpy())
    assert np.array_equal(ppm(png), den.cpu().numpy())
    assert not np.array_equal(ppm(png), ppm(noisy))


# ---- 5. does it denoise -------------------------------------------------------------------------------------------------------
def test_the_denoised_image_is_closer_to_a_converged_render(hip, oracle):
    """Spheres, 160 x 96, a limit of 16 spp with threshold 0 (every tile takes 16), default parameters; the reference is the
    fixed path at 1024 spp with another seed. Measured on one MI355X: RMSE of the noisy image 0.01562, of the denoised one
    0.00895: a ratio of 0.573."""
    import torch
    w, h, n = 160, 96, 16
    cam = scenes.camera(oracle, w, h)
    sc = scenes.spheres_scene()
    with hip.HipScene(sc) as hs:
        ref = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        hs.render_device(cam, abi.default_opts(spp=1024, seed=T.SEED + 1), ref.data_ptr())
        noisy = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        res = hs.render_adaptive(cam, abi.default_opts(spp=n, seed=T.SEED), 0.0, 16, 64, noisy.data_ptr())
        assert res["samples"] == w * h * n
        den = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        hs.denoise(den.data_ptr())
        torch.cuda.synchronize()
        hs.check()
    ref, noisy, den = (t.cpu().numpy().astype(np.float64) for t in (ref, noisy, den))
    rmse_noisy, rmse_den = float(np.sqrt(np.mean((noisy - ref) ** 2))), float(np.sqrt(np.mean((den - ref) ** 2)))
    print(f"RMSE noisy {rmse_noisy:.5f}, denoised {rmse_den:.5f}, ratio {rmse_den / rmse_noisy:.3f}")
    assert np.isfinite(den).all()
    assert rmse_den < rmse_noisy, (rmse_den, rmse_noisy)
