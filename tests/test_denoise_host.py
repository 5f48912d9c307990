"""The denoiser without a GPU: the numpy restatement of the rule (np_denoise.py) against scalar arithmetic written out by
hand, the layout of the new struct against a host-compiled probe, and the CLI's flags, refusals and help text."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_denoise as D
from rbrt_amd import abi, srchash

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32


def halves(h, w, seed, noise=0.05):
    rng = np.random.default_rng(seed)
    base = rng.uniform(0.2, 0.9, (h, w, 3)).astype(f32)
    a = (base + rng.normal(0, noise, (h, w, 3)).astype(f32)).astype(f32)
    b = (base + rng.normal(0, noise, (h, w, 3)).astype(f32)).astype(f32)
    return a, b, rng.uniform(0.3, 0.7, (h, w)).astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the rule ----------------------------------------------------------------------------------------------------------------
def by_hand(A, B, wa, R, P, k, py, px):
    """One output pixel with scalars, every operation and loop written as in the rule."""
    H, W, _ = A.shape
    inside = lambda y, x: 0 <= y < H and 0 <= x < W
    eps, k2 = f32(1e-7), f32(f32(k) * f32(k))

    def V(y, x, c):
        s, n = f32(0), 0
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if inside(y + dy, x + dx):
                    d = f32(A[y + dy, x + dx, c] - B[y + dy, x + dx, c])
                    s = f32(s + f32(d * d))
                    n += 1
        return f32(f32(s / f32(n)) * f32(0.5))

    def delta(G, y, x, dy, dx):
        if not (inside(y, x) and inside(y + dy, x + dx)):
            return f32(0)
        t = []
        for c in range(3):
            vp, vq = V(y, x, c), V(y + dy, x + dx, c)
            g = f32(G[y + dy, x + dx, c] - G[y, x, c])
            t.append(f32(f32(f32(g * g) - f32(vp + min(vp, vq))) / f32(eps + f32(k2 * f32(vp + vq)))))
        return f32(f32(t[0] + t[1]) + t[2])

    def filt(F, G):
        num, den = [f32(0)] * 3, f32(0)
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                if not inside(py + dy, px + dx):
                    continue
                Dd, cnt = f32(0), 0
                for j in range(-P, P + 1):
                    r = f32(0)
                    for i in range(-P, P + 1):
                        r = f32(r + delta(G, py + j, px + i, dy, dx))
                        cnt += inside(py + j, px + i) and inside(py + j + dy, px + i + dx)
                    Dd = f32(Dd + r)
                Dd = f32(Dd / f32(3 * cnt))
                t = max(f32(0), f32(f32(1) - f32(f32(0.25) * max(Dd, f32(0)))))
                w = f32(f32(t * t) * f32(t * t))
                num = [f32(num[c] + f32(w * F[py + dy, px + dx, c])) for c in range(3)]
                den = f32(den + w)
        return [f32(num[c] / den) for c in range(3)]

    ah, bh = filt(A, B), filt(B, A)
    m = f32(wa[py, px])
    return np.array([f32(f32(ah[c] * m) + f32(bh[c] * f32(f32(1) - m))) for c in range(3)], f32)


@pytest.mark.parametrize("R,P,k", [(2, 1, 0.7), (1, 2, 1.2), (3, 0, 0.45)])
def test_the_restatement_by_hand(R, P, k):
    """Corners, edges and the middle of a 7 x 6 image (smaller than most windows), every pixel with scalars."""
    a, b, wa = halves(6, 7, 11)
    b[:2, :3] = a[:2, :3]  # V = 0 in a corner
    out, rgb8 = D.denoise(a, b, wa, R, P, k)
    assert out.dtype == f32 and rgb8.dtype == np.uint8
    for py, px in ((0, 0), (0, 6), (5, 0), (5, 6), (2, 3), (0, 3), (3, 6), (1, 1)):
        assert np.array_equal(bits(by_hand(a, b, wa, R, P, k, py, px)), bits(out[py, px])), (py, px)


def test_identities_of_the_rule():
    a, b, wa = halves(9, 13, 3)
    # R = 0: no filtering, whatever the patch
    for P in (0, 3):
        assert np.array_equal(bits(D.denoise(a, b, wa, 0, P, 0.7)[0]), bits(D.mix(a, b, wa)))
    assert np.array_equal(bits(D.denoise(a, b, None, 0, 0, 0.7)[0]), bits((a * f32(0.5)) + (b * f32(0.5))))
    # the weight at o = 0 is exactly 1, and weights lie in [0, 1]
    V = D.variance(a, b)
    assert (D.weight(D.patch_distance(b, V, 0, 0, 3, f32(0.49))) == 1).all()
    w = D.weight(D.patch_distance(b, V, 1, -2, 3, f32(0.49)))[:8, 2:]
    assert ((w >= 0) & (w <= 1)).all()
    # equal halves of a constant image: every weight 1, the output is the image
    flat = np.full((6, 8, 3), 0.375, f32)
    assert np.array_equal(bits(D.denoise(flat, flat.copy(), None, 3, 2, 0.7)[0]), bits(flat))
    # filtering brings noisy halves of a smooth image closer to it
    y, x = np.meshgrid(np.arange(24, dtype=f32), np.arange(32, dtype=f32), indexing="ij")
    clean = (f32(0.3) + f32(0.01) * x + f32(0.005) * y)[..., None] * np.ones(3, f32)
    rng = np.random.default_rng(1)
    na, nb = (clean + rng.normal(0, 0.05, clean.shape).astype(f32)).astype(f32), (clean + rng.normal(0, 0.05, clean.shape).astype(f32)).astype(f32)
    den = D.denoise(na, nb)[0]
    rmse = lambda im: float(np.sqrt(np.mean((im.astype(np.float64) - clean) ** 2)))
    assert rmse(den) < 0.5 * rmse(D.mix(na, nb))


def test_halves_from_samples():
    n, h, w = 7, 10, 19
    rng = np.random.default_rng(2)
    samples = rng.uniform(0, 1, (n, h, w, 3)).astype(f32)
    counts = np.array([[7, 4, 5], [2, 6, 7]], np.uint32)
    S, E = D.halves_from_samples(samples, counts)
    a, b, wa = D.halves(S, E, counts)
    for (y, x) in ((0, 0), (3, 9), (9, 18), (8, 2)):
        nt = int(counts[y // 8, x // 8])
        s = e = o = np.zeros(3, f32)
        for k in range(nt):
            s = s + samples[k, y, x]
            if k % 2 == 0:
                e = e + samples[k, y, x]
        hh = (nt + 1) // 2
        assert np.array_equal(bits(S[y, x]), bits(s)) and np.array_equal(bits(E[y, x]), bits(e))
        assert np.array_equal(bits(a[y, x]), bits(e * (f32(1) / f32(hh)))) and np.array_equal(bits(b[y, x]), bits((s - e) * (f32(1) / f32(nt - hh))))
        assert wa[y, x] == f32(hh) * (f32(1) / f32(nt))
    assert wa[0, 0] == f32(4) * (f32(1) / f32(7)) and wa[0, 8] == f32(0.5)


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_denoise_layout_matches_the_c_header(tmp_path):
    cname, cls = "rbrt_denoise_opts_t", abi.DenoiseOpts
    lines = [f'printf("{cname} %zu\\n", sizeof({cname}));'] + [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines.append('printf("tile %u\\n", RBRT_DENOISE_TILE);')
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip_debug.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "dn.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "dn"), str(tmp_path / "dn.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "dn")], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got[cname]) == C.sizeof(cls) == 16
    for f, _ in cls._fields_:
        assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f
    assert [f for f, _ in cls._fields_] == ["window_radius", "patch_radius", "strength", "reserved"]
    assert int(got["tile"]) >= 8
    lib = abi.load_hip()  # (raises if the library lacks a declared symbol)
    assert lib.rbrt_hip_abi_version() == 2
    assert len(abi.HIP_SYMBOLS["rbrt_hip_denoise_halves"][1]) == 10 and len(abi.HIP_SYMBOLS["rbrt_hip_scene_denoise"][1]) == 7
    d = abi.DenoiseOpts(9, 9, 9.0, 9)
    lib.rbrt_denoise_opts_default(C.byref(d))
    assert (d.window_radius, d.patch_radius, d.reserved) == (5, 3, 0) and d.strength == f32(0.7)
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    for text in ("int rbrt_hip_denoise_halves(", "int rbrt_hip_scene_denoise(", "multi-rank denoising is out of scope", "never faults"):
        assert text in header, text


def test_refusals_come_before_the_device_is_touched():
    """(no GPU here: a call that got as far as the device would answer RBRT_ERR_NO_DEVICE or RBRT_ERR_HIP)"""
    lib = abi.load_hip()
    one = (C.c_float * 3)(0.5, 0.5, 0.5)
    p = C.cast(one, C.c_void_p)
    ok = abi.DenoiseOpts(5, 3, 0.7, 0)
    rows = {"null a": (None, p, ok, 1, 1), "null b": (p, None, ok, 1, 1), "null opts": (p, p, None, 1, 1), "width 0": (p, p, ok, 0, 1),
            "height 0": (p, p, ok, 1, 0), "reserved": (p, p, abi.DenoiseOpts(5, 3, 0.7, 2), 1, 1), "R": (p, p, abi.DenoiseOpts(11, 3, 0.7, 0), 1, 1),
            "P": (p, p, abi.DenoiseOpts(5, 5, 0.7, 0), 1, 1), "nan": (p, p, abi.DenoiseOpts(5, 3, float("nan"), 0), 1, 1),
            "inf": (p, p, abi.DenoiseOpts(5, 3, float("inf"), 0), 1, 1), "zero": (p, p, abi.DenoiseOpts(5, 3, 0.0, 0), 1, 1),
            "negative": (p, p, abi.DenoiseOpts(5, 3, -1.0, 0), 1, 1)}
    for what, (a, b, o, w, h) in rows.items():
        rc = lib.rbrt_hip_denoise_halves(0, None, a, b, None, w, h, C.byref(o) if o is not None else None, p, None)
        assert rc == abi.RBRT_ERR_INVALID_ARG and lib.rbrt_hip_last_error(), (what, rc)
    assert lib.rbrt_hip_scene_denoise(None, C.byref(ok), None, None, None, None, None) == abi.RBRT_ERR_INVALID_ARG


def test_the_kernel_source_is_built_and_hashed():
    assert "rbrt_amd/csrc/denoise.hip" in srchash.KERNEL_SOURCES
    mk = (ROOT / "Makefile").read_text()
    assert len(re.findall(r"-shared -o \$@ [^\n]*\$\(CSRC\)/denoise\.hip", mk)) == 2  # both library rules
    assert "rbrt_amd/csrc/denoise.hip" in (ROOT / "tools" / "build_variant.sh").read_text()


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_denoise_help_and_refusals(tmp_path):
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--denoise  ", "--denoise-radius <r>", "--denoise-patch <p>", "--denoise-strength <k>", "--noisy <file>"):
        assert flag in r.stdout, flag
    for text in ("radius of the search window, 0 to 10 [default: 5]", "radius of the compared patches, 0 to 4 [default: 3]",
                 "larger smooths more [default: 0.7]", "--samples must be at least 2", "also write the unfiltered image there"):
        assert text in r.stdout, text
    out = ["-t", str(tmp_path / "x.png")]

    def refused(argv, *names):
        r = subprocess.run([str(EXE), *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and all(n in r.stderr for n in names), (argv, r.returncode, r.stderr)
        assert not (tmp_path / "x.png").exists()

    # every refusal of --adaptive, by name
    for argv, name in ((["--gpus", "2"], "--gpus > 1"), (["--checkpoint", str(tmp_path / "c.bin")], "--checkpoint"), (["--pass-samples", "4"], "--pass-samples")):
        refused(["--denoise", "-s", "8", *argv], "--denoise", name)
        refused(["--denoise", "--adaptive", "0.05", "-s", "8", *argv], name)
    refused(["--denoise", "--adaptive", "0.05", "--min-samples", "1", "-s", "8"], "--min-samples")
    refused(["--denoise", "--adaptive", "0.05", "--adaptive-step", "0", "-s", "8"], "--adaptive-step")
    refused(["--denoise", "--sample-map", str(tmp_path / "m.png"), "-s", "8"], "--sample-map", "--adaptive")
    # fewer than two samples: a half would be empty
    refused(["--denoise", "-s", "1"], "--denoise", "--samples")
    refused(["--denoise", "-s", "0"], "--denoise", "--samples")
    # the parameters' ranges
    for argv, name in ((["--denoise-radius", "11"], "--denoise-radius"), (["--denoise-radius", "-1"], "--denoise-radius"),
                       (["--denoise-radius", "x"], "--denoise-radius"), (["--denoise-patch", "5"], "--denoise-patch"),
                       (["--denoise-patch=1.5"], "--denoise-patch"), (["--denoise-strength", "0"], "--denoise-strength"),
                       (["--denoise-strength", "-0.7"], "--denoise-strength"), (["--denoise-strength", "nan"], "--denoise-strength"),
                       (["--denoise-strength", "inf"], "--denoise-strength"), (["--denoise-strength="], "--denoise-strength")):
        refused(["--denoise", "-s", "8", *argv], name)
    refused(["--denoise=1", "-s", "8"], "--denoise")
    # the parameters and --noisy without --denoise
    for argv, name in ((["--denoise-radius", "3"], "--denoise-radius"), (["--denoise-patch", "2"], "--denoise-patch"),
                       (["--denoise-strength", "0.5"], "--denoise-strength"), (["--noisy", str(tmp_path / "n.png")], "--noisy")):
        refused(["-s", "8", *argv], name, "--denoise")
    for flag in ("--denoise-radius", "--denoise-patch", "--denoise-strength", "--noisy"):  # a value is required
        assert subprocess.run([str(EXE), "--denoise", flag], capture_output=True, text=True).returncode == 2
