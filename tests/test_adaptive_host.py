"""Adaptive sampling without a GPU: the numpy restatement of the rule (np_adaptive.py) on synthetic sample arrays, the
layout of the two new structs against a host-compiled probe, and the CLI's refusals and help text."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import np_adaptive as A
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32


def noisy(n, h, w, seed, quiet_rows=0):
    """n samples of an h x w image: noise of amplitude 1 around 1, except `quiet_rows` rows at the top with amplitude 1e-4."""
    rng = np.random.default_rng(seed)
    amp = np.ones((h, w, 1), f32)
    amp[:quiet_rows] = f32(1e-4)
    return (f32(1.0) + amp * rng.uniform(-1.0, 1.0, (n, h, w, 3)).astype(f32)).astype(f32)


def sequential_mean(samples, n):
    s = np.zeros_like(samples[0])
    for k in range(n):
        s = s + samples[k]
    return s * (f32(1.0) / f32(n))


# ---- the rule ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mn,step", [(12, 4, 4), (11, 4, 3), (7, 16, 16), (13, 2, 5), (5, 4, 1)])
def test_threshold_zero_and_a_huge_threshold(n, mn, step):
    s = noisy(n, 21, 37, n)
    r = A.adaptive(s, 0.0, mn, step)
    n0 = min(mn, n)
    assert (r.counts == n).all() and r.samples == r.samples_fixed == 21 * 37 * n
    assert r.rounds == 1 + -(-(n - n0) // step)  # (step need not divide N - n_0: the last round is shorter)
    assert np.array_equal(r.image.view(np.uint32), sequential_mean(s, n).view(np.uint32))
    assert r.round_active == [15] * r.rounds
    big = A.adaptive(s, 1e30, mn, step)
    assert (big.counts == n0).all() and big.rounds == 1 and big.samples == 21 * 37 * n0
    assert np.array_equal(big.image.view(np.uint32), sequential_mean(s, n0).view(np.uint32))
    assert np.array_equal(big.errors.view(np.uint32), r.round_errors[0].view(np.uint32))  # round 0 does not depend on the threshold


def test_tiles_stop_one_by_one_and_keep_the_fixed_render_of_their_count():
    n, mn, step, h, w = 11, 4, 3, 21, 37  # odd N, a step that does not divide N - n_0, ragged both ways
    s = noisy(n, h, w, 3, quiet_rows=8)
    r0 = A.adaptive(s, 0.0, mn, step)
    e0 = r0.round_errors[0]
    thr = float(f32(0.6) * e0[1:].min())  # below every noisy tile's first error, far above the quiet row's
    assert e0[0].max() < 0.01 * thr
    r = A.adaptive(s, thr, mn, step)
    assert (r.counts[0] == mn).all() and (r.counts[1:] > mn).all()  # the quiet tile row stops at once, the others go on
    assert set(np.unique(r.counts)) <= {4, 7, 10, 11} and len(np.unique(r.counts)) >= 2
    ty, tx = np.meshgrid(np.arange(h) // 8, np.arange(w) // 8, indexing="ij")
    for c in np.unique(r.counts):
        m = r.counts[ty, tx] == c
        assert np.array_equal(r.image[m].view(np.uint32), sequential_mean(s, int(c))[m].view(np.uint32))
    assert r.samples == int((r.counts[ty, tx].astype(np.int64)).sum()) and r.samples_fixed == h * w * n
    assert r.round_active[0] == 15 and r.round_active == sorted(r.round_active, reverse=True)
    # a stopped tile keeps the error it stopped with; a tile that reached N has the error of N samples
    e_n = A.tile_error(*sums(s, n), n)
    at_n = r.counts == n
    assert np.array_equal(r.errors[at_n].view(np.uint32), e_n[at_n].view(np.uint32))
    stopped = r.counts == mn
    assert (r.errors[stopped] < f32(thr)).all()
    assert np.array_equal(r.errors[stopped].view(np.uint32), r0.round_errors[0][stopped].view(np.uint32))


def sums(samples, n):
    s, e = np.zeros_like(samples[0]), np.zeros_like(samples[0])
    for k in range(n):
        s = s + samples[k]
        if k % 2 == 0:
            e = e + samples[k]
    return s, e


def test_tile_error_by_hand():
    """One whole tile and one ragged one (a 3 x 2 corner), each pixel computed with scalars in the rule's order."""
    n, h, w = 5, 10, 11
    s = noisy(n, h, w, 9)
    S, E = sums(s, n)
    got = A.tile_error(S, E, n)
    assert got.shape == (2, 2) and got.dtype == f32
    inv_n, inv_h = f32(1.0) / f32(5), f32(1.0) / f32(3)
    for ty, tx in ((0, 0), (1, 1)):
        q = np.zeros(64, f32)
        inside = 0
        for p in range(64):
            y, x = ty * 8 + p // 8, tx * 8 + p % 8
            if y >= h or x >= w:
                continue
            inside += 1
            I = [f32(S[y, x, c] * inv_n) for c in range(3)]
            a = [f32(E[y, x, c] * inv_h) for c in range(3)]
            e = f32(f32(abs(I[0] - a[0]) + abs(I[1] - a[1])) + abs(I[2] - a[2]))
            q[p] = e / f32(np.sqrt(f32(f32(I[0] + I[1]) + I[2])) + f32(0.0001))
        v = q.copy()
        for d in (1, 2, 4, 8, 16, 32):
            v = np.array([f32(v[p] + v[p ^ d]) for p in range(64)], f32)
        assert len(set(v.view(np.uint32).tolist())) == 1
        assert inside == (64 if (ty, tx) == (0, 0) else 6)
        assert f32(v[0] / f32(inside)).view(np.uint32) == got[ty, tx].view(np.uint32)


def test_nan_samples_keep_a_tile_active():
    n, mn, step = 12, 4, 4
    s = noisy(n, 16, 16, 4)
    s[1, 9, 3, 1] = np.nan  # one pixel of tile (1, 0), in the first round
    r = A.adaptive(s, 1e30, mn, step)
    assert r.counts[1, 0] == n and np.isnan(r.errors[1, 0])  # never below any threshold: sampled to the limit
    assert (np.delete(r.counts.ravel(), 2) == mn).all()
    assert r.rounds == 3 and r.round_active == [4, 1, 1]
    assert np.isnan(r.image[9, 3, 1]) and r.rgb8[9, 3, 1] == 0 and np.isfinite(r.image[9, 3, 0])
    # an infinite sample: inf - inf is NaN, too
    s = noisy(n, 16, 16, 4)
    s[0, 0, 0, 0] = np.inf
    assert A.adaptive(s, 1e30, mn, step).counts[0, 0] == n


def test_quantise_and_sample_map():
    c = np.array([0.0, 1.0, 0.25, 4.0, -1.0, np.nan, np.inf, 0.9921], f32)
    assert A.quantise(c).tolist() == [0, 255, 128, 255, 0, 0, 255, 254]
    counts = np.array([[4, 12], [8, 11]], np.uint32)
    m = A.sample_map(counts, 10, 12, 12)
    assert m.shape == (10, 12) and m[0, 0] == 85 and m[0, 11] == 255 and m[9, 0] == 170 and m[9, 9] == 233
    assert A.per_rank(np.arange(6).reshape(2, 3)).tolist() == [0, 1, 2, 3, 4, 5]  # (three tiles a row: the skew of 3 is a whole turn)
    assert sorted(A.per_rank(np.arange(10).reshape(2, 5), 0, 3).tolist() + A.per_rank(np.arange(10).reshape(2, 5), 1, 3).tolist() +
                  A.per_rank(np.arange(10).reshape(2, 5), 2, 3).tolist()) == list(range(10))


# ---- the ABI -----------------------------------------------------------------------------------------------------------------
def test_adaptive_layout_matches_the_c_header(tmp_path):
    structs = {"rbrt_adaptive_opts_t": abi.AdaptiveOpts, "rbrt_adaptive_result_t": abi.AdaptiveResult}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "ad.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "ad"), str(tmp_path / "ad.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "ad")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert C.sizeof(abi.AdaptiveOpts) == 16 and C.sizeof(abi.AdaptiveResult) == 24
    assert [f for f, _ in abi.AdaptiveOpts._fields_] == ["threshold", "min_samples", "step", "reserved"]
    assert [f for f, _ in abi.AdaptiveResult._fields_] == ["rounds", "reserved", "samples", "samples_fixed"]
    lib = abi.load_hip()  # (raises if the library lacks a declared symbol)
    assert lib.rbrt_hip_abi_version() == 2
    assert "rbrt_hip_render_adaptive" in abi.HIP_SYMBOLS and len(abi.HIP_SYMBOLS["rbrt_hip_render_adaptive"][1]) == 10
    assert "rbrt_hip_scene_adaptive_rounds" in abi.DEBUG_SYMBOLS
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "int rbrt_hip_render_adaptive(" in header and "THIS CALL BLOCKS" in header


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def test_cli_adaptive_help_and_refusals(tmp_path):
    assert EXE.exists(), "build the CLI with `make`"
    r = subprocess.run([str(EXE), "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--adaptive <threshold>", "--min-samples <n>", "--adaptive-step <k>", "--sample-map <file>"):
        assert flag in r.stdout, flag
    assert "samples of the first round, at least 2 [default: 16]" in r.stdout
    assert "samples of every later round, at least 1 [default: 64]" in r.stdout
    assert "Cannot be combined with --gpus > 1, --checkpoint or --pass-samples" in r.stdout
    out = ["-t", str(tmp_path / "x.png")]
    for argv, name in ((["--gpus", "2"], "--gpus > 1"), (["--checkpoint", str(tmp_path / "c.bin")], "--checkpoint"),
                       (["--pass-samples", "4"], "--pass-samples")):
        r = subprocess.run([str(EXE), "--adaptive", "0.05", *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and "--adaptive" in r.stderr and name in r.stderr, (argv, r.returncode, r.stderr)
        assert not (tmp_path / "x.png").exists()
    for bad in ("nan", "inf", "-0.1", "x", ""):
        r = subprocess.run([str(EXE), f"--adaptive={bad}", *out], capture_output=True, text=True)
        assert r.returncode == 2 and "--adaptive" in r.stderr, (bad, r.stderr)
    for argv in (["--min-samples", "1"], ["--min-samples", "0"], ["--adaptive-step", "0"], ["--min-samples", "-3"]):
        r = subprocess.run([str(EXE), "--adaptive", "0.05", *argv, *out], capture_output=True, text=True)
        assert r.returncode == 2 and ("--min-samples" in r.stderr or "--adaptive-step" in r.stderr), (argv, r.stderr)
    r = subprocess.run([str(EXE), "--sample-map", str(tmp_path / "m.png"), *out], capture_output=True, text=True)
    assert r.returncode == 2 and "--sample-map" in r.stderr and "--adaptive" in r.stderr
    r = subprocess.run([str(EXE), "--adaptive"], capture_output=True, text=True)
    assert r.returncode == 2
