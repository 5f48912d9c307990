"""The numpy restatement of the spike removal (np_despike.py) pinned without a GPU: against a second evaluation of the rule,
pixel by pixel with float32 scalars and a sort, that shares no code with it; by every consequence include/rbrt_hip.h lists; by
the branches the frozen case takes; and by what the stage is for: on oracle renders of a scene with a small, very bright
emitter the despiked image is closer to a converged one, as a plain mix and behind the guided filter.

Measured by the oracle test (relMSE = mean(|x - ref|^2 / (|ref|^2 + 0.01)); 160 x 96, seeds 31, 32; reference 8192 spp, seed 33):
   8 spp a half: plain mix RMSE 5.0312 -> 4.9801, relMSE 10.6739 -> 0.0261; guided RMSE 6.2245 -> 6.2192, relMSE 1.4148 -> 0.0233;
                 flagged 4 in A, 7 in B; image mean 0.8271 -> 0.8156 (reference 0.8883)
  32 spp a half: plain mix RMSE 2.3660 -> 2.3379, relMSE 2.8594 -> 0.0280; guided RMSE 5.4549 -> 5.4528, relMSE 0.3834 -> 0.0244;
                 flagged 18 in A, 23 in B; image mean 0.8711 -> 0.8594 (reference 0.8883)"""
import functools

import numpy as np
import pytest

import despike_cases as DC
import np_despike as ND
import np_features
import np_guided
import scenes
from rbrt_amd import abi

f32 = np.float32
ROWS = {"defaults": {}, "R1 k1": dict(radius=1, rank=1), "R2 k4": dict(radius=2, rank=4), "R1 k4": dict(radius=1, rank=4),
        "R2 k3": dict(radius=2, rank=3), "t1 f0": dict(threshold=1.0, floor=0.0), "t1e6": dict(threshold=1e6)}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(x, y):
    return np.array_equal(bits(x), bits(y))


# ---- 1. an independent evaluator ------------------------------------------------------------------------------------------------
def scalar_despike(A, B, radius, rank, threshold, floor):
    """include/rbrt_hip.h "Spike removal" one pixel and one operation at a time, np.float32 scalars throughout; the k-th largest
    by sorting the multiset the header names (the finite neighbours inside the image as they are, negative ones too, and k
    zeros), not by the restatement's chain."""
    H, W, _ = A.shape
    t, f, maxf, zero = f32(threshold), f32(floor), f32(3.4028235e38), f32(0)

    def fin(x):
        return bool(x <= maxf and x >= -maxf)

    def Y(c):
        return ((f32(0.2126) * c[0]) + (f32(0.7152) * c[1])) + (f32(0.0722) * c[2])

    out = [A.copy(), B.copy()]
    mask = np.zeros((H, W), np.uint8)
    with np.errstate(all="ignore"):
        for h, (X, O) in enumerate(((A, B), (B, A))):
            for y_ in range(H):
                for x_ in range(W):
                    y, yo = Y(X[y_, x_]), Y(O[y_, x_])
                    values = [zero] * rank
                    for dy in range(-radius, radius + 1):
                        for dx in range(-radius, radius + 1):
                            qy, qx = y_ + dy, x_ + dx
                            if (dy or dx) and 0 <= qy < H and 0 <= qx < W:
                                v = Y(X[qy, qx])
                                if fin(v):
                                    values.append(v)
                    r = sorted(values, reverse=True)[rank - 1]
                    r = zero if r == 0 else r                       # (a -0 neighbour that ties with the zeros: the header's zeros are +0)
                    other = yo if fin(yo) and yo > 0 else zero
                    base = r if r >= other else other
                    lim = (t * base) + f
                    lim = lim if lim <= maxf else maxf
                    if not fin(y):
                        out[h][y_, x_] = lim
                        mask[y_, x_] |= 1 << h
                    elif y > lim:
                        s = lim / y
                        for c in range(3):
                            out[h][y_, x_, c] = X[y_, x_, c] * s
                        mask[y_, x_] |= 1 << h
    return out[0], out[1], mask


@pytest.mark.parametrize("row", list(ROWS))
def test_the_restatement_equals_a_scalar_evaluation_on_the_main_case(row):
    c = DC.case(*DC.MAIN, nonfinite=True)
    p = dict(ND.DEFAULTS, **ROWS[row])
    ea, eb, em = scalar_despike(c.a, c.b, **p)
    ga, gb, gm, counts, _ = ND.despike(c.a, c.b, **p)
    assert same(ga, ea) and same(gb, eb) and np.array_equal(gm, em)
    assert counts == (int((em & 1).sum()), int((em >> 1).sum()))


@pytest.mark.parametrize("w,h", [s for s in DC.SIZES if s != DC.MAIN], ids=lambda v: str(v))
def test_the_restatement_equals_a_scalar_evaluation_at_every_size(w, h):
    for nonfinite in (False, True):
        c = DC.case(w, h, nonfinite)
        for row in ("defaults", "R1 k1", "R1 k4"):
            p = dict(ND.DEFAULTS, **ROWS[row])
            ea, eb, em = scalar_despike(c.a, c.b, **p)
            ga, gb, gm, _, _ = ND.despike(c.a, c.b, **p)
            assert same(ga, ea) and same(gb, eb) and np.array_equal(gm, em), (w, h, nonfinite, row)


# ---- 2. the consequences the header states ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def main_result(row="defaults", nonfinite=True):
    c = DC.case(*DC.MAIN, nonfinite=nonfinite)
    return c, ND.despike(c.a, c.b, **dict(ND.DEFAULTS, **ROWS[row]))


@pytest.mark.parametrize("row", list(ROWS))
def test_unflagged_pixels_pass_bit_for_bit_and_flagged_ones_come_out_finite(row):
    c, (oa, ob, mask, counts, info) = main_result(row)
    fa, fb = (mask & 1) != 0, (mask & 2) != 0
    assert same(oa[~fa], c.a[~fa]) and same(ob[~fb], c.b[~fb])
    assert np.isfinite(oa[fa]).all() and np.isfinite(ob[fb]).all()
    assert np.isfinite(oa).all() and np.isfinite(ob).all()   # ... so the whole image is: what is not finite is flagged
    assert counts == (int(fa.sum()), int(fb.sum())) and (mask <= 3).all()
    assert np.array_equal(ND.spike_map(mask), np.array([0, 85, 170, 255], np.uint8)[mask])


def test_the_main_case_takes_every_branch():
    c, (oa, ob, mask, counts, info) = main_result()
    for i in (info.a, info.b):
        assert i.above.sum() >= 10 and i.nonfinite.sum() >= 2        # flagged for y > lim; flagged for not finite
        assert i.kept_by_other.sum() >= 1 and i.kept_by_rank.sum() >= 3  # kept by the other half alone; by the rank alone
    assert set(np.unique(mask)) == {0, 1, 2, 3}
    assert (c.spikes_a & ~(mask & 1).astype(bool)).any() and (c.spikes_a & (mask & 1).astype(bool)).any()
    # t * base overflows somewhere with k = 1, and the limit is MAXF there
    _, (_, _, _, _, info1) = main_result("R1 k1")
    assert (info1.a.lim == ND.MAXF).any()


def test_a_result_depends_only_on_its_window_and_the_other_halfs_pixel():
    c = DC.case(*DC.MAIN)
    H, W = c.H, c.W
    rng = np.random.default_rng(3)
    for R in (1, 2):
        oa, ob, mask, _, _ = ND.despike(c.a, c.b, radius=R)
        for _ in range(6):
            y, x = int(rng.integers(H)), int(rng.integers(W))
            a2, b2 = rng.uniform(0, 5000, c.a.shape).astype(f32), rng.uniform(0, 5000, c.b.shape).astype(f32)
            ys, xs = slice(max(0, y - R), y + R + 1), slice(max(0, x - R), x + R + 1)
            a2[ys, xs] = c.a[ys, xs]        # A's window and B's pixel are kept; everything else is noise
            b2[y, x] = c.b[y, x]
            pa, _, pm, _, _ = ND.despike(a2, b2, radius=R)
            assert same(pa[y, x], oa[y, x]) and (pm[y, x] & 1) == (mask[y, x] & 1)


def test_a_value_both_halves_hold_is_never_flagged():
    rng = np.random.default_rng(4)
    x = (rng.uniform(0, 1, (20, 30, 3)) * (rng.uniform(0, 1, (20, 30, 1)) < 0.2) * 5000).astype(f32)
    x[3, 3] = -1.0
    for p in ({}, dict(threshold=1.0, floor=0.0), dict(radius=1, rank=4)):
        oa, ob, mask, counts, _ = ND.despike(x, x.copy(), **dict(ND.DEFAULTS, **p))
        assert counts == (0, 0) and not mask.any() and same(oa, x) and same(ob, x)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("R", [1, 2])
def test_a_cluster_of_k_plus_one_survives_and_a_cluster_of_k_does_not(R, k):
    base = np.full((12, 12, 3), 0.2, f32)
    for n, survives in ((k + 1, True), (k, False)):
        a = base.copy()
        if n == 5 and R == 1:
            continue                # (five pixels are mutually adjacent only within 3 x 3: R = 2)
        cells = DC.CLUSTERS[n]      # (within 2 x 2 up to four, within 2 x 3 with the fifth)
        for dy, dx in cells:
            a[5 + dy, 5 + dx] = DC.SPIKE
        oa, _, mask, counts, _ = ND.despike(a, base, radius=R, rank=k)
        assert (counts[0] == 0) == survives and counts[1] == 0, (R, k, n, counts)
        if survives:
            assert same(oa, a)
        else:
            assert counts[0] == n and float(oa.max()) < 5.0


@pytest.mark.parametrize("row", list(ROWS))
def test_swapping_the_halves_swaps_the_results(row):
    c, (oa, ob, mask, counts, _) = main_result(row)
    sa, sb, sm, sc, _ = ND.despike(c.b, c.a, **dict(ND.DEFAULTS, **ROWS[row]))
    assert same(sa, ob) and same(sb, oa) and sc == counts[::-1]
    assert np.array_equal(sm, ((mask & 1) << 1) | (mask >> 1))


def test_with_nothing_flagged_the_call_is_the_identity():
    for w, h in DC.SIZES:
        c = DC.case(w, h)
        oa, ob, mask, counts, _ = ND.despike(c.a, c.b, threshold=1e6)
        assert counts == (0, 0) and not mask.any() and same(oa, c.a) and same(ob, c.b), (w, h)
        assert ND.despike(c.a, c.b)[3] != (0, 0) or w * h < 23, (w, h)   # (the defaults do flag something in it, where a window is not the whole image)


# ---- 3. what it is for -----------------------------------------------------------------------------------------------------------
def rel_mse(x, ref):
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.mean(((x - ref) ** 2).sum(-1) / ((ref ** 2).sum(-1) + 0.01)))


def rmse(x, ref):
    return float(np.sqrt(np.mean((np.asarray(x, np.float64) - np.asarray(ref, np.float64)) ** 2)))


@functools.lru_cache(maxsize=None)
def emitter_scene(oracle):
    """scenes.EXAMPLE_SPHERES and a small, very bright emitter under the default sky; the converged reference."""
    W, H = 160, 96
    cam = scenes.camera(oracle, W, H)
    light = ((2.0, 6.0, -8.0), 0.08, abi.material(abi.MAT_EMISSIVE, (3000.0, 2700.0, 2100.0)))
    sc = scenes.spheres_scene(scenes.EXAMPLE_SPHERES + [light])
    ref = oracle.render(cam, sc, abi.default_opts(spp=8192, seed=33))[0]
    ref.flags.writeable = False
    return cam, sc, ref


@pytest.mark.parametrize("spp", [8, 32])
def test_oracle_renders_with_a_small_bright_emitter_get_closer_to_a_converged_one(oracle, spp):
    cam, sc, ref = emitter_scene(oracle)
    A = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=31))[0]
    B = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=32))[0]
    ft = np_features.features(oracle, cam, sc, abi.default_opts(spp=spp, seed=31), 4)
    half = f32(0.5)
    A2, B2, mask, counts, _ = ND.despike(A, B)
    plain, plain2 = (A * half) + (B * half), (A2 * half) + (B2 * half)
    guided = np_guided.denoise(A, B, None, ft.albedo, ft.normal, ft.depth, ft.coverage)[0]
    guided2 = np_guided.denoise(A2, B2, None, ft.albedo, ft.normal, ft.depth, ft.coverage)[0]
    print(f"{spp} spp a half: plain mix RMSE {rmse(plain, ref):.4f} -> {rmse(plain2, ref):.4f}, relMSE {rel_mse(plain, ref):.4f} -> "
          f"{rel_mse(plain2, ref):.4f}; guided RMSE {rmse(guided, ref):.4f} -> {rmse(guided2, ref):.4f}, relMSE {rel_mse(guided, ref):.4f} -> "
          f"{rel_mse(guided2, ref):.4f}; flagged {counts[0]} in A, {counts[1]} in B; mean {plain.mean():.4f} -> {plain2.mean():.4f}, ref {ref.mean():.4f}")
    assert np.isfinite(plain2).all() and np.isfinite(guided2).all()
    assert rmse(plain2, ref) < rmse(plain, ref)
    assert rel_mse(plain2, ref) < rel_mse(plain, ref)
    assert rel_mse(guided2, ref) < rel_mse(guided, ref)
