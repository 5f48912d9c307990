"""The numpy restatement of guided upsampling (np_upsample.py) pinned without a GPU: against a scalar evaluation of the rule
pixel by pixel, by the rule's stated consequences (the f = 1 identity, no light across a feature edge, zero-weight taps without
influence), the low camera's footprints in float64, the conditions the frozen inputs must meet for the GPU tests to mean
something, and its gain over plain bilinear upsampling on oracle renders."""
from __future__ import annotations

import math

import numpy as np
import pytest

import np_features
import np_upsample as NU
import scenes
import upsample_cases as UC
from rbrt_amd import abi

f32 = np.float32
MAIN = (50, 47)  # the main case's full size; its factors are 2..4


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def run(c, **kw):
    return NU.upsample(c.a, c.b, c.wa, c.rho, c.N, c.z, c.cov, factor=c.f, **kw)


# ---- 1. a scalar evaluation ------------------------------------------------------------------------------------------------------
def fmax(x, y):
    """C's fmaxf on float32 scalars."""
    if x != x:
        return y
    if y != y:
        return x
    return x if x > y else y


def scalar_upsample(a, b, wa, rho, N, z, cov, f, kn, kz, ka, flags):
    """The rule of rbrt_hip.h one pixel and one operation at a time, on float32 scalars."""
    H, W = z.shape
    w, h = (W + f - 1) // f, (H + f - 1) // f
    one, zero = f32(1), f32(0)
    kn, kz, ka = f32(kn), f32(kz), f32(ka)
    inv_n, inv_a, kz2, invf = one / (kn * kn), one / (ka * ka), kz * kz, one / f32(f)
    eps, floor = f32(1e-7), f32(0.01)
    low = {}
    for j in range(h):
        for i in range(w):
            s = [zero] * 8
            cnt = 0
            for y in range(j * f, min(j * f + f, H)):
                for x in range(i * f, min(i * f + f, W)):
                    vals = [rho[y, x, 0], rho[y, x, 1], rho[y, x, 2], N[y, x, 0], N[y, x, 1], N[y, x, 2], z[y, x], cov[y, x]]
                    s = [t + v for t, v in zip(s, vals)]
                    cnt += 1
            inv = one / f32(cnt)
            s = [t * inv for t in s]
            m = [fmax(s[k] + (one - s[7]), floor) for k in range(3)]
            u = [one if flags & 1 else m[k] for k in range(3)]
            low[j, i] = dict(a=[a[j, i, k] / u[k] for k in range(3)], b=[b[j, i, k] / u[k] for k in range(3)],
                             wa=f32(0.5) if wa is None else wa[j, i], n=s[3:6], z=s[6], m=m)
    A, B, wo = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32), np.zeros((H, W), f32)
    for R in range(H):
        for C in range(W):
            m = [fmax(rho[R, C, k] + (one - cov[R, C]), floor) for k in range(3)]
            u = [one if flags & 1 else m[k] for k in range(3)]
            xl = ((f32(C) + f32(0.5)) * invf) - f32(0.5)
            yl = ((f32(R) + f32(0.5)) * invf) - f32(0.5)
            i, j = math.floor(xl), math.floor(yl)
            fx, fy = xl - f32(i), yl - f32(j)
            gx, gy = one - fx, one - fy
            den, nw, na, nb = zero, zero, [zero] * 3, [zero] * 3
            for (qj, qi, bw) in ((j, i, gx * gy), (j, i + 1, fx * gy), (j + 1, i, gx * fy), (j + 1, i + 1, fx * fy)):
                q = low[min(max(qj, 0), h - 1), min(max(qi, 0), w - 1)]
                n = [q["n"][k] - N[R, C, k] for k in range(3)]
                Dn = (((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2])) * inv_n
                d = [q["m"][k] - m[k] for k in range(3)]
                Da = (((d[0] * d[0]) + (d[1] * d[1])) + (d[2] * d[2])) * inv_a
                dz = q["z"] - z[R, C]
                Dz = (dz * dz) / (eps + (kz2 * (z[R, C] * q["z"])))
                D = (Dn + Dz) + Da
                g = fmax(zero, one - f32(0.25) * fmax(D, zero))
                wt = bw * ((g * g) * (g * g))
                if wt > 0:
                    den = den + wt
                    na = [na[k] + wt * q["a"][k] for k in range(3)]
                    nb = [nb[k] + wt * q["b"][k] for k in range(3)]
                    nw = nw + wt * q["wa"]
            if den >= f32(0.01):
                for k in range(3):
                    A[R, C, k], B[R, C, k] = (na[k] / den) * u[k], (nb[k] / den) * u[k]
                wo[R, C] = nw / den
            else:
                q = low[R // f, C // f]
                for k in range(3):
                    A[R, C, k], B[R, C, k] = q["a"][k] * u[k], q["b"][k] * u[k]
                wo[R, C] = q["wa"]
    return A, B, wo


@pytest.mark.parametrize("f", [1, 2, 3, 4])
@pytest.mark.parametrize("W,H,row", [(13, 9, "defaults"), (7, 5, "flag"), (5, 1, "defaults"), (1, 6, "flag"), (1, 1, "defaults"), (12, 8, "tight")])
def test_the_restatement_equals_a_scalar_evaluation(W, H, f, row):
    kw = dict(defaults=dict(normal=0.5, depth=0.1, albedo=0.2, flags=0), flag=dict(normal=0.5, depth=0.1, albedo=0.2, flags=1),
              tight=dict(normal=0.2, depth=0.03, albedo=0.6, flags=0))[row]
    c = UC.case(W, H, f)
    wa = None if row == "flag" else c.wa
    with np.errstate(all="ignore"):
        ea, eb, ew = scalar_upsample(c.a, c.b, wa, c.rho, c.N, c.z, c.cov, f, kw["normal"], kw["depth"], kw["albedo"], kw["flags"])
    A, B, wo, _ = NU.upsample(c.a, c.b, wa, c.rho, c.N, c.z, c.cov, factor=f, **kw)
    assert same(A, ea) and same(B, eb) and same(wo, ew)


# ---- 2. the rule's consequences ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (13, 9), MAIN])
def test_factor_one_without_demodulation_is_the_identity(W, H):
    c = UC.case(W, H, 1)
    A, B, wo, info = run(c, flags=NU.NO_DEMODULATION)
    assert same(A, c.a) and same(B, c.b) and same(wo, c.wa) and not info.fallback.any()
    A, B, wo, _ = NU.upsample(c.a, c.b, None, c.rho, c.N, c.z, c.cov, factor=1, flags=NU.NO_DEMODULATION)
    assert same(A, c.a) and (wo == f32(0.5)).all()
    # with the albedo divided out and multiplied back it is the identity up to two roundings
    A, _, _, _ = run(c)
    assert np.allclose(A, c.a, rtol=3e-7, atol=0)


@pytest.mark.parametrize("f", [2, 3, 4])
def test_light_does_not_cross_the_albedo_edge(f):
    """The low pixels left of the albedo edge and across it get other values: on the ground right of the edge only fallback
    pixels whose own low pixel q0 was changed may change, and they are listed. The changed low pixels are among those pixels'
    taps -- with a positive bilinear weight and a zero weight -- so the claim is not empty."""
    c = UC.case(*MAIN, f)
    A, B, wo, info = run(c)
    changed = c.left | c.straddle
    a2, b2, w2 = c.a.copy(), c.b.copy(), c.wa.copy()
    a2[changed] *= f32(7.0)
    b2[changed] += f32(3.0)
    w2[changed] = f32(0.9)
    A2, B2, wo2, info2 = NU.upsample(a2, b2, w2, c.rho, c.N, c.z, c.cov, factor=f)
    right = (c.obj == 2) & (c.cov == 1) & (c.rho == np.asarray(UC.ALBEDO["right"], f32)).all(-1)
    assert right.sum() > 200
    listed = info.fallback & changed[info.q0]
    differs = (bits(A) != bits(A2)).any(-1) | (bits(B) != bits(B2)).any(-1) | (bits(wo) != bits(wo2))
    assert not (differs & right & ~listed).any(), np.argwhere(differs & right & ~listed)[:5]
    print(f"f = {f}: listed fallback pixels on the right: {np.argwhere(listed & right).tolist()}")
    tapped = np.zeros(c.z.shape, bool)   # pixels with a tap on a changed low pixel that has bilinear weight but no weight
    for (qy, qx), wt, bw in zip(info.taps, info.weights, info.bilinear):
        tapped |= changed[qy, qx] & (wt == 0) & (bw > 0)
    assert (tapped & right).sum() >= 10
    # ... and left of the edge everything changes
    left = (c.obj == 1) & (c.cov == 1) & (np.arange(c.W) < c.edge - f)[None, :]
    assert differs[left].all()


@pytest.mark.parametrize("f", [2, 3, 4])
def test_zero_weight_taps_have_no_influence(f):
    """NaN and infinities in low pixels that no accepted tap reaches: every pixel outside the listed ones (the fallback pixels
    whose q0 is planted) holds the clean run's bits."""
    c = UC.case(*MAIN, f)
    A, B, wo, info = run(c)
    a2, b2, w2, bad, listed = UC.planted(c, info)
    assert bad.sum() >= 2 and not np.isfinite(a2).all() and not np.isfinite(b2).all() and not np.isfinite(w2).all()
    A2, B2, wo2, info2 = NU.upsample(a2, b2, w2, c.rho, c.N, c.z, c.cov, factor=f)
    keep = ~listed
    assert same(A2[keep], A[keep]) and same(B2[keep], B[keep]) and same(wo2[keep], wo[keep])
    assert np.isfinite(A2[keep]).all() and 0 < listed.sum() < 0.05 * listed.size
    assert not (np.isfinite(A2[listed]).all() and np.isfinite(B2[listed]).all() and np.isfinite(wo2[listed]).all())


def test_both_halves_get_the_same_weights():
    """Swapping a and b swaps A and B; the weights never see the halves."""
    c = UC.case(*MAIN, 2)
    A, B, wo, info = run(c)
    B2, A2, _, info2 = NU.upsample(c.b, c.a, c.wa, c.rho, c.N, c.z, c.cov, factor=2)
    assert same(A, A2) and same(B, B2) and all(same(x, y) for x, y in zip(info.weights, info2.weights))


# ---- 3. the low camera --------------------------------------------------------------------------------------------------------------
def targets64(cam, rows, cols):
    """Pixel-centre targets on the image plane in float64 (camera_target with both jitter draws at 0.5)."""
    W, H = cam.img_width_pix, cam.img_height_pix
    c, r, u = (np.array(list(v), np.float64) for v in (cam.img_center_point, cam.right, cam.up))
    cm = (np.asarray(cols, np.float64) - (W // 2)) * float(cam.mm_per_pix_hor)
    rm = (np.asarray(rows, np.float64) - (H // 2)) * float(cam.mm_per_pix_vert)
    return c + (0.001 * cm)[..., None] * r - (0.001 * rm)[..., None] * u


@pytest.mark.parametrize("W,H,f", [(16, 8, 2), (15, 9, 2), (17, 7, 3), (16, 12, 4), (5, 5, 4)])
def test_the_low_cameras_pixels_cover_their_blocks(oracle, W, H, f):
    """The mean of the block's f x f pixel-centre targets (the whole block, also where it reaches beyond the image) equals the
    low pixel's centre target. The helper's rule makes each component of c' with 2 roundings for k, 2 for its scaling, 1 for the
    product with the axis and 1 for the sum, twice (right and up): 12 float32 roundings, each at most half an ulp of the largest
    coordinate involved; float(f) * mm_per_pix adds 1 rounding, relative, on an offset of at most max(w, h) / 2 low pixels."""
    cam = scenes.camera(oracle, W, H)
    low = NU.low_camera(cam, f)
    w, h = NU.low_size(W, H, f)
    assert (low.img_width_pix, low.img_height_pix) == (w, h)
    assert f32(low.mm_per_pix_hor) == f32(f) * f32(cam.mm_per_pix_hor)
    jj, ii = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    got = targets64(low, jj, ii)
    exp = targets64(cam, jj * f + (f - 1) / 2.0, ii * f + (f - 1) / 2.0)   # the mean of a regular block is its centre
    block = np.mean([targets64(cam, jj * f + dy, ii * f + dx) for dy in range(f) for dx in range(f)], axis=0)
    assert np.allclose(block, exp, rtol=0, atol=1e-12)
    biggest = max(abs(float(v)) for v in list(cam.img_center_point) + list(cam.position))
    ulp = float(np.spacing(f32(biggest)))
    extent = 0.001 * max(w, h) / 2 * float(low.mm_per_pix_hor) * max(np.linalg.norm(list(cam.right)), np.linalg.norm(list(cam.up)))
    tol = 12 * 0.5 * ulp + 2 * extent * 2.0 ** -24
    assert np.abs(got - exp).max() <= tol, (np.abs(got - exp).max(), tol)
    # ... which a camera that only scales the pixels misses by a good part of a pixel, unless W and H are multiples of 2 f
    naive = type(cam).from_buffer_copy(low)
    for k in range(3):
        naive.img_center_point[k] = cam.img_center_point[k]
    if f > 1:
        assert np.abs(targets64(naive, jj, ii) - exp).max() > 0.2 * 0.001 * float(cam.mm_per_pix_hor)


def test_the_low_camera_leaves_the_rest_alone(oracle):
    cam = scenes.camera(oracle, 50, 47)
    one = NU.low_camera(cam, 1)
    assert bytes(one) == bytes(cam)   # f = 1: k = 0 and the same camera, bit for bit
    low = NU.low_camera(cam, 3)
    assert list(low.position) == list(cam.position) and list(low.right) == list(cam.right) and list(low.up) == list(cam.up)


# ---- 4. conditions on the inputs -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 3, 4])
def test_the_main_case_takes_every_path(f):
    """Every count of accepted taps 0..4 occurs and the fallback share lies between 0.2 % and 20 %. Confirmed on the CPU for the
    frozen 50 x 47 case at the defaults: 3.11 % (f = 2), 4.00 % (f = 3), 5.70 % (f = 4)."""
    c = UC.case(*MAIN, f)
    A, B, wo, info = run(c)
    assert set(np.unique(info.count)) == {0, 1, 2, 3, 4}
    share = float(info.fallback.mean())
    print(f"f = {f}: fallback share {100 * share:.2f} %")
    assert 0.002 <= share <= 0.20
    assert (info.fallback & (info.count > 0)).any()   # too little weight, not none
    assert np.isfinite(A).all() and np.isfinite(B).all() and np.isfinite(wo).all()
    assert ((c.cov > 0) & (c.cov < 1)).sum() >= 40 and (c.cov == 0).any()   # partly covered pixels (the horizon's row), and sky
    # the demodulated low value differs per object
    d = c.truth / np.maximum(c.rho + (f32(1) - c.cov)[..., None], f32(0.01))
    means = [d[(c.obj == k) & ((c.cov == 1) | (k == 0))].mean(0) for k in range(4)]
    assert np.abs(means[0] - means[1]).max() > 0.1 and np.abs(means[1] - means[3]).max() > 0.05
    # the options matter
    for kw in (dict(flags=1), dict(normal=0.2, depth=0.03, albedo=0.6)):
        assert not same(run(c, **kw)[0], A)


def test_guided_beats_bilinear_on_the_synthetic_scene():
    for f in (2, 3, 4):
        c = UC.case(*MAIN, f)
        A, B, wo, _ = run(c)
        Ab, Bb, wb, ib = run(c, **NU.BILINEAR)
        assert ib.fallback.mean() < 0.01   # (not none: a depth of 0 against a hit is a distance no sigma lets through)
        assert UC.rmse(NU.mix(A, B, wo), c.truth) < 0.7 * UC.rmse(NU.mix(Ab, Bb, wb), c.truth)


# ---- 5. oracle renders ----------------------------------------------------------------------------------------------------------------
LOW_SPP, REF_SPP = 64, 256


def test_oracle_renders_upsampled_with_guides_beat_bilinear(oracle):
    """160 x 96, f = 2: the low halves are two oracle renders of the low camera at LOW_SPP samples with different seeds, the
    features np_features' at 4 samples of the full camera, the reference a full-size oracle render at REF_SPP with a third seed.
    Asserts only that the ratio of the RMSEs, guided over plain bilinear, is below 1; the measured figure is in DESIGN.md."""
    W, H, f = 160, 96, 2
    cam = scenes.camera(oracle, W, H)
    low = NU.low_camera(cam, f)
    sc = scenes.spheres_scene()
    a = oracle.render(low, sc, abi.default_opts(spp=LOW_SPP, seed=31))[0]
    b = oracle.render(low, sc, abi.default_opts(spp=LOW_SPP, seed=32))[0]
    ref = oracle.render(cam, sc, abi.default_opts(spp=REF_SPP, seed=33))[0]
    ft = np_features.features(oracle, cam, sc, abi.default_opts(spp=4, seed=31), 4)
    A, B, wo, info = NU.upsample(a, b, None, ft.albedo, ft.normal, ft.depth, ft.coverage, factor=f)
    Ab, Bb, wb, _ = NU.upsample(a, b, None, ft.albedo, ft.normal, ft.depth, ft.coverage, factor=f, **NU.BILINEAR)
    r_guided, r_plain = UC.rmse(NU.mix(A, B, wo), ref), UC.rmse(NU.mix(Ab, Bb, wb), ref)
    print(f"RMSE guided {r_guided:.5f}, bilinear {r_plain:.5f}, ratio {r_guided / r_plain:.3f}, fallback {100 * info.fallback.mean():.2f} %")
    assert np.isfinite(A).all() and r_guided < r_plain, (r_guided, r_plain)
