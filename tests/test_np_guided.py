"""The numpy restatement of the guided denoiser (np_guided.py) pinned without a GPU: against a second evaluation of the rule,
pixel by pixel with float32 scalars, that shares no code with it; by an exact property (light does not cross a feature edge);
at the limits of the rule; and by what it is for: the filtered image is closer to the truth than the noisy one, on the synthetic
scene the rule was prototyped on and on oracle renders of the spheres scene."""
import numpy as np
import pytest

import guided_cases as GC
import np_features
import np_guided as G
import scenes
from rbrt_amd import abi

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- 1. an independent evaluator ------------------------------------------------------------------------------------------------
def scalar_guided(A, B, wa, rho, N, z, cov, levels, colour, normal, depth, albedo, flags):
    """include/rbrt_hip.h "Guided denoising" one pixel and one operation at a time, np.float32 scalars throughout."""
    H, W, _ = A.shape
    one, zero = f32(1), f32(0)
    eps, floor = f32(1e-7), f32(0.01)
    kc, kn, kz, ka = f32(colour), f32(normal), f32(depth), f32(albedo)
    kc2, kz2, inv_n, inv_a = kc * kc, kz * kz, one / (kn * kn), one / (ka * ka)
    m = [[[max(rho[y, x, c] + (one - cov[y, x]), floor) for c in range(3)] for x in range(W)] for y in range(H)]
    u = [[[one if flags & 1 else m[y][x][c] for c in range(3)] for x in range(W)] for y in range(H)]
    a = [[[A[y, x, c] / u[y][x][c] for c in range(3)] for x in range(W)] for y in range(H)]
    b = [[[B[y, x, c] / u[y][x][c] for c in range(3)] for x in range(W)] for y in range(H)]
    I = [[[None] * 3 for _ in range(W)] for _ in range(H)]
    V = [[[None] * 3 for _ in range(W)] for _ in range(H)]
    for y in range(H):
        for x in range(W):
            w_a = f32(0.5) if wa is None else wa[y, x]
            for c in range(3):
                I[y][x][c] = (a[y][x][c] * w_a) + (b[y][x][c] * (one - w_a))
                total, count = zero, 0
                for dy in (-1, 0, 1):
                    for dx in (-1, 0, 1):
                        if 0 <= y + dy < H and 0 <= x + dx < W:
                            d = a[y + dy][x + dx][c] - b[y + dy][x + dx][c]
                            total = total + d * d
                            count += 1
                V[y][x][c] = (total / f32(count)) * f32(0.25)
    h5 = [f32(0.0625), f32(0.25), f32(0.375), f32(0.25), f32(0.0625)]
    for l in range(levels):
        s = 1 << l
        I2 = [[[None] * 3 for _ in range(W)] for _ in range(H)]
        V2 = [[[None] * 3 for _ in range(W)] for _ in range(H)]
        for y in range(H):
            for x in range(W):
                num, nv, den = [zero] * 3, [zero] * 3, zero
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        qy, qx = y + j * s, x + i * s
                        if not (0 <= qy < H and 0 <= qx < W):
                            continue
                        hh = h5[j + 2] * h5[i + 2]
                        n = [N[qy, qx, c] - N[y, x, c] for c in range(3)]
                        Dn = (((n[0] * n[0]) + (n[1] * n[1])) + (n[2] * n[2])) * inv_n
                        e = [m[qy][qx][c] - m[y][x][c] for c in range(3)]
                        Da = (((e[0] * e[0]) + (e[1] * e[1])) + (e[2] * e[2])) * inv_a
                        dz = z[qy, qx] - z[y, x]
                        Dz = (dz * dz) / (eps + (kz2 * (z[y, x] * z[qy, qx])))
                        t = []
                        for c in range(3):
                            g = I[qy][qx][c] - I[y][x][c]
                            t.append((g * g) / (eps + (kc2 * (V[y][x][c] + V[qy][qx][c]))))
                        Dc = ((t[0] + t[1]) + t[2]) * f32(0.33333334)
                        D = ((Dn + Dz) + Da) + Dc
                        f = max(zero, one - f32(0.25) * max(D, zero))
                        w = hh * ((f * f) * (f * f))
                        for c in range(3):
                            num[c] = num[c] + w * I[qy][qx][c]
                            nv[c] = nv[c] + (w * w) * V[qy][qx][c]
                        den = den + w
                for c in range(3):
                    I2[y][x][c] = num[c] / den
                    V2[y][x][c] = nv[c] / (den * den)
        I, V = I2, V2
    out = np.zeros((H, W, 3), f32)
    for y in range(H):
        for x in range(W):
            for c in range(3):
                v = I[y][x][c] * u[y][x][c]
                assert type(v) is f32
                out[y, x, c] = v
    return out


@pytest.mark.parametrize("w,h,levels", [(9, 7, 2), (5, 3, 6)])
@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("use_wa", [True, False])
def test_the_restatement_is_the_scalar_evaluation(w, h, levels, flags, use_wa):
    A, B, wa, rho, N, z, cov = GC.synthetic(w, h)
    wa = wa if use_wa else None
    p = dict(levels=levels, colour=2.0, normal=0.35, depth=0.05, albedo=0.1, flags=flags)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        exp = scalar_guided(A, B, wa, rho, N, z, cov, **p)
    got, got8 = G.denoise(A, B, wa, rho, N, z, cov, **p)
    assert np.isfinite(exp).all()
    assert np.array_equal(bits(got), bits(exp)), int((bits(got) != bits(exp)).sum())
    assert np.array_equal(got8, G.quantise(exp))


def test_the_weights_of_the_synthetic_inputs_are_not_all_0_or_1():
    """A condition on the inputs the GPU tests share: at the defaults, taps one pixel to the right have weights strictly
    between, weights of exactly 0 (across the checker's and the normal's steps) and weights near the B-spline's own."""
    A, B, wa, rho, N, z, cov = GC.synthetic(37, 21)
    m, u, I, V = G.prepare(A, B, wa, rho, cov)
    kc2, kz2, inv_n, inv_a = G.constants(2.0, 0.35, 0.05, 0.1)
    pr = G._pairs(21, 37, 0, 1)
    w = G.tap_weight(N, z, m, I, V, pr, f32(1), kc2, kz2, inv_n, inv_a)
    assert ((w > 0.01) & (w < 0.99)).sum() > 100 and (w == 0).any() and (w > 0.9).any(), np.histogram(w, 10, (0, 1))[0]


# ---- 2. light does not cross a feature edge ---------------------------------------------------------------------------------------
def edge_case(kind, W=70, H=40, col=33):
    rng = np.random.default_rng(5)
    A = (rng.integers(1, 1024, (H, W, 3)).astype(f32) * f32(2.0 ** -10)).astype(f32)
    B = (rng.integers(1, 1024, (H, W, 3)).astype(f32) * f32(2.0 ** -10)).astype(f32)
    rho = np.full((H, W, 3), 0.5, f32)
    N = np.zeros((H, W, 3), f32)
    N[..., 2] = 1
    z = np.full((H, W), 4.0, f32)
    if kind == "albedo":
        rho[:, col:] = f32(0.75)     # Da = 3 * 0.0625 * 100 = 18.75
    elif kind == "normal":
        N[:, col:] = (1, 0, 0)       # Dn = 2 / 0.1225 = 16.3
    else:
        z[:, col:] = f32(8.0)        # Dz = 16 / (0.0025 * 32) = 200
    return A, B, rho, N, z, np.ones((H, W), f32), col


@pytest.mark.parametrize("kind", ["albedo", "normal", "depth"])
def test_light_does_not_cross_a_feature_edge(kind):
    """Without demodulation nothing of a pixel's left side depends on the right side once a feature term alone is >= 4: adding
    4.0 to every colour right of the edge leaves every bit left of it, at the widest filter."""
    A, B, rho, N, z, cov, col = edge_case(kind)
    p = dict(G.DEFAULTS, levels=6, flags=G.NO_DEMODULATION)
    base, _ = G.denoise(A, B, None, rho, N, z, cov, **p)
    A2, B2 = A.copy(), B.copy()
    A2[:, col:] += f32(4.0)
    B2[:, col:] += f32(4.0)
    lit, _ = G.denoise(A2, B2, None, rho, N, z, cov, **p)
    assert np.array_equal(bits(base[:, :col]), bits(lit[:, :col]))
    assert (lit[:, col:] > base[:, col:] + 3.9).all()                   # ... and the light stays where it was put
    smooth, _ = G.denoise(A, B, None, np.full_like(rho, 0.5), np.broadcast_to(f32([0, 0, 1]), N.shape).copy(), np.full_like(z, 4.0),
                          cov, **p)
    assert not np.array_equal(bits(base[:, col - 3:col]), bits(smooth[:, col - 3:col]))  # (without the edge the sides do mix)


# ---- 3. the limits ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
def test_outputs_are_finite_at_the_limits(flags):
    """|A|, |B| up to 1e6 with m at its floor (albedo 0 under full coverage): I reaches 1e8, g * g 1e16."""
    H, W = 24, 40
    rng = np.random.default_rng(9)
    A = rng.choice(f32([1e6, 1e-6, 0.0, 3e5]), (H, W, 3)).astype(f32)
    B = rng.choice(f32([1e6, 1e-6, 0.0, 7e5]), (H, W, 3)).astype(f32)
    rho = np.zeros((H, W, 3), f32)
    N = rng.normal(0, 1, (H, W, 3)).astype(f32)
    z = rng.choice(f32([0.0, 1e-3, 2000.0]), (H, W)).astype(f32)
    cov = np.ones((H, W), f32)
    for levels in (1, 6):
        out, rgb = G.denoise(A, B, None, rho, N, z, cov, **dict(G.DEFAULTS, levels=levels, flags=flags))
        assert np.isfinite(out).all() and (out >= 0).all()


# ---- 4. does it denoise -------------------------------------------------------------------------------------------------------------
def test_the_prototype_scene_gets_closer_to_the_truth_and_keeps_its_texture():
    c = GC.prototype()
    noisy = G.prepare(c.A, c.B, None, c.rho, c.cov, G.NO_DEMODULATION)[2]
    out, _ = G.denoise(c.A, c.B, None, c.rho, c.N, c.z, c.cov)
    r_noisy, r_out = GC.rmse(noisy, c.truth), GC.rmse(out, c.truth)
    print(f"RMSE noisy {r_noisy:.4f}, filtered {r_out:.4f}")
    assert np.isfinite(out).all() and r_out < r_noisy, (r_out, r_noisy)
    # the checker's contrast across a cell edge inside the lit left half (columns 7 | 8, rows 0..31, signed by which side is
    # the bright cell): the truth's, within a tenth
    rows = slice(0, 32)
    sign = (c.checker[rows, 8] - c.checker[rows, 7]).astype(np.float64)[:, None]
    step_truth = float(np.mean(sign * (c.truth[rows, 8].astype(np.float64) - c.truth[rows, 7])))
    step_out = float(np.mean(sign * (out[rows, 8].astype(np.float64) - out[rows, 7])))
    assert abs(step_truth) > 0.3 and abs(step_out - step_truth) < 0.1 * abs(step_truth), (step_out, step_truth)
    # ... which a filter that does not know the albedo loses: the same filter, albedo buffer constant, keeps less than that
    flat, _ = G.denoise(c.A, c.B, None, np.full_like(c.rho, 0.5), c.N, c.z, c.cov)
    assert GC.rmse(out, c.truth) < GC.rmse(flat, c.truth)


def test_oracle_renders_of_the_spheres_scene_get_closer_to_a_converged_one(oracle):
    """A and B are two oracle renders at 4 spp with different seeds, the features np_features' at 4 samples, the reference an
    oracle render at 256 spp with a third seed."""
    w, h, n = 80, 48, 4
    cam = scenes.camera(oracle, w, h)
    sc = scenes.spheres_scene()
    A = oracle.render(cam, sc, abi.default_opts(spp=n, seed=21))[0]
    B = oracle.render(cam, sc, abi.default_opts(spp=n, seed=22))[0]
    ref = oracle.render(cam, sc, abi.default_opts(spp=256, seed=23))[0]
    ft = np_features.features(oracle, cam, sc, abi.default_opts(spp=n, seed=21), 4)
    noisy = (A * f32(0.5)) + (B * f32(0.5))
    out, _ = G.denoise(A, B, None, ft.albedo, ft.normal, ft.depth, ft.coverage)
    r_noisy, r_out = GC.rmse(noisy, ref), GC.rmse(out, ref)
    print(f"RMSE noisy {r_noisy:.5f}, filtered {r_out:.5f}, ratio {r_out / r_noisy:.3f}")
    assert np.isfinite(out).all() and r_out < r_noisy, (r_out, r_noisy)
