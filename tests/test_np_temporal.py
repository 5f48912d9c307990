"""The numpy restatement of the temporal accumulation (np_temporal.py) pinned from outside, without a GPU: a scalar evaluation
of the rule of include/rbrt_hip.h with per-pixel Python loops, which shares no code with the restatement, agrees bit for bit;
the rule's exact consequences hold; a static camera gives the running mean; eight frames lower the error as a mean of at least
four would; and the frozen inputs (temporal_cases.py) exercise what they are meant to."""
import math

import numpy as np
import pytest

import np_temporal as NT
import temporal_cases as TC

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def run(c, **kw):
    return NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, c.hist, **dict(NT.DEFAULTS, **kw))


# ---- the rule again, one pixel at a time -----------------------------------------------------------------------------------------
def s_dot(a, b):
    return f32(f32(f32(a[0] * b[0]) + f32(a[1] * b[1])) + f32(a[2] * b[2]))


def s_vec(x):
    return [f32(x[0]), f32(x[1]), f32(x[2])]


def scalar_accumulate(c, M, kz, kn):
    """-> (A', B', len) by the header's rule, every operation on numpy float32 scalars."""
    M, kz, kn = f32(M), f32(kz), f32(kn)
    K, Kp = c.cam, c.cam_prev
    W, H = int(K.img_width_pix), int(K.img_height_pix)
    r, u = s_vec(Kp.right), s_vec(Kp.up)
    n = [f32(f32(r[1] * u[2]) - f32(r[2] * u[1])), f32(f32(r[2] * u[0]) - f32(r[0] * u[2])), f32(f32(r[0] * u[1]) - f32(r[1] * u[0]))]
    w = [f32(f32(Kp.img_center_point[k]) - f32(Kp.position[k])) for k in range(3)]
    wn, rr, uu, ru = s_dot(w, n), s_dot(r, r), s_dot(u, u), s_dot(r, u)
    det = f32(f32(rr * uu) - f32(ru * ru))
    sx, sy = f32(f32(0.001) * f32(Kp.mm_per_pix_hor)), f32(f32(0.001) * f32(Kp.mm_per_pix_vert))
    hx, hy = f32(W // 2), f32(H // 2)
    pos, posp, right, up, centre = s_vec(K.position), s_vec(Kp.position), s_vec(K.right), s_vec(K.up), s_vec(K.img_center_point)
    oa, ob, ol = np.array(c.A, f32), np.array(c.B, f32), np.ones((H, W), f32)
    h = c.hist
    with np.errstate(all="ignore"):
        for row in range(H):
            for col in range(W):
                cm = f32(f32(f32(col) - hx) * f32(K.mm_per_pix_hor))
                rm = f32(f32(f32(row) - hy) * f32(K.mm_per_pix_vert))
                kc, kr = f32(f32(0.001) * cm), f32(f32(0.001) * rm)
                T = [f32(f32(centre[k] + f32(kc * right[k])) - f32(kr * up[k])) for k in range(3)]
                e = [f32(T[k] - pos[k]) for k in range(3)]
                ln = f32(np.sqrt(s_dot(e, e)))
                d = [f32(e[k] / ln) for k in range(3)]
                cp = f32(c.c[row, col])
                surface = cp > 0
                if surface:
                    zbar = f32(f32(c.z[row, col]) / cp)
                    v = [f32(f32(pos[k] + f32(zbar * d[k])) - posp[k]) for k in range(3)]
                else:
                    v = d
                t = f32(wn / s_dot(v, n))
                if not (t > 0 and t < f32(np.inf)):
                    continue
                Q = [f32(f32(t * v[k]) - w[k]) for k in range(3)]
                qr, qu = s_dot(Q, r), s_dot(Q, u)
                a = f32(f32(f32(qr * uu) - f32(qu * ru)) / det)
                b = f32(f32(f32(qr * ru) - f32(qu * rr)) / det)
                xs, ys = f32(f32(a / sx) + hx), f32(f32(b / sy) + hy)
                if not (xs > f32(-1) and xs < f32(W) and ys > f32(-1) and ys < f32(H)):
                    continue
                i, j = math.floor(float(xs)), math.floor(float(ys))
                fx, fy = f32(xs - f32(i)), f32(ys - f32(j))
                gx, gy = f32(f32(1) - fx), f32(f32(1) - fy)
                ze = f32(np.sqrt(s_dot(v, v)))
                ws, sl, sa, sb = f32(0), f32(0), [f32(0)] * 3, [f32(0)] * 3
                for qy, qx, bw in ((j, i, f32(gx * gy)), (j, i + 1, f32(fx * gy)), (j + 1, i, f32(gx * fy)), (j + 1, i + 1, f32(fx * fy))):
                    if not (0 <= qy < H and 0 <= qx < W):
                        continue
                    cq = f32(h.c[qy, qx])
                    if surface:
                        if not cq > 0:
                            continue
                        zq = f32(f32(h.z[qy, qx]) / cq)
                        if not abs(f32(zq - ze)) <= f32(kz * ze):
                            continue
                        D = [f32(f32(c.N[row, col, k]) - f32(h.n[qy, qx, k])) for k in range(3)]
                        if not s_dot(D, D) <= f32(kn * kn):
                            continue
                    elif not cq == 0:
                        continue
                    ws = f32(ws + bw)
                    sa = [f32(sa[k] + f32(bw * f32(h.a[qy, qx, k]))) for k in range(3)]
                    sb = [f32(sb[k] + f32(bw * f32(h.b[qy, qx, k]))) for k in range(3)]
                    sl = f32(sl + f32(bw * f32(h.length[qy, qx])))
                if not ws >= f32(0.01):
                    continue
                hl = f32(sl / ws)
                length = min(f32(hl + f32(1)), M)
                alpha = f32(f32(1) / length)
                for k in range(3):
                    HA, HB = f32(sa[k] / ws), f32(sb[k] / ws)
                    oa[row, col, k] = f32(HA + f32(alpha * f32(f32(c.A[row, col, k]) - HA)))
                    ob[row, col, k] = f32(HB + f32(alpha * f32(f32(c.B[row, col, k]) - HB)))
                ol[row, col] = length
    return oa, ob, ol


@pytest.mark.parametrize("pair", list(TC.PAIRS))
def test_a_scalar_evaluation_agrees_bit_for_bit(pair):
    c = TC.case(pair, 37, 21)
    for p in (NT.DEFAULTS, dict(max_history=4.0, depth=0.0, normal=0.0), dict(max_history=1000.0, depth=0.5, normal=2.0)):
        oa, ob, ln, nxt, _ = run(c, **p)
        ea, eb, el = scalar_accumulate(c, p["max_history"], p["depth"], p["normal"])
        assert np.array_equal(bits(oa), bits(ea)) and np.array_equal(bits(ob), bits(eb)) and np.array_equal(bits(ln), bits(el)), (pair, p)
        # the next history is the outputs and this frame's features
        assert all(np.array_equal(bits(x), bits(y)) for x, y in ((nxt.a, oa), (nxt.b, ob), (nxt.length, ln), (nxt.n, c.N), (nxt.z, c.z), (nxt.c, c.c)))


# ---- exact properties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", list(TC.PAIRS))
def test_exact_properties(pair):
    c = TC.case(pair, 50, 47)
    oa, ob, ln, _, info = run(c)
    inv = ~info.valid
    # a pixel without a valid history equals its input bits and has len 1
    assert np.array_equal(bits(oa)[inv], bits(c.A)[inv]) and np.array_equal(bits(ob)[inv], bits(c.B)[inv]) and (ln[inv] == 1).all()
    assert (info.accepted.sum(0)[~info.projects] == 0).all()
    # len never exceeds M, whatever the history's lengths (they reach 40)
    assert c.hist.length.max() == 40
    for M in (1.0, 7.5, 32.0, 1000.0):
        l2 = run(c, max_history=M)[2]
        assert (l2 >= 1).all() and l2.max() <= f32(M)
    if info.valid.any():
        assert ln.max() == 32 and run(c, max_history=1.0)[2].max() == 1
    # changing the history at the taps that no pixel accepts changes no output bit
    used = np.zeros((c.h, c.w), bool)
    for k, (dj, di) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        acc = info.accepted[k]
        used[(info.j + dj)[acc], (info.i + di)[acc]] = True
    assert not used.all()
    h2 = NT.History(c.hist.a.copy(), c.hist.b.copy(), c.hist.length.copy(), c.hist.n, c.hist.z, c.hist.c)
    h2.a[~used], h2.b[~used], h2.length[~used] = f32(np.nan), f32(-3e38), f32(np.inf)
    pa, pb, pl, _, _ = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam, c.cam_prev, h2, **NT.DEFAULTS)
    assert np.array_equal(bits(pa), bits(oa)) and np.array_equal(bits(pb), bits(ob)) and np.array_equal(bits(pl), bits(ln))


def test_the_first_frame_is_the_identity():
    c = TC.case("turn", 37, 21)
    oa, ob, ln, nxt, info = NT.accumulate(c.A, c.B, c.N, c.z, c.c, c.cam)
    assert info is None and np.array_equal(bits(oa), bits(c.A)) and np.array_equal(bits(ob), bits(c.B)) and (ln == 1).all()
    assert np.array_equal(bits(nxt.a), bits(c.A)) and np.array_equal(bits(nxt.n), bits(c.N)) and (nxt.length == 1).all()
    packed = NT.pack(nxt)
    assert packed.shape == (3, 21, 37, 4) and packed.nbytes == 48 * 37 * 21
    assert np.array_equal(packed[0, ..., 3], ln) and np.array_equal(packed[1, ..., 3], c.c) and np.array_equal(packed[2, ..., 3], c.z)


# ---- does it accumulate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(48, 64), (37, 21)])
def test_a_static_camera_gives_the_running_mean_and_lowers_the_error(w, h):
    n = 8
    F = TC.frames(w, h, n)
    hist, off, D, big = None, 0.0, 0.0, 0.0
    for k in range(n):
        oa, ob, ln, hist, info = NT.accumulate(F.A[k], F.B[k], F.N, F.z, F.c, F.cam, F.cam, hist, **NT.DEFAULTS)
        if info is not None:
            assert info.valid.all() and (np.abs(ln - f32(k + 1)) <= 1e-5 * (k + 1)).all()
            off = max(off, float(np.abs(info.xs - np.arange(w, dtype=f32)).max()), float(np.abs(info.ys - np.arange(h, dtype=f32)[:, None]).max()))
        for img in (oa, ob):  # the largest difference between a pixel and one of its eight neighbours, and the largest value
            i64 = img.astype(np.float64)
            D = max(D, np.abs(i64[1:] - i64[:-1]).max(), np.abs(i64[:, 1:] - i64[:, :-1]).max(),
                    np.abs(i64[1:, 1:] - i64[:-1, :-1]).max(), np.abs(i64[1:, :-1] - i64[:-1, 1:]).max())
            big = max(big, np.abs(i64).max())
    assert off < 1e-3, off  # a static camera reprojects every pixel onto itself, up to the rounding of the point and back
    # The tolerance. A frame reads its history through a bilinear footprint that is off its own pixel by at most `off` in each
    # axis, so what it reads differs from its own pixel's value by at most (2 off + off^2) D, D being the largest difference
    # between neighbours; a frame's mix passes on less than the error it received plus that, so n frames stay within n times
    # it. The float32 operations add a few units in the last place of the largest value a frame: 16 * 2^-24 a frame is generous.
    tol = n * ((2 * off + off * off) * D + 16 * 2.0 ** -24 * big)
    assert tol < 0.01  # (far below the frames' noise, whose sigma is 0.3 of values up to 1: the comparison means something)
    for got, frames_ in ((oa, F.A), (ob, F.B)):
        assert np.abs(got - frames_.astype(np.float64).mean(0)).max() <= tol, (np.abs(got - frames_.astype(np.float64).mean(0)).max(), tol)
    # eight frames of independent noise: at most the error of a four-frame mean (the ideal is 1/sqrt(8) = 0.354)
    single = TC.rmse((F.A[n - 1].astype(np.float64) + F.B[n - 1]) / 2, F.truth)
    accumulated = TC.rmse((oa.astype(np.float64) + ob) / 2, F.truth)
    print(f"{w}x{h}: RMSE of one frame {single:.5f}, of eight accumulated {accumulated:.5f} (ratio {accumulated / single:.3f})")
    assert accumulated <= 0.5 * single, (accumulated, single)


# ---- conditions on the inputs ------------------------------------------------------------------------------------------------------
def test_the_inputs_exercise_the_rule():
    for w, h in ((37, 21), (50, 47)):
        counts, outside, bg_acc, bg_rej = set(), False, False, False
        for pair in TC.MOVED:
            c = TC.case(pair, w, h)
            info = run(c)[4]
            share = info.valid.mean()
            assert 0.05 <= share <= 0.99, (pair, w, h, share)
            counts |= set(np.unique(info.accepted.sum(0)).tolist())
            outside |= bool((~info.projects).any())
            bg_acc |= bool((~info.surface & info.valid).any())
            bg_rej |= bool((~info.surface & ~info.valid).any())
        assert counts == {0, 1, 2, 3, 4} and outside and bg_acc and bg_rej, (w, h, counts, outside, bg_acc, bg_rej)
        st = run(TC.case("static", w, h))[4]
        assert st.projects.all() and np.abs(st.xs - np.arange(w, dtype=f32)).max() < 1e-3
        assert np.abs(st.ys - np.arange(h, dtype=f32)[:, None]).max() < 1e-3
        assert 0.001 < np.abs(run(TC.case("drift_0.002", w, h))[4].xs - np.arange(w, dtype=f32)).max() < 0.5   # within a pixel
        assert np.abs(run(TC.case("turn", w, h))[4].xs - np.arange(w, dtype=f32))[run(TC.case("turn", w, h))[4].projects].max() > 2  # several
        assert not run(TC.case("away", w, h))[4].projects.any()                       # t <= 0 everywhere
        aside = run(TC.case("aside", w, h))[4]
        assert not aside.projects[aside.surface].any() and aside.projects[~aside.surface].all()  # the sky is reprojected by direction
        c = TC.case("turn", w, h)
        assert (c.c == 0.5).any() and (c.c == 0).any() and (c.c == 1).any() and max(c.A.max(), c.B.max()) == f32(1e6)
        up, right = np.array(list(c.cam_prev.up)), np.array(list(c.cam_prev.right))
        assert abs(up @ right) > 0.05 and abs(up @ up - 1) > 0.05  # the Gram solve has something to solve
