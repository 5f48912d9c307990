"""The kernels' short IEEE forms (kernels.hip "IEEE square root and division, the short way") over the whole domain their
gates admit, against a correctly rounded reference: host float64 rounded to float32, which is correctly rounded for sqrt
and for / (53 >= 2 * 24 + 2; for a subnormal quotient a midpoint is either exact in float64 or at least 2^-48 away
relative, so the second rounding cannot go wrong either). Operands are packed so that whole 64-lane waves are inside the
gates, and the hook's per-element flags show that those waves really took the short path."""
import ctypes as C

import numpy as np
import pytest

import ieee_model as M
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

f32 = np.float32


def bits(x):
    return int(np.float32(x).view(np.uint32))


def from_bits(b):
    return np.asarray(b, np.uint32).view(np.float32)


def debug_ieee(x, v):
    x = np.ascontiguousarray(x, f32)
    v = np.ascontiguousarray(v, f32).reshape(-1, 3)
    n, m = len(x), len(v)
    out_s, out_sf = np.zeros(max(n, 1), f32), np.zeros(max(n, 1), np.uint8)
    out_q, out_qf = np.zeros((max(m, 1), 3), f32), np.zeros(max(m, 1), np.uint8)
    abi.check(abi.load_hip().rbrt_hip_debug_ieee(abi.fptr(x), n, abi.fptr(v), m, abi.fptr(out_s), out_sf.ctypes.data_as(abi.u8p),
                                                 abi.fptr(out_q), out_qf.ctypes.data_as(abi.u8p)))
    return out_s[:n], out_sf[:n].astype(bool), out_q[:m], out_qf[:m].astype(bool)


def ref_sqrt(x):
    return np.sqrt(x.astype(np.float64)).astype(f32)


def ref_normalize(v):
    v = v.astype(f32)
    s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]  # f32, unfused, the kernel's order
    with np.errstate(all="ignore"):
        ln = np.sqrt(s.astype(np.float64)).astype(f32)
        return (v.astype(np.float64) / ln.astype(np.float64)[:, None]).astype(f32)


def in_gate(v):
    v = v.astype(f32)
    with np.errstate(over="ignore", under="ignore"):
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return (s > f32(M.S_LO)) & (s < f32(M.S_HI)) & (np.abs(v).min(1) > f32(M.MIN))


def packed(v):
    """v reordered as whole waves inside normalize's gate, then the rest; returns (vectors, inside)."""
    ok = in_gate(v)
    a, b = v[ok], v[~ok]
    pad = (-len(a)) % 64
    if pad and len(a):
        a = np.concatenate([a, a[:pad]])
    return np.concatenate([a, b]), np.concatenate([np.ones(len(a), bool), np.zeros(len(b), bool)])


def same(p, q):
    return (p.view(np.uint32) == q.view(np.uint32)) | (np.isnan(p) & np.isnan(q))


def check_normalize(v):
    v, inside = packed(np.asarray(v, f32).reshape(-1, 3))
    _, _, q, short = debug_ieee(np.zeros(0, f32), v)
    exp = ref_normalize(v)
    bad = ~same(q, exp).all(1)
    assert not bad.any(), (int(bad.sum()), v[bad][:4].tolist(), q[bad][:4].tolist(), exp[bad][:4].tolist())
    assert short[inside].all()  # whole waves inside the gate ran the short path
    n_out = (~inside).sum()
    if n_out >= 64:
        assert not short[~inside][: n_out // 64 * 64].any()
    return v, inside


def test_sqrt_exhaustive_over_the_short_domain(hip):
    """Every float in (2^-80, 2^100), about 1.5e9, through ieee_sqrt on the device: each result passes the exact integer
    test of correct rounding, equals the compiler's sqrt, and came from the short path."""
    first, last = bits(2.0 ** -80) + 1, bits(2.0 ** 100) - 1
    n = last - first + 1
    counts = (C.c_uint64 * 3)()
    abi.check(abi.load_hip().rbrt_hip_selftest_sqrt_sweep(first, n, counts))
    assert list(counts) == [0, 0, n]
    # the test is not vacuous: the sweep over the whole positive normal range leaves the gate for the ends' waves
    abi.check(abi.load_hip().rbrt_hip_selftest_sqrt_sweep(bits(2.0 ** -126), bits(3e38) - bits(2.0 ** -126), counts))
    assert counts[0] == 0 and counts[1] == 0 and counts[2] < bits(3e38) - bits(2.0 ** -126)


def test_sqrt_at_the_gate_constants(hip):
    """x at 2^-80 and 2^100 and 64 floats either side, a wave of each: the waves inside take the short path, those with a
    lane outside do not, and every result is correctly rounded."""
    x = []
    for c in (2.0 ** -80, 2.0 ** 100):
        b = bits(c)
        x += [from_bits(np.arange(b - 64, b)), from_bits(np.arange(b + 1, b + 65)), from_bits(np.arange(b - 32, b + 32))]
    x = np.concatenate(x)
    r, short, _, _ = debug_ieee(x, np.zeros((0, 3), f32))
    assert same(r, ref_sqrt(x)).all()
    assert short.reshape(-1, 64).all(1).tolist() == [False, True, False, True, False, False]


def test_normalize_subnormal_midpoints(hip):
    """(x, L, x) with x / L on, and one ulp next to, a midpoint between two subnormals (x = L (2k+1) 2^-150), for L from
    2^0 to 2^50: the short division rounds those quotients on its own, which gets about half of the midpoints wrong (the
    exact model, test_ieee_model.py); the gate has to keep them off the short path."""
    fam = np.array(list(M.midpoint_family(range(0, 51))), f32)
    assert len(fam) > 600 and (np.abs(ref_normalize(fam)[:, 0]) < 2.0 ** -126).all()
    check_normalize(np.concatenate([fam, -fam, fam[:, [1, 0, 2]]]))


def test_normalize_whole_domain_families(hip):
    """len from 2^-40 to 2^50, smallest component just above 2^-100, quotients down to 2^-150, exponent gaps of 96 and
    more, and the gate's constants one ulp either side: all correctly rounded, and the in-gate waves short."""
    rng = np.random.default_rng(7)
    small = f32(np.nextafter(f32(2.0 ** -100), f32(1)))
    vecs = []
    for le in range(-40, 51):
        L = f32((1 + rng.random(64)) * 2.0 ** le)
        for gap in list(range(0, 130, 7)) + [95, 96, 97, 120, 126, 127, 140, 149]:
            x = (L * f32(2.0 ** -gap)).astype(f32) if le - gap > -101 else np.full(64, small)
            x = np.maximum(x, small)
            vecs.append(np.stack([x, L, np.maximum(small, (L * f32(2.0 ** -60)).astype(f32))], 1))
    for target in (2.0 ** -80, 2.0 ** 52, 2.0 ** 100):  # |a|^2 at the gate's constants (and sqrt_in_range's) and around them
        y0 = bits(np.sqrt(target))
        ys = from_bits(np.arange(y0 - 8, y0 + 8))
        for z in (small, f32(np.sqrt(target) * 2.0 ** -12), f32(np.sqrt(target) * 2.0 ** -13)):
            vecs.append(np.stack([np.full(16, small), ys, np.full(16, z)], 1))
    for c in (bits(2.0 ** -100) - 1, bits(2.0 ** -100), bits(2.0 ** -100) + 1):  # the smallest component around kNormMin
        vecs.append(np.stack([np.full(64, from_bits(c)), f32(2.0 ** rng.uniform(-39, 49, 64)), np.full(64, f32(0.5))], 1))
    v = np.concatenate(vecs).astype(f32)
    signs = np.where(rng.random(v.shape) < 0.5, f32(-1), f32(1))
    v, inside = check_normalize(np.concatenate([v, v * signs]))
    s = ((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])[inside]
    assert s.min() < 2.0 ** -78 and s.max() > 2.0 ** 51  # the gate's whole range was reached on the short path


def test_normalize_random_over_the_full_domain(hip):
    """Random vectors: the largest component 2^-40 .. 2^50, the others from just above 2^-100 up to it, random signs."""
    rng = np.random.default_rng(8)
    n = 1 << 20
    e_top = rng.integers(-40, 50, n)
    e = np.minimum(rng.integers(-100, 50, (n, 3)), e_top[:, None])
    e[np.arange(n), rng.integers(0, 3, n)] = e_top
    v = ((1 + rng.random((n, 3))) * np.exp2(e.astype(np.float64))).astype(f32)
    v = np.maximum(v, f32(np.nextafter(f32(2.0 ** -100), f32(1)))) * np.where(rng.random((n, 3)) < 0.5, f32(-1), f32(1))
    v, inside = check_normalize(v)
    assert inside.sum() > n // 4

