"""Exact model of the kernels' short normalize (kernels.hip "IEEE square root and division, the short way"), for the CPU
tests and for building the GPU tests' operands: every f32 operation is its exact rational value rounded once to f32
(round to nearest even, subnormals kept), v_rcp_f32 is the correctly rounded reciprocal moved by a chosen number of ulps.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

# normalize's gate (kernels.hip kNormSLo / kNormSHi / kNormMin): s = |a|^2 in (S_LO, S_HI), every |component| > MIN
S_LO, S_HI, MIN = 2.0 ** -80, 2.0 ** 52, 2.0 ** -100
# the bound it had before quotients below 2^-126 were kept off the short path (that of sqrt_in_range)
S_HI_SQRT = 2.0 ** 100


def f32(x: Fraction) -> Fraction:
    """x rounded to the nearest f32 (ties to even; subnormals kept; the domain here never overflows)."""
    if x == 0:
        return Fraction(0)
    sign, a = (-1, -x) if x < 0 else (1, x)
    e = a.numerator.bit_length() - a.denominator.bit_length()  # 2^e <= a < 2^(e+2)
    if Fraction(2) ** e > a:
        e -= 1
    q = Fraction(2) ** (max(e, -126) - 23)  # the spacing of f32 at a
    n, r = divmod(a / q, 1)
    n = int(n) + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and int(n) % 2 == 1) else 0)
    assert n * q < Fraction(2) ** 128
    return sign * n * q


def ulp_step(x: Fraction, k: int) -> Fraction:
    """The f32 k steps away from the positive normal f32 x."""
    b = int(np.float32(float(x)).view(np.uint32)) + k
    return Fraction(float(np.uint32(b).view(np.float32)))


def sqrt32(s: Fraction) -> Fraction:
    """The correctly rounded f32 square root of a positive f32 (what sqrt_core returns on its domain)."""
    e = (s.numerator.bit_length() - s.denominator.bit_length()) // 2 - 60
    scale = Fraction(2) ** (2 * e)  # s / 4^e has ~120 integer bits: isqrt of it is exact to far below a half ulp
    m = s / scale
    r = Fraction(math.isqrt(m.numerator // m.denominator)) * Fraction(2) ** e
    # r <= sqrt(s) < r + 2^e, 2^e far below the spacing of f32 near sqrt(s): no square root of an f32 is a midpoint
    return f32(r + Fraction(2) ** e / 2)


def fma(a: Fraction, b: Fraction, c: Fraction) -> Fraction:
    return f32(a * b + c)


def gate(a) -> bool:
    """normalize's gate on the f32 components a (Fractions), s computed as the kernel does ((x x + y y) + z z)."""
    s = f32(f32(f32(a[0] * a[0]) + f32(a[1] * a[1])) + f32(a[2] * a[2]))
    return Fraction(S_LO) < s < Fraction(S_HI) and min(abs(c) for c in a) > Fraction(MIN)


def length(a) -> Fraction:
    return sqrt32(f32(f32(f32(a[0] * a[0]) + f32(a[1] * a[1])) + f32(a[2] * a[2])))


def short_normalize(a, rcp_ulps: int):
    """The short path's arithmetic, operation by operation, with v_rcp_f32 rcp_ulps ulps off the correctly rounded 1/len."""
    ln = length(a)
    rc0 = ulp_step(f32(1 / ln), rcp_ulps)
    rc = fma(fma(-ln, rc0, Fraction(1)), rc0, rc0)
    out = []
    for c in a:
        v = f32(c * rc)
        v = fma(fma(-ln, v, c), rc, v)
        out.append(fma(fma(-ln, v, c), rc, v))
    return out


def exact_normalize(a):
    """The reference: three correctly rounded divisions by the correctly rounded length."""
    ln = length(a)
    return [f32(c / ln) for c in a]


def midpoint_family(top_exps, odd_steps=(1, 3, 9, 27, 81, 12345, 2 ** 23 - 1), near=(-1, 0, 1)):
    """Vectors (x, L, x) whose x / |a| is (near) a midpoint between two subnormals: L = m 2^e (m odd, up to 3 bits) and
    x = L (2k+1) 2^-150, so x / L = (k + 1/2) 2^-149 exactly; near = the x one ulp below and above as well. x has to be a
    normal f32 above 2^-100, which holds for L (2k+1) > 2^50. Yields f32 triples as floats."""
    for e in top_exps:
        for m in (1, 3, 5, 7):
            L = m * 2.0 ** e
            for odd in odd_steps:
                x = L * odd * 2.0 ** -150
                if x <= 2.0 ** -100 or np.float32(x) != x:
                    continue
                for k in near:
                    xs = float(np.uint32(int(np.float32(x).view(np.uint32)) + k).view(np.float32))
                    yield (xs, L, xs)
