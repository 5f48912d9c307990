"""The proof behind normalize's short path (kernels.hip "IEEE square root and division, the short way"), checked in exact
rational arithmetic (tests/ieee_model.py) on the operands where division goes wrong: quotients on and next to the
rounding midpoints, at the smallest quotients the gate admits, with v_rcp_f32 anywhere within one ulp. No GPU needed."""
from fractions import Fraction as F

import numpy as np

import ieee_model as M

RCP = (-1, 0, 1)


def _check(vectors):
    """(inside the gate, mismatches of the short sequence inside the gate, mismatches outside it) over rcp at -1, 0, +1 ulp."""
    n_in, bad_in, bad_out = 0, [], []
    for v in vectors:
        a = [F(float(c)) for c in v]
        ok = M.gate(a)
        n_in += ok
        ex = M.exact_normalize(a)
        for k in RCP:
            if M.short_normalize(a, k) != ex:
                (bad_in if ok else bad_out).append((tuple(v), k))
    return n_in, bad_in, bad_out


def test_the_issue_case_is_off_by_one_ulp_and_outside_the_gate():
    """a = (27 2^-104, 3 2^46, 27 2^-104): x / |a| = 9 2^-150 = 4.5 ulps of the smallest subnormal, which rounds to 4; the
    short sequence gives 5 whichever way v_rcp_f32 errs. It passed the gate's old bound |a|^2 < 2^100, not the current one."""
    a = [F(27) * F(2) ** -104, F(3) * F(2) ** 46, F(27) * F(2) ** -104]
    assert M.exact_normalize(a)[0] == 4 * F(2) ** -149
    assert all(M.short_normalize(a, k)[0] == 5 * F(2) ** -149 for k in RCP)
    assert not M.gate(a)
    old, M.S_HI = M.S_HI, M.S_HI_SQRT
    try:
        assert M.gate(a)
    finally:
        M.S_HI = old


def test_subnormal_midpoints_never_pass_the_gate():
    """Quotients on and one ulp either side of every subnormal midpoint family, lengths 2^0 .. 2^50: the short sequence
    gets some of them wrong (so the family is sharp), and the gate lets none of those -- nor any subnormal quotient -- in."""
    fam = list(M.midpoint_family(range(0, 51)))
    n_in, bad_in, bad_out = _check(fam)
    assert n_in == 0 and not bad_in
    assert len(bad_out) > 100
    assert {k for _, k in bad_out} == set(RCP)  # every rcp variant fails somewhere: no reciprocal fixes it


def test_gate_admits_only_normal_quotients():
    """The smallest component just above 2^-100 and the length just below 2^26: the smallest quotient the gate admits is
    above 2^-126. Lengths at 2^26 and above let subnormal quotients in, so the bound is where it has to be."""
    small = float(np.nextafter(np.float32(2.0 ** -100), np.float32(1)))
    for top in (np.nextafter(np.float32(2.0 ** 26), np.float32(0)), np.float32(2.0 ** 25 * 1.5), np.float32(2.0 ** 20)):
        a = [F(small), F(float(top)), F(small)]
        assert M.gate(a)
        assert M.exact_normalize(a)[0] >= F(2) ** -126
    a = [F(small), F(2) ** 26, F(small)]
    assert not M.gate(a)  # |a|^2 = 2^52


def test_near_midpoint_normal_quotients_inside_the_gate():
    """Inside the gate: quotients next to the midpoints of normal f32 from 2^-126 up to 1, exponent gaps between component
    and length from 0 to beyond 96, lengths from 2^-40 to just below 2^26, the smallest component just above 2^-100 and
    the gate's own constants one ulp either side. The short sequence equals the correctly rounded division for v_rcp_f32
    at -1, 0 and +1 ulp."""
    rng = np.random.default_rng(5)
    vecs = []
    small = float(np.nextafter(np.float32(2.0 ** -100), np.float32(1)))
    for _ in range(600):
        le = int(rng.integers(-40, 26))
        L = float(np.float32((1 + rng.random()) * 2.0 ** le))
        qe = int(rng.integers(max(-126, -99 - le), 1))
        mid = (2 * int(rng.integers(2 ** 23, 2 ** 24)) + 1) * 2.0 ** (qe - 24)  # a midpoint between two f32 of exponent qe
        x = np.float32(F(L) * F(mid))
        if not 2.0 ** -100 < float(x) < L:
            continue
        for k in (-1, 0, 1):
            vecs.append((float(np.uint32(int(x.view(np.uint32)) + k).view(np.float32)), L, max(small, float(np.float32(L * 2.0 ** -110)))))
    for L in (2.0 ** -40 * 1.0000002, 2.0 ** -4, 2.0 ** 10, 2.0 ** 25 * 1.9):
        vecs.append((small, float(np.float32(L)), small))
    for target in (2.0 ** -80, 2.0 ** 52):  # |a|^2 at the gate's constants and their neighbours
        y0 = np.float32(np.sqrt(target))
        for dy in range(-3, 4):
            y = np.float32(np.uint32(int(y0.view(np.uint32)) + dy).view(np.float32))
            vecs.append((small, float(y), small))
    n_in, bad_in, _ = _check(vecs)
    assert n_in > 1000
    assert not bad_in, bad_in[:5]
    gaps = [np.log2(abs(v[1])) - np.log2(abs(v[0])) for v in vecs if M.gate([F(c) for c in v])]
    assert max(gaps) > 120 and min(gaps) < 2
