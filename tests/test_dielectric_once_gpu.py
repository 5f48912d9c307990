"""The dielectric's unit vectors computed once (scatter_dielectric, kernels.hip) against the oracle's scatter entry.

The reference normalises the incoming direction and the normal (or its negation) three times each (reflect, the cosine,
refract); the device computes du and nu once when every lane of the wave passes normalize's gate and runs the reference's
sequence otherwise. rbrt_hip_debug_scatter runs event i in lane i % 64, so 64 consecutive events are one wave: 500 waves
of seeded events, replayed the way test_scatter_events.py replays its fixture -- direction, returned flag and stream state
afterwards, bit for bit. (A lane whose normal is zero or subnormal produces NaN: which NaN an operation returns is the
processor's choice, x86 and gfx950 differ in its sign, so for such a lane the same components must be NaN; its 63
neighbours, which run the reference's sequence because of it, are compared bit for bit like every other lane.)
"""
import ctypes as C

import numpy as np
import pytest

from rbrt_amd import abi

pytestmark = pytest.mark.gpu

F = np.float32
N_WAVES = 500
INDICES = (1.0, 1.5, 2.4)
LENGTHS = (1e-3, 0.5, 1.0, 1000.0)


def unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make_events():
    rng = np.random.default_rng(777)
    n = 64 * N_WAVES
    param = np.array(INDICES, F)[rng.integers(0, 3, n)]
    nlen = np.array(LENGTHS, np.float64)[rng.integers(0, 4, n)]
    nrm = unit(rng.normal(size=(n, 3)))
    d = unit(rng.normal(size=(n, 3))).astype(F)
    d = (d * (F(1) + rng.integers(-3, 4, (n, 3)).astype(F) * F(2.0 ** -23))).astype(F)  # off unit length by a few ulp, as refract's output is
    wave = np.arange(n) // 64
    lane = np.arange(n) % 64
    kind = wave % 5
    # 1: a == 0 exactly in a quarter of the lanes: axis-aligned direction and normal (normalize is exact on them)
    m = (kind == 1) & (lane % 4 == 0)
    ax = rng.integers(0, 3, n)
    e = np.eye(3)
    d[m] = (e[ax[m]] * rng.choice([-1.0, 1.0, 0.5, -2.0], (m.sum(), 1))).astype(F)
    nrm[m] = e[(ax[m] + 1 + rng.integers(0, 2, m.sum())) % 3] * rng.choice([-1.0, 1.0], (m.sum(), 1))
    # 2: leaving (a > 0) with the cosine swept ulp by ulp across the critical one, discr == 0: c^2 = 1 - 1 / index^2
    m = kind == 2
    c = np.sqrt(np.maximum(0.0, 1.0 - 1.0 / param[m].astype(np.float64) ** 2)) * (1.0 + (lane[m] - 32.0) * 2.0 ** -23) + (lane[m] - 32.0) * 2.0 ** -26
    nrm[m] = [0.0, 1.0, 0.0]
    d[m] = np.stack([np.sqrt(np.maximum(0.0, 1.0 - c * c)), c, np.zeros_like(c)], 1).astype(F)
    # 3: leaving at grazing angles: total internal reflection for the indices above 1
    m = kind == 3
    c = rng.uniform(0.01, 0.5, m.sum())
    t = unit(np.cross(nrm[m], rng.normal(size=(m.sum(), 3))))
    d[m] = (nrm[m] * c[:, None] + t * np.sqrt(1 - c * c)[:, None]).astype(F)
    normal = (nrm * nlen[:, None]).astype(F)  # un-normalised, as a sphere's normal p - centre is
    # 4: one lane of the wave has a zero or a subnormal normal: the whole wave runs the reference's sequence
    m = (kind == 4) & (lane == (wave * 7) % 64)
    normal[m] = np.where((wave[m] % 2 == 0)[:, None], F(0), np.array([1e-40, -2e-40, 1e-41], F)[None])
    point = rng.uniform(-5, 5, (n, 3)).astype(F)
    key = np.stack([np.full(n, 99), np.arange(n) % 4093, np.arange(n) // 4093], 1).astype(np.uint32)
    return dict(param=param, in_dir=d, normal=normal, point=point, key=key, odd=m)


@pytest.fixture(scope="module")
def ev(oracle):
    e = make_events()
    n = len(e["param"])
    out_dir, ok = np.zeros((n, 3), F), np.zeros(n, np.uint8)
    before, after = np.zeros((n, 2), np.uint32), np.zeros((n, 2), np.uint32)
    u32p = C.POINTER(C.c_uint32)
    fn = oracle.lib().rbrt_oracle_kat_scatter_state
    att, out, b, a = np.zeros(3, F), np.zeros(6, F), np.zeros(2, np.uint32), np.zeros(2, np.uint32)
    for i in range(n):
        mat = abi.material(abi.MAT_DIELECTRIC, (0.0, 0.0, 0.0), float(e["param"][i]))
        in_ray = np.concatenate([e["point"][i], e["in_dir"][i]]).astype(F)
        seed, pixel, sample = (int(x) for x in e["key"][i])
        ok[i] = fn(C.byref(mat), oracle._p(in_ray), oracle._p(e["point"][i].copy()), oracle._p(e["normal"][i].copy()), seed, pixel, sample,
                   oracle._p(att), oracle._p(out), b.ctypes.data_as(u32p), a.ctypes.data_as(u32p))
        out_dir[i], before[i], after[i] = out[3:], b, a
    e.update(exp_dir=out_dir, exp_ok=ok, before=before, after=after)
    return e


def test_events_cover_the_cases(ev):
    d, nr, idx = ev["in_dir"].astype(np.float64), ev["normal"].astype(np.float64), ev["param"].astype(np.float64)
    good = ~ev["odd"]
    with np.errstate(all="ignore"):
        a = (unit(d) * unit(nr)).sum(axis=1)
        ratio = np.where(a > 0, idx, 1.0 / idx)
        discr = 1.0 - ratio * ratio * (1.0 - a * a)
    assert (a[good] > 0).sum() > 5000 and (a[good] < 0).sum() > 5000 and (a[good] == 0).sum() > 100
    assert ((discr < 0) & good).sum() > 3000 and ((np.abs(discr) < 1e-6) & (discr > 0) & good).sum() > 100 and ((np.abs(discr) < 1e-6) & (discr < 0) & good).sum() > 100
    assert ev["odd"].sum() == N_WAVES // 5 and set(np.unique(ev["param"]).tolist()) == {1.0, 1.5, F(2.4).item()}
    assert np.isnan(ev["exp_dir"][ev["odd"]]).any(axis=1).all() and not np.isnan(ev["exp_dir"][good]).any()
    assert (ev["exp_ok"] == 1).all()  # dielectric.rs:58


def test_device_dielectric_matches_the_oracle_bit_for_bit(hip, ev):
    n = len(ev["param"])
    got_dir, got_ok, got_st = hip.debug_scatter(np.full(n, abi.MAT_DIELECTRIC, np.int32), np.zeros((n, 3), F), ev["param"], ev["in_dir"],
                                                ev["point"], ev["normal"], ev["before"])
    assert np.array_equal(got_ok, ev["exp_ok"])
    assert np.array_equal(got_st, ev["after"]), "draw count / order differs"
    gb, eb = got_dir.view(np.uint32), ev["exp_dir"].view(np.uint32)
    nan_lane = ev["odd"][:, None] & np.isnan(ev["exp_dir"])
    bad = ((gb != eb) & ~nan_lane).any(axis=1) | (nan_lane & ~np.isnan(got_dir)).any(axis=1)
    idx = np.nonzero(bad)[0]
    assert len(idx) == 0, [(int(i), ev["in_dir"][i].tolist(), ev["normal"][i].tolist(), float(ev["param"][i]), got_dir[i].tolist(),
                            ev["exp_dir"][i].tolist()) for i in idx[:6]]
