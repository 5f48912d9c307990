"""sphere_hit's two roots from one square root (kernels.hip), and the TERM pass's attenuation fold (megakernel.inl).

sphere_hit takes the square root of the discriminant and 2a once and forms both roots from them; which forms of sqrt
and division a wave runs depends on a vote of its lanes (ieee_sqrt, and the second root's block runs only where some
lane's first root is negative). HipScene.trace_rays runs ray i in lane i % 64, so a group of 64 consecutive rays is one
wave: every special ray below is traced once in a group of ordinary rays that also holds a ray with a vanishing
direction (den == 0, the compiler's forms) and once among ordinary rays only. What the device answers is compared with
the oracle bit for bit.

The special rays are built around the operand ranges in which the sign of n1 = -b - sqrt(sol) decides the sign of the first
root n1 / den: den = 2a and a negative n1 both within [2^-60, 2^60] (`ok` in model() below). A sphere_hit that picked the
root before a single division would have to vote on exactly that (measured and dropped for its register cost, DESIGN.md
§6); the rays sit on those bounds and either side of them so that such a form, or any other shortcut on these operands,
meets its edges here. The float32 restatement in this file only checks that the rays are where they are meant to be.

The render at the end pins the fold's word boundaries: a path's recorded bounces are packed four to a word, and
max_depth 3, 4, 5 and 9 between two mirrors give paths of up to that many records (none, one and two full words).
"""
import numpy as np
import pytest

import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

F = np.float32
LO, HI = F(2.0 ** -60), F(2.0 ** 60)  # the ranges of den and of a negative n1, see above
TINY_C, TINY_R = (0.0, 0.0, 0.0), 1e-3
HUGE_C, HUGE_R = (0.0, 0.0, -131072.0), 1e5
SPHERES = list(scenes.EXAMPLE_SPHERES) + [
    (TINY_C, TINY_R, abi.material(abi.MAT_LAMBERTIAN, (0.5, 0.5, 0.5))),
    (HUGE_C, HUGE_R, abi.material(abi.MAT_LAMBERTIAN, (0.3, 0.3, 0.3))),
]


def model(rays):
    """sphere_hit's operands in float32, in the kernel's order: (n_rays, n_spheres) arrays sol, n1, den and `ok`."""
    rays = np.asarray(rays, F)
    o, d = rays[:, None, :3], rays[:, None, 3:]
    c = np.array([s[0] for s in SPHERES], F)[None]
    r = np.array([s[1] for s in SPHERES], F)[None]
    with np.errstate(all="ignore"):
        dot = lambda u, v: (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
        a = dot(d, d) + np.zeros_like(r)
        l = o - c
        b = dot(d * F(2), l)
        cc = dot(l, l) - r * r
        sol = b * b - F(4) * a * cc
        s = np.sqrt(np.where(sol >= 0, sol, F(0))).astype(F)
        n1 = -b - s
        den = F(2) * a
        ok = (den >= LO) & (den <= HI) & ((n1 >= 0) | ((n1 <= -LO) & (n1 >= -HI)))
    return sol, n1, den, ok


def ordinary_rays(rng, n):
    """Rays from around the scene towards the four example spheres, directions of length 0.2 to 3."""
    c = np.array([s[0] for s in SPHERES[:4]], np.float64)
    r = np.array([s[1] for s in SPHERES[:4]], np.float64)
    k = rng.integers(0, 4, n)
    tgt = c[k] + rng.uniform(-1, 1, (n, 3)) * r[k, None] * 1.2
    o = np.array([0.0, 6.0, 2.0]) + rng.normal(size=(n, 3)) * np.array([8.0, 3.0, 8.0])
    d = tgt - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 3.0, (n, 1))
    rays = np.concatenate([o, d], 1).astype(F)
    sol, _, _, ok = model(rays)
    return rays[(ok | ~(sol >= 0)).all(axis=1)]  # (all but a freak ray are in range wherever they are active)


def special_rays():
    out = []
    add = lambda o, d: out.append(np.concatenate([np.asarray(o, F), np.asarray(d, F)]))
    for (c, r, _) in SPHERES:
        c, r = np.array(c, F), F(r)
        z = np.array([0, 0, 1], F)
        for dirn in ([0, 0, -1], [0, 0, 1], [0.6, 0, -0.8], [1, 0, 0], [-1, -1, -1], [1, 1, 1]):
            dirn = np.array(dirn, F)
            add(c + z * (r * F(3)), dirn)       # outside: towards, away (both roots negative), grazing, b == 0
            add(c + z * (r * F(0.5)), dirn)     # inside: the second root
            add(c + z * r, dirn)                # on the surface: n1 == 0 or the second root
            add(c, dirn)                        # at the centre: b == +0 and b == -0
            add(c - z * (r * F(3)), dirn)
        zs = c[2] + r                            # origins a few ulp either side of the surface: n1 a few ulp either side of 0
        up, dn = zs, zs
        for _ in range(4):
            up, dn = np.nextafter(up, F(np.inf)), np.nextafter(dn, F(-np.inf))
            for q in (up, dn):
                add([c[0], c[1], q], [0, 0, -1])
                add([c[0], c[1], q], [0, 0, -0.37])
        for ln in (1e-25, 1e-12, 1.0, 1e12, 1e20):  # direction lengths: den underflows, below, inside and above its range
            u = np.array([0.36, -0.48, -0.8], np.float64)
            add(c.astype(np.float64) - u * float(r) * 2.5, u * ln)
            add(c.astype(np.float64) + u * float(r) * 0.25, u * ln)
        add(c + z * (r * F(3)), [np.nan, 0, -1])
        add(c + z * (r * F(0.5)), [0, np.nan, -1])
    # exact tangents from small integers: l = (r, -m, 0), d = (0, +-1, 0): sol = 4 m^2 - 4 (r^2 + m^2 - r^2) == 0 exactly; with
    # d = +y the sphere is ahead (t = m), with d = -y behind (t = -m: sol == 0 keeps the negative t, the reference accepts it)
    for (c, r, _), m in zip(SPHERES[:4] + SPHERES[5:], (2, 2, 2, 2, 32)):
        c = np.array(c, F)
        o = c + np.array([r, -m, 0], F)
        for sgn in (1, -1):
            add(o, [0, sgn, 0])
            add(o, [0, 2 * sgn, 0])
    # the bounds of den's range: |d|^2 = 2^-61 and 2^59 exactly (den on the bound passes), and the floats around them
    for (c, r, _) in SPHERES[:4]:
        c = np.array(c, F)
        for k in (F(2.0 ** -31), F(2.0 ** 29)):
            for kk in (np.nextafter(k, F(0)), k, np.nextafter(k, F(np.inf))):
                add(c - np.array([2 * r, 2 * r, 0], F), [kk, kk, 0])                  # from outside through the centre
                add(c + np.array([r / 4, r / 4, 0], F), [kk, kk, 0])                  # from inside: n1 < 0
    # the lower bound of n1's range, on the tiny sphere at the origin (o - c is exact): o = (0, 0, r + j ulp), d = (0, 0, -k),
    # k ~ 2^-30 (den in range) gives n1 = 2 k j ulp(r), a difference of two floats near 2^-39, so a multiple of 2^-62.
    # With den inside its range a |n1| near 2^-60 only comes from such a cancellation (an n1 that is no difference is
    # ~ k r >= 2^-41 for the smallest sphere here), so the values next to the bound are 3, 4 and 5 times 2^-62, not
    # floats a few ulp from it: the sweep takes what the cancellation gives between 2^-61 and 2^-59, both signs.
    r = F(TINY_R)
    ulp = np.nextafter(r, F(1)) - r
    for k in (F(2.0 ** -30), F(1.25 * 2.0 ** -30), F(1.5 * 2.0 ** -30)):
        cand = np.zeros((17, 6), F)
        cand[:, 2] = r + np.arange(-8, 9, dtype=F) * ulp
        cand[:, 5] = -k
        _, n1, _, _ = model(cand)
        for i in np.nonzero((np.abs(n1[:, 4]) >= LO / 2) & (np.abs(n1[:, 4]) <= LO * 2))[0]:
            out.append(cand[i])
    # ... and the upper bound: heading away from far off, n1 = -(b + s) ~ -2 k (z0 + r) around -2^60 with k = 2^29
    for k in (F(2.0 ** 29),):
        z0 = F(2.0 ** 30)
        for q in (np.nextafter(z0, F(0)), z0, np.nextafter(z0, F(np.inf))):
            for kk in (np.nextafter(k, F(0)), k):
                add([0, 0, q], [0, 0, kk])
    return np.array(out, F)


@pytest.fixture(scope="module")
def batch(oracle):
    """The rays, grouped in waves of 64, with the oracle's answers (computed once)."""
    rng = np.random.default_rng(20260)
    sp = special_rays()
    pool = ordinary_rays(rng, 64 * 2100)
    assert len(pool) >= 64 * 2000
    random_part = pool[:64 * 2000]
    rest = pool[64 * 2000:]
    failer = np.array([0.0, 6.0, 2.0, 0.36e-25, -0.48e-25, -0.8e-25], F)  # a == 0: active on every sphere, out of every range
    groups, where = [], []
    for i, ray in enumerate(sp):
        for with_failer in (True, False):
            g = rest[rng.integers(0, len(rest), 64)].copy()
            lane = (7 * i + 3) % 64
            g[lane] = ray
            if with_failer:
                g[(lane + 29) % 64] = failer
            where.append((len(groups) * 64 + lane, with_failer))
            groups.append(g)
    rays = np.concatenate([np.concatenate(groups), random_part])
    sc = abi.SceneData(spheres=SPHERES)
    return dict(rays=rays, scene=sc, n_special=len(sp), where=where, exp=oracle.trace_rays(sc, rays))


def test_rays_reach_both_votes_and_the_ranges_edges(batch):
    rays = batch["rays"]
    sol, n1, den, ok = model(rays)
    active = sol >= 0
    passing = ok | ~active
    n_groups = 2 * batch["n_special"]
    wave_short = passing[:n_groups * 64].reshape(n_groups, 64, -1).all(axis=1)  # (group, sphere): every active lane in range
    assert not wave_short[0::2].any()   # the groups with the vanishing direction: out of range on every sphere
    assert wave_short[1::2].sum() > 0.8 * wave_short[1::2].size
    second = active & (sol > 0) & (n1 < 0)
    lanes = np.array([w for w, _ in batch["where"]])
    assert (second[lanes].any(axis=1)).sum() > 50 and (active[lanes] & (n1[lanes] == 0)).any()
    assert (active[lanes] & (sol[lanes] == 0) & (n1[lanes] < 0)).any() and (active[lanes] & (sol[lanes] == 0) & (n1[lanes] > 0)).any()
    assert np.isnan(sol[lanes]).any()
    b0 = rays[lanes][:, None, :3] == np.array([s[0] for s in SPHERES], F)[None]  # origin at a centre: b == +-0
    assert b0.all(axis=2).any()
    for bound in (LO, HI):  # den on, below and above each bound
        bb = int(bound.view(np.uint32))
        dd = den[lanes].view(np.uint32).astype(np.int64) - bb
        assert (dd[active[lanes]] == 0).any() and ((dd > 0) & (dd <= 8) & active[lanes]).any() and ((dd < 0) & (dd >= -8) & active[lanes]).any()
    neg = active[lanes] & (n1[lanes] < 0) & (den[lanes] >= LO) & (den[lanes] <= HI)  # n1's own bounds decide
    mag = np.abs(n1[lanes])
    assert ((mag == LO) & neg).any() and ((mag < LO) & (mag >= LO / 2) & neg).any() and ((mag > LO) & (mag <= LO * 2) & neg).any()
    hi_d = mag.view(np.uint32).astype(np.int64) - int(HI.view(np.uint32))
    assert ((hi_d == 0) & neg).any() and ((hi_d > 0) & (hi_d <= 3) & neg).any() and ((hi_d < 0) & (hi_d >= -3) & neg).any()


def test_trace_rays_matches_the_oracle_bit_for_bit(hip, batch):
    et, eo, ei, ed = batch["exp"]
    with hip.HipScene(batch["scene"]) as hs:
        gt, go, gi, gd = hs.trace_rays(batch["rays"])
    bad = (eo != go) | (et.view(np.uint32) != gt.view(np.uint32)) | (ed.view(np.uint32) != gd.view(np.uint32))
    idx = np.nonzero(bad)[0]
    assert len(idx) == 0, [(int(i), batch["rays"][i].tolist(), int(eo[i]), int(go[i]), float(et[i]), float(gt[i])) for i in idx[:6]]
    assert (eo >= 0).sum() > len(eo) // 2 and len(set(eo.tolist())) == len(SPHERES) + 1  # every sphere is hit, and something misses


@pytest.mark.parametrize("max_depth", [3, 4, 5, 9])
def test_fold_word_boundaries_between_two_mirrors(hip, oracle, max_depth):
    """64x64, 4 spp, the camera between two metal spheres: paths bounce until max_depth runs out, so their attenuation folds
    over max_depth records: three in the word in hand, one full word, a full word and one, two full words and one."""
    mirror = lambda c, col: (c, 6.0, abi.material(abi.MAT_METAL, col, 0.0))
    sc = abi.SceneData(spheres=[mirror((-6.5, 0.0, 0.0), (0.9, 0.8, 0.7)), mirror((6.5, 0.0, 0.0), (0.7, 0.8, 0.9)),
                                ((0.0, -1000.5, 0.0), 1000.0, abi.material(abi.MAT_LAMBERTIAN, (0.4, 0.5, 0.3)))])
    cam = scenes.camera(oracle, 64, 64, position=(0.0, 0.2, 0.0), look_at=(1.0, 0.1, 0.15), up=(0.0, 1.0, 0.0))
    exp, exp8, _ = oracle.render(cam, sc, abi.default_opts(spp=4, seed=11, max_depth=max_depth))
    got, got8 = hip.render_scene(cam, 4, sc, seed=11, max_depth=max_depth)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), int((got.view(np.uint32) != exp.view(np.uint32)).any(axis=-1).sum())
    assert np.array_equal(got8, exp8)
    # some path uses its last bounce, so its fold runs over max_depth records: one bounce less gives another image
    shallower, _, _ = oracle.render(cam, sc, abi.default_opts(spp=4, seed=11, max_depth=max_depth - 1))
    assert not np.array_equal(exp, shallower)
