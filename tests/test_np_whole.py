"""np_whole.py, the joined restatement of every per-sample feature, pinned without a GPU: with the other features off it is each
single-feature restatement bit for bit, with none of the five new ones it is the CPU oracle's extended render, and one path
through everything -- a lens and a shutter in front, a patterned sphere advanced by phase + t, an odd cell, a bounce into a
noise environment -- is evaluated by hand with Python floats rounded through struct. Also here, from the descriptors of
whole_scenes.fuzz_case over the seeds tests/test_whole_gpu.py runs: every pair of features occurs together, a third of the
patterned cases reach both colours of an object, and no sample meets a NaN discriminant."""
from __future__ import annotations

import functools
import itertools
import math
import struct

import numpy as np
import pytest

import full_scenes as F
import np_animation as NA
import np_env
import np_full
import np_motion as NM
import np_pattern
import np_reference as R
import np_shutter as NS
import np_whole as NW
import scenes
import test_np_motion as TM
import test_np_pattern as TP
import whole_scenes as WS
from rbrt_amd import abi

f32 = np.float32
W, H, SPP = 7, 5, 2
LENS = TM.LENS
SKEW = TM.SKEW


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])


# ---- reductions ---------------------------------------------------------------------------------------------------------------------
def test_without_the_new_features_it_is_np_full(oracle):
    cam, lens = F.all_features_camera(oracle, W, H)
    sc, opts = F.all_features_scene(oracle), F.all_features_opts(SPP, 6)
    assert same(NW.restated_image(cam, sc, opts, lens=lens), np_full.restated_image(cam, sc, opts, lens=lens))
    assert same(NW.restated_image(cam, sc, opts), np_full.restated_image(cam, sc, opts))


def test_with_patterns_alone_it_is_np_pattern(oracle):
    cam = scenes.camera(oracle, W, H)
    sc = TP._sphere_scene(abi.checker((0.8, 0.8, 0.7), 0.7, (0.1, -1.0, 0.3)))
    opts = abi.default_opts(spp=SPP, seed=4, max_depth=6)
    for lens in (None, LENS):
        ta, tb = {}, {}
        assert same(NW.restated_image(cam, sc, opts, lens=lens, traces=ta), np_pattern.restated_image(cam, sc, opts, lens=lens, traces=tb))
        assert ta == tb and any((0, 1) in v for v in ta.values()) and any((0, 0) in v for v in ta.values())


def test_with_an_environment_alone_it_is_np_env(oracle):
    cam = scenes.camera(oracle, W, H)
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(abi.MAT_EMISSIVE, (3.0, 2.5, 1.5)))])
    nodes = np_env.noise_map(8, 3)
    # (bg and the constant flag are set and ignored: np_env reads neither)
    opts = abi.default_opts(spp=SPP, seed=5, max_depth=6, bg=(0.9, 0.1, 0.4), flags=abi.FLAG_CONSTANT_BACKGROUND)
    for lens in (None, LENS):
        assert same(NW.restated_image(cam, sc, opts, lens=lens, nodes=nodes), np_env.restated_image(cam, sc, opts, nodes, lens=lens))
    assert not same(NW.restated_image(cam, sc, opts, nodes=nodes), NW.restated_image(cam, sc, opts))


def test_with_a_shutter_alone_it_is_np_shutter(oracle):
    cam = scenes.camera(oracle, W, H)
    sc, opts = TM.small_scene(), abi.default_opts(spp=SPP, seed=6, max_depth=6)
    for lens, travel in ((None, SKEW), (LENS, SKEW), (LENS, (0.0, 0.0, 0.0)), (LENS, None)):
        assert same(NW.restated_image(cam, sc, opts, lens=lens, shutter=travel), NS.restated_image(cam, sc, opts, lens, travel))
    # a phase without a motion has no effect
    assert same(NW.restated_image(cam, sc, opts, shutter=SKEW, phase=7.0), NS.restated_image(cam, sc, opts, None, SKEW))


def test_with_a_motion_alone_it_is_np_motion_and_at_a_phase_np_animation(oracle):
    cam = scenes.camera(oracle, W, H)
    sc, opts = TM.small_scene(), abi.default_opts(spp=SPP, seed=7, max_depth=6)
    tv = TM.small_travels(len(sc.spheres))
    for lens, shutter in ((None, None), (LENS, SKEW)):
        assert same(NW.restated_image(cam, sc, opts, lens=lens, shutter=shutter, travels=tv), NM.restated_image(cam, sc, opts, tv, lens=lens, shutter=shutter))
        for phase in (0.5, -3.0, 4096.25):
            assert same(NW.restated_image(cam, sc, opts, lens=lens, shutter=shutter, travels=tv, phase=phase),
                        NA.restated_image(cam, sc, opts, tv, phase, lens=lens, shutter=shutter))
    nodes = np_env.noise_map(2, 9)
    assert same(NW.restated_image(cam, sc, opts, travels=tv, phase=0.5, nodes=nodes), NA.restated_image(cam, sc, opts, tv, 0.5, nodes=nodes))


@pytest.mark.parametrize("seed", [5, 12, 13])
def test_with_none_of_the_new_features_it_is_the_oracle(oracle, seed):
    """full_scenes' tiny cases: a lens with emitters (5), a flat and a smooth lambertian mesh (12), a lens and a smooth mesh (13)."""
    case = F.fuzz_case(oracle, seed, tiny=True)
    nan0 = oracle.lib().rbrt_oracle_nan_discriminants()
    exp, exp8, _ = oracle.render(case["cam"], case["sc"], case["opts"], lens=case["lens"])
    assert oracle.lib().rbrt_oracle_nan_discriminants() == nan0
    got, got8 = NW.restated_image(case["cam"], case["sc"], case["opts"], lens=case["lens"])
    assert F.same_bits(got, exp) and np.array_equal(got8, exp8), case["what"]


def test_the_features_reduce_to_np_animations_and_take_the_cells_colour(oracle):
    """No pattern: np_animation.features as it was. A pattern with equal colours: the same buffers. Two colours: the albedo alone
    changes, and only where the patterned object is hit."""
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=SPP, seed=5)
    tv = TM.small_travels(5)
    plain = TP._sphere_scene(None)
    a1 = tuple(plain.spheres[0][2].albedo)
    for sc, changes in ((TP._sphere_scene(abi.checker(a1, 0.3, (0.1, 0.2, 0.3))), False), (TP._sphere_scene(abi.checker((0.9, 0.8, 0.1), 0.3, (0.1, 0.2, 0.3))), True)):
        exp, exp_mv = NA.features(cam, plain, opts, 3, tv, 0.5, lens=LENS, shutter=SKEW)
        got, got_mv = NW.features(cam, sc, opts, 3, lens=LENS, shutter=SKEW, travels=tv, phase=0.5)
        for k in ("normal", "depth", "coverage"):
            assert np.array_equal(bits(getattr(got, k)), bits(getattr(exp, k))), k
        assert np.array_equal(got.object, exp.object) and np.array_equal(bits(got_mv), bits(exp_mv))
        differs = (bits(got.albedo) != bits(exp.albedo)).any(-1)
        assert differs.any() == changes and not differs[exp.coverage == 0].any()
    # a shutter without a motion: the shutter's rays, an all +0 motion buffer
    got, mv = NW.features(cam, plain, opts, 3, shutter=SKEW)
    still, _ = NW.features(cam, plain, opts, 3)
    assert not bits(mv).any() and not np.array_equal(bits(got.depth), bits(still.depth))


# ---- one path by hand ---------------------------------------------------------------------------------------------------------------
def r(x):
    """A Python float rounded to float32: a double sum, product, quotient or square root of float32 values rounds once more."""
    return struct.unpack("f", struct.pack("f", x))[0]


M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


class Stream:
    """The build's random stream (DESIGN.md "RNG"), with Python integers."""

    def __init__(self, seed, pixel, sample):
        def mix(x):
            x = (x + 0x9E3779B97F4A7C15) & M64
            x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
            x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
            return x ^ (x >> 31)
        key = mix(mix(seed) ^ ((pixel << 32) | sample))
        self.a, self.b = key & M32, key >> 32
        assert self.a or self.b

    def next(self):
        rot = lambda x, k: ((x << k) | (x >> (32 - k))) & M32  # noqa: E731
        out = (rot((self.a * 0x9E3779BB) & M32, 5) * 5) & M32
        t = self.b ^ self.a
        self.a = rot(self.a, 26) ^ t ^ ((t << 9) & M32)
        self.b = rot(t, 13)
        return (out >> 8) * 2.0 ** -24


def v_dot(a, b):
    return r(r(r(a[0] * b[0]) + r(a[1] * b[1])) + r(a[2] * b[2]))


def v_unit(a):
    ln = r(math.sqrt(v_dot(a, a)))
    return [r(c / ln) for c in a]


def hand_sphere(o, d, c, radius, lo, hi):
    """sphere.rs:20-66 -> None or (p, t)."""
    a = v_dot(d, d)
    l = [r(o[k] - c[k]) for k in range(3)]
    b = v_dot([r(x * 2.0) for x in d], l)
    cc = r(v_dot(l, l) - r(radius * radius))
    sol = r(r(b * b) - r(r(4.0 * a) * cc))
    assert not math.isnan(sol)
    if sol < 0.0:
        return None
    t = r(r(-b - r(math.sqrt(sol))) / r(2.0 * a))
    if sol > 0.0 and t < 0.0:
        t = r(r(-b + r(math.sqrt(sol))) / r(2.0 * a))
        if t < 0.0:
            return None
    p = [r(o[k] + r(t * d[k])) for k in range(3)]
    q = [r(o[k] - p[k]) for k in range(3)]
    dist = r(math.sqrt(v_dot(q, q)))
    if dist < lo or dist > hi:
        return None
    return p, t


def hand_environment(E, d):
    n = E.shape[0] - 1
    s = r(r(abs(d[0]) + abs(d[1])) + abs(d[2]))
    px, py, pz = (r(c / s) for c in d)
    if py >= 0.0:
        u, v = px, pz
    else:
        u, v = r(r(1.0 - abs(pz)) * (1.0 if px >= 0.0 else -1.0)), r(r(1.0 - abs(px)) * (1.0 if pz >= 0.0 else -1.0))
    x, y = r(r(r(u * 0.5) + 0.5) * float(n)), r(r(r(v * 0.5) + 0.5) * float(n))
    i, j = (min(int(math.floor(x)), n - 1) if x >= 0.0 else 0), (min(int(math.floor(y)), n - 1) if y >= 0.0 else 0)
    fx, fy = r(x - float(i)), r(y - float(j))
    out = []
    for c in range(3):
        e = lambda jj, ii: float(E[jj, ii, c])  # noqa: E731
        top = r(e(j, i) + r(fx * r(e(j, i + 1) - e(j, i))))
        bot = r(e(j + 1, i) + r(fx * r(e(j + 1, i + 1) - e(j + 1, i))))
        out.append(r(top + r(fy * r(bot - top))))
    return out


HAND = dict(centre=(0.5, 1.0, -8.0), radius=2.5, albedo=(0.7, 0.4, 0.3), albedo2=(0.1, 0.9, 0.5), size=0.37, origin=(0.11, -0.07, 0.23),
            travel=(0.02, -0.01, 0.03), phase=7.0, row=2, col=3)


def hand_path(cam, seed, nodes):
    """One sample of pixel (HAND row, col) through lens, shutter, the advanced sphere, its cell and the environment: None if the
    camera ray misses or the bounce hits again, else (odd, radiance)."""
    f = lambda a: [float(x) for x in a]  # noqa: E731
    pos, right, up, ctr = f(cam.position), f(cam.right), f(cam.up), f(cam.img_center_point)
    w, h, row, col = cam.img_width_pix, cam.img_height_pix, HAND["row"], HAND["col"]
    rng = Stream(seed, row * w + col, 0)
    col_mm = r(r(r(float(col - w // 2) + rng.next()) - 0.5) * float(cam.mm_per_pix_hor))
    row_mm = r(r(r(float(row - h // 2) + rng.next()) - 0.5) * float(cam.mm_per_pix_vert))
    k = r(0.001)
    target = [r(r(ctr[c] + r(r(k * col_mm) * right[c])) - r(r(k * row_mm) * up[c])) for c in range(3)]
    while True:
        lx = r(r(2.0 * rng.next()) - 1.0)
        ly = r(r(2.0 * rng.next()) - 1.0)
        if r(r(lx * lx) + r(ly * ly)) < 1.0:
            break
    lu, lv, fs = [r(x) for x in LENS[0]], [r(x) for x in LENS[1]], r(LENS[2])
    o = [r(pos[c] + r(r(lx * lu[c]) + r(ly * lv[c]))) for c in range(3)]
    focus = [r(pos[c] + r(fs * r(target[c] - pos[c]))) for c in range(3)]
    d = v_unit([r(focus[c] - o[c]) for c in range(3)])
    t = rng.next()
    o = [r(o[c] + r(t * r(SKEW[c]))) for c in range(3)]
    s = r(r(HAND["phase"]) + t)
    centre = [r(r(HAND["centre"][c]) + r(s * r(HAND["travel"][c]))) for c in range(3)]
    radius = r(HAND["radius"])
    hit = hand_sphere(o, d, centre, radius, r(0.001), r(2000.0))
    if hit is None:
        return None
    p, _ = hit
    inv = r(1.0 / r(HAND["size"]))
    odd = 0
    for c in range(3):
        odd ^= int(math.floor(min(max(r(r(p[c] - r(HAND["origin"][c])) * inv), -1e9), 1e9))) & 1
    nhat = v_unit([r(p[c] - centre[c]) for c in range(3)])
    while True:
        q = [r(r(2.0 * rng.next()) - 1.0) for _ in range(3)]
        if not r(math.sqrt(v_dot(q, q))) > 1.0:
            break
    nd = v_unit([r(r(r(p[c] + nhat[c]) + q[c]) - p[c]) for c in range(3)])
    if hand_sphere(p, nd, centre, radius, r(0.001), r(2000.0)) is not None:
        return None
    L = hand_environment(nodes, nd)
    a = HAND["albedo2"] if odd else HAND["albedo"]
    return odd, [r(r(a[c]) * L[c]) for c in range(3)]


def test_one_path_through_everything_by_hand(oracle):
    """The first seeds whose sample hits the sphere and escapes: the cell's parity and the radiance to the bit, in odd cells and in
    even ones. The sphere has travelled 7.x exposures; the unmoved one would be hit 0.3 units elsewhere."""
    cam = scenes.camera(oracle, W, H)
    nodes = np_env.noise_map(8, 3)
    sc = abi.SceneData(spheres=[(HAND["centre"], HAND["radius"], abi.material(abi.MAT_LAMBERTIAN, HAND["albedo"]))],
                       patterns={0: abi.checker(HAND["albedo2"], HAND["size"], HAND["origin"])})
    seen = {0: 0, 1: 0}
    for seed in range(1, 40):
        hand = hand_path(cam, seed, nodes)
        if hand is None:
            continue
        odd, want = hand
        # (bg and the flag are set: the environment takes their place)
        opts = abi.default_opts(spp=1, seed=seed, max_depth=3, bg=(0.3, 0.6, 0.9), flags=abi.FLAG_CONSTANT_BACKGROUND)
        tr = {}
        got, _ = NW.restated_image(cam, sc, opts, lens=LENS, shutter=SKEW, travels=[HAND["travel"]], phase=HAND["phase"], nodes=nodes,
                                   pixels=[(HAND["row"], HAND["col"])], traces=tr)
        assert tr[(HAND["row"], HAND["col"], 0)] == [(0, odd)], seed
        assert np.array_equal(bits(got[HAND["row"], HAND["col"]]), bits(np.array(want, f32))), (seed, odd)
        seen[odd] += 1
        if seen[0] >= 2 and seen[1] >= 2:
            break
    assert seen[0] >= 2 and seen[1] >= 2, seen


# ---- the generator, from its descriptors ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_cases():
    """Every case of the GPU fuzz with its restated image, traces and NaN flag, made once."""
    from oracle import pyoracle
    out = []
    for seed in range(WS.N_FUZZ):
        case = WS.fuzz_case(pyoracle, seed)
        traces, nan = {}, False
        try:
            WS.restate(NW, case, traces=traces)
        except R.NanDiscriminant:
            nan = True
        out.append((case, traces, nan))
    return out


def test_every_pair_of_features_occurs_together():
    cases = [c for c, _, _ in restated_cases()]
    missing = [(a, b) for a, b in itertools.combinations(WS.FEATURES, 2) if not any(a in c.has and b in c.has for c in cases)]
    assert not missing, missing
    # ... and what the generator promises beside the pairs
    assert {(None if c.shutter is None else "zero" if not any(c.shutter) else "small" if max(map(abs, c.shutter)) < 0.5 else "large") for c in cases} == {None, "zero", "small", "large"}
    assert any(c.travels is None for c in cases)
    zero = cases[WS.ZERO_MOTION_SEED]
    assert zero.travels is not None and len(zero.travels) and not zero.travels.any()
    moving = [c for c in cases if c.travels is not None and c.travels.any()]
    assert any((np.linalg.norm(c.travels, axis=1) >= 30.0).any() for c in moving) and any((~c.travels.any(axis=1)).any() for c in moving)
    assert {c.phase for c in cases} == set(WS.PHASES)
    assert {c.nodes.shape[0] - 1 for c in cases if c.nodes is not None} == {1, 2, 8}
    assert all(any(c.opts.bg) for c in cases if c.nodes is not None)
    equal = cases[WS.EQUAL_COLOURS_SEED]
    mats = WS.object_materials(equal.sc)
    assert equal.patterns and all(tuple(p.albedo2) == tuple(mats[k].albedo) for k, p in equal.patterns.items())
    sizes = [p.size for c in cases for p in c.patterns.values()]
    assert min(sizes) < 0.01 and max(sizes) > 50.0
    assert all(c.cam.img_width_pix <= 12 and c.cam.img_height_pix <= 9 and c.opts.spp <= 2 and c.opts.max_depth in (0, 1, 3) for c in cases)
    assert all(len(c.sc.spheres) + len(c.sc.triangles) + len(c.sc.meshes) <= 255 and len(c.sc.meshes) <= 7 for c in cases)


def test_a_third_of_the_patterned_cases_reach_both_colours():
    patterned = both = 0
    for case, traces, _ in restated_cases():
        if not case.patterns:
            continue
        patterned += 1
        seen = {}
        for tr in traces.values():
            for obj, second in tr:
                seen.setdefault(obj, set()).add(second)
        both += any(len(v) == 2 for v in seen.values())
    print(f"{both} of {patterned} patterned cases record both colours of one object")
    assert patterned >= WS.N_FUZZ // 2 and 3 * both >= patterned, (both, patterned)


def test_the_walk_sets_replaces_and_clears_every_part_of_the_state():
    """whole_scenes.walk, the sequence test_whole_gpu.py walks one handle through: sixteen changes, each of which changes the state."""
    steps = WS.walk()
    assert len(steps) == 16 and {w.split()[-1] for w, _ in steps} == set(WS.KINDS)
    assert {w.split()[0] for w, _ in steps} == {"set", "replace", "clear", "change", "swap"}
    start = dict(shutter=None, motion=None, phase=0, environment=None, camera=0, lens=0)
    assert all(a != b for a, b in zip([start] + [s for _, s in steps], [s for _, s in steps]))
    # two parts of the key in turn: somewhere both a shutter and a motion are set while the phase, the camera or the lens changes
    assert any(s["shutter"] is not None and s["motion"] is not None and w.split()[-1] in ("phase", "camera", "lens") for w, s in steps)


def test_no_case_meets_a_nan_discriminant():
    assert not [c.what for c, _, nan in restated_cases() if nan]
