"""np_pattern.py, the numpy restatement of the solid checker, pinned without a GPU: against a scalar evaluation with Python
integers and math.floor on the float32 products, by the exact properties of power-of-two sizes (a step of one cell flips the
colour, two keep it; swapping the colours and shifting the origin by a cell changes nothing), by np_smooth's image for equal
colours, and at NaN, infinite and out-of-range coordinates."""
import math

import numpy as np
import pytest

import np_pattern as NP
import np_smooth
import scenes
from rbrt_amd import abi

f32 = np.float32
L, M, D, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE


def scalar_odd(p, origin, size):
    """The rule with Python integers: float32 only where the rule says float32."""
    inv = f32(1.0) / f32(size)
    par = 0
    for c in range(3):
        t = f32(f32(f32(p[c]) - f32(origin[c])) * inv)
        if math.isnan(float(t)):
            u = -1e9
        else:
            u = min(max(float(t), -1e9), 1e9)
        par ^= int(math.floor(u)) & 1  # (Python's & on a negative integer is two's complement: the parity of k)
    return par


def test_the_rule_against_a_scalar_evaluation():
    rng = np.random.default_rng(11)
    for size, origin in ((0.3, (0.11, -0.07, 0.23)), (2.0, (0.0, -1.0, 0.0)), (1e-3, (5.0, 5.0, 5.0)), (7.5, (-100.0, 3.0, 0.5))):
        pts = rng.uniform(-20, 20, (400, 3)).astype(f32)
        # points on and one ulp either side of cell faces
        k = rng.integers(-30, 30, (100, 3))
        on = (np.asarray(origin, f32) + (k * f32(size)).astype(f32)).astype(f32)
        pts = np.concatenate([pts, on, np.nextafter(on, f32(np.inf)), np.nextafter(on, f32(-np.inf))])
        got = NP.odd(pts, origin, size)
        exp = np.array([scalar_odd(p, origin, size) for p in pts])
        assert np.array_equal(got, exp)
        assert 0 < got.sum() < len(got)


@pytest.mark.parametrize("size", [0.25, 1.0, 8.0])
def test_a_step_of_one_cell_flips_and_two_cells_keep(size):
    rng = np.random.default_rng(5)
    origin = np.array([0.5, -2.0, 16.0], f32)  # (small dyadic numbers, like the points: every difference and product is exact)
    pts = (rng.integers(-4000, 4000, (500, 3)) * f32(size / 16)).astype(f32)  # exact multiples of size / 16
    base = NP.odd(pts, origin, size)
    for axis in range(3):
        for sign in (-1.0, 1.0):
            step = np.zeros(3, f32)
            step[axis] = f32(sign * size)
            assert np.array_equal(NP.odd(pts + step, origin, size), base ^ 1)
            assert np.array_equal(NP.odd(pts + step + step, origin, size), base)


def _sphere_scene(pattern, ground_albedo=(0.02, 0.2, 0.1)):
    spheres = [((0.0, -1000.0, -5.0), 1000.0, abi.material(L, ground_albedo)),
               ((-5.0, 1.5, -9.0), 1.5, abi.material(L, (0.1, 0.1, 0.9))),
               ((-2.5, 2.9, -15.0), 3.0, abi.material(M, (0.8, 0.8, 0.8), 0.005)),
               ((1.5, 1.25, -9.0), 1.5, abi.material(D, (0, 0, 0), 1.8)),
               ((4.0, 0.6, -8.0), 0.6, abi.material(EM, (0.5, 3.0, 3.0)))]
    return abi.SceneData(spheres=spheres, patterns=None if pattern is None else {0: pattern})


def test_swapped_colours_and_a_shifted_origin_leave_the_image_unchanged(oracle):
    cam = scenes.camera(oracle, 12, 8)
    opts = abi.default_opts(spp=2, seed=4, max_depth=6)
    a1, a2 = (0.02, 0.2, 0.1), (0.8, 0.8, 0.7)
    one = _sphere_scene(abi.checker(a2, 2.0, (0.0, -1.0, 0.0)), a1)
    imgs = [NP.restated_image(cam, one, opts)[0]]
    for shift in ((2.0, 0, 0), (0, -2.0, 0), (0, 0, 2.0)):
        origin = tuple(np.array((0.0, -1.0, 0.0)) + np.array(shift))
        imgs.append(NP.restated_image(cam, _sphere_scene(abi.checker(a1, 2.0, origin), a2), opts)[0])
    for im in imgs[1:]:
        assert np.array_equal(im.view(np.uint32), imgs[0].view(np.uint32))
    plain = np_smooth.restated_image(cam, _sphere_scene(None, a1), opts)[0]
    assert not np.array_equal(plain, imgs[0])  # (the pattern shows)


def test_equal_colours_reproduce_np_smooth(oracle):
    cam = scenes.camera(oracle, 12, 8)
    opts = abi.default_opts(spp=2, seed=4, max_depth=6)
    a1 = (0.02, 0.2, 0.1)
    got = NP.restated_image(cam, _sphere_scene(abi.checker(a1, 0.3, (0.1, 0.2, 0.3)), a1), opts)
    exp = np_smooth.restated_image(cam, _sphere_scene(None, a1), opts)
    assert np.array_equal(got[0].view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(got[1], exp[1])
    # ... and np_smooth's image is the oracle's (the anchor of the whole chain)
    ora = oracle.render(cam, _sphere_scene(None, a1), opts)[0]
    assert np.array_equal(exp[0].view(np.uint32), ora.view(np.uint32))


def test_nan_infinite_and_far_coordinates_give_the_documented_cell():
    size, origin = 0.5, (0.0, 0.0, 0.0)
    inside = 0.25  # cell 0 on the other two axes
    lo, hi = -1000000000, 1000000000  # int32(floor(-1e9f)), int32(floor(1e9f)): both even
    for x, k in ((np.nan, lo), (-np.inf, lo), (np.inf, hi), (-6e8, lo), (6e8, hi), (-3e38, lo), (3e38, hi), (0.75, 1), (-0.25, -1)):
        for axis in range(3):
            p = np.full(3, inside, f32)
            p[axis] = x
            cells = NP.cells(p, origin, size)
            assert cells[axis] == k and all(cells[a] == 0 for a in range(3) if a != axis), (x, axis, cells)
            assert int(NP.odd(p, origin, size)) == (k & 1)
    # beyond +-1e9 * size the products clamp: a step of one cell no longer flips anything
    far = np.array([6e8, 0.25, 0.25], f32)
    assert int(NP.odd(far, origin, size)) == int(NP.odd(far + np.array([64.0, 0, 0], f32), origin, size)) == 0
