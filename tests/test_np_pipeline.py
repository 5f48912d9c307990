"""np_pipeline.py can tell right from wrong (no GPU): with every stage off it is the plain mix of the halves; on the frozen rows of
pipeline_cases.py every optional stage changes the final image, and so does each swap of two stages, the mix 0.5 in place of an
odd count's, and the full camera in place of the low one. A GPU comparison fed such inputs therefore notices those mistakes.

The samples here are stand-ins made with the CPU oracle: sample s of a frame is the difference of its renders at s + 1 and at s
samples a pixel, each times its count (a sample's stream does not depend on the count). That is the GPU's sample s up to the
rounding of the two means, so a row that meets its conditions here is expected to meet them on the GPU, where they are asserted
again on the exact samples. The features are np_features' own."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import np_adaptive
import np_denoise
import np_features
import np_pipeline as P
import np_upsample
import pipeline_cases as PC
import scenes

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def same(got, exp):
    return np.array_equal(bits(got), bits(exp))


@functools.lru_cache(maxsize=None)
def _inputs(name):
    from oracle import pyoracle as oracle
    oracle.lib()
    r = PC.ROWS[name]
    sc = PC.scene_of(oracle, r)
    cam0 = scenes.camera(oracle, r.w, r.h)
    lens = PC.lens_of(r, cam0)
    frames = []
    for k in range(r.frames):
        full, traced = PC.cameras(r, cam0, k)
        seed = P.frame_seed(r.seed, k)
        sums = [np.zeros((traced.img_height_pix, traced.img_width_pix, 3))]
        sums += [oracle.render(traced, sc, PC.opts_of(r, m, seed), want_rgb8=False, lens=lens)[0].astype(np.float64) * m for m in range(1, r.n + 1)]
        samples = np.stack([np.maximum(sums[s + 1] - sums[s], 0.0) for s in range(r.n)]).astype(f32)
        ft = np_features.features(oracle, full, sc, PC.opts_of(r, r.n, seed), PC.FEATURE_SAMPLES, lens)
        for x in (samples, *ft):
            x.flags.writeable = False
        frames.append(P.frame(samples, ft.albedo, ft.normal, ft.depth, ft.coverage, full))
    return r, frames


@functools.lru_cache(maxsize=None)
def _result(name):
    r, frames = _inputs(name)
    return P.pipeline(frames, PC.options(r))


def replicated(fr, f, w, h):
    """The frame with its low samples repeated over their blocks: what a render without guided upsampling would be fed."""
    s = np.repeat(np.repeat(fr.samples, f, axis=1), f, axis=2)[:, :h, :w]
    return P.frame(s, fr.albedo, fr.normal, fr.depth, fr.coverage, fr.cam)


# ---- 1. the host's own arithmetic -----------------------------------------------------------------------------------------------------
def test_mix_weight_seed_and_maps():
    assert P.mix_weight(6) == f32(0.5) and P.mix_weight(2) == f32(0.5)
    assert P.mix_weight(5) == f32(3) * (f32(1) / f32(5)) and P.mix_weight(5) != f32(0.5) and P.mix_weight(5).dtype == f32
    assert P.mix_weight(7) == f32(4) * (f32(1) / f32(7)) and P.mix_weight(7) != f32(0.5)
    assert P.frame_seed(3, 0) == 3 and P.frame_seed(3, 2) == 5
    assert list(P.spike_map(np.array([0, 1, 2, 3, 7], np.uint8))) == [0, 85, 170, 255, 255]
    length = np.array([0.0, 1.0, 16.0, 31.9, 32.0, 40.0, np.nan, -1.0], f32)
    assert list(P.history_map(length, 32.0)) == [0, 7, 127, 254, 255, 255, 0, 0]


def test_frame_camera_moves_position_and_image_centre_alone(oracle):
    cam = scenes.camera(oracle, 50, 47)
    moved = P.frame_camera(cam, (0.03, 0.0, -0.5), 2)
    for c, step in enumerate((0.03, 0.0, -0.5)):
        shift = f32(2) * f32(step)
        assert f32(moved.position[c]) == f32(cam.position[c]) + shift and f32(moved.img_center_point[c]) == f32(cam.img_center_point[c]) + shift
    assert bytes(P.frame_camera(cam, (0.03, 0.0, -0.5), 0)) == bytes(cam) and bytes(moved) != bytes(cam)
    assert (list(moved.right), list(moved.up), moved.mm_per_pix_hor, moved.img_width_pix) == (list(cam.right), list(cam.up), cam.mm_per_pix_hor, 50)


# ---- 2. every stage off -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 6])
def test_every_stage_off_is_the_mix_of_the_halves(oracle, n):
    rng = np.random.default_rng(n)
    w, h = 13, 9
    samples = rng.gamma(0.7, 1.5, (n, h, w, 3)).astype(f32)
    z = np.zeros((h, w), f32)
    res = P.pipeline([P.frame(samples, np.zeros((h, w, 3), f32), np.zeros((h, w, 3), f32), z, z, scenes.camera(oracle, w, h))], P.options())
    counts = np.full(np_adaptive.tile_grid(h, w), n, np.uint32)
    a, b, wa = np_denoise.halves(*np_denoise.halves_from_samples(samples, counts), counts)
    assert same(res.filtered, np_denoise.mix(a, b, wa)) and same(res.frames[0].raw_a, a) and same(res.frames[0].raw_b, b)
    assert np.array_equal(res.final8, np_adaptive.quantise(np_denoise.mix(a, b, wa))) and np.array_equal(res.noisy_final8, res.frames[0].own8)
    assert res.spike_map is None and res.history_map is None and res.glared is None and res.chosen is None and res.compare is None
    assert (res.render_width, res.render_height) == (w, h) and (wa == P.mix_weight(n)).all()


# ---- 3. the frozen rows: every stage and the order matter ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(PC.ROWS))
def test_the_rows_meet_their_conditions_with_the_stand_in_samples(name):
    r, frames = _inputs(name)
    res = _result(name)
    PC.check_conditions(name, r, res, frames)
    assert (res.render_width, res.render_height) == (np_upsample.low_size(r.w, r.h, r.f) if r.f else (r.w, r.h))
    assert (res.wa != f32(0.5)) == (r.n % 2 == 1)
    assert np.isfinite(res.filtered).all() and res.final8.shape == (r.h, r.w, 3)


@pytest.mark.parametrize("name", list(PC.ROWS))
def test_each_optional_stage_changes_the_final_image(name):
    r, frames = _inputs(name)
    base = _result(name)
    o = lambda **kw: P.options(**dict(dict(upscale=r.f, despike=r.despike, frames=r.frames, end=r.end, nlm=r.nlm, guided=r.guided, glare=r.glare,
                                          tonemap=r.tonemap), **kw))
    if r.despike is not None:
        assert not np.array_equal(P.pipeline(frames, o(despike=None)).final8, base.final8), "despike"
    if r.f:
        assert not np.array_equal(P.pipeline([replicated(fr, r.f, r.w, r.h) for fr in frames], o(upscale=0)).final8, base.final8), "upscale"
    if r.frames > 1:
        assert not np.array_equal(P.pipeline(frames[-1:], o(frames=0)).final8, base.final8), "frames"
    else:  # one frame: the accumulation passes the halves through
        assert np.array_equal(P.pipeline(frames[-1:], o(frames=0)).final8, base.final8)
    if r.end != "mix":
        assert not np.array_equal(P.pipeline(frames, o(end="mix")).final8, base.final8), r.end
    if r.glare is not None:
        assert not np.array_equal(P.pipeline(frames, o(glare=None)).final8, base.final8), "glare"
    if r.tonemap is not None:
        assert not np.array_equal(P.pipeline(frames, o(tonemap=None)).final8, base.final8), "tonemap"
    plain_upsampled = r.f and r.frames == 1 and r.end == "mix"  # (then the target IS the mix of the upsampled halves)
    assert np.array_equal(base.noisy_final8, base.final8) == bool(plain_upsampled)


@pytest.mark.parametrize("name", ["all-3", "all-2"])
def test_the_order_of_the_stages_matters(name):
    r, frames = _inputs(name)
    base = _result(name)
    o = PC.options(r)
    late_despike = P.pipeline(frames, o, order=("upsample", "despike", "accumulate"))
    early_accumulation = P.pipeline(frames, o, order=("despike", "accumulate", "upsample"))
    late_glare = P.pipeline(frames, o, display_order=("tonemap", "glare"))
    for what, other in (("despike behind upsampling", late_despike), ("accumulation in front of upsampling", early_accumulation),
                        ("glare behind the display transform", late_glare)):
        assert not np.array_equal(other.final8, base.final8), what
    assert not same(late_despike.filtered, base.filtered) and not same(early_accumulation.filtered, base.filtered)
    assert same(late_glare.filtered, base.filtered)  # (the display stages leave the linear radiance alone)


def test_the_gpu_comparison_names_the_first_stage_that_differs():
    """test_pipeline_gpu.differences, fed a composition with two stages swapped in place of the library's chain: equal up to the
    swap, and everything behind it listed."""
    from test_pipeline_gpu import differences, planted
    r, frames = _inputs("all-3")
    ref = planted(_result("all-3").noisy)
    right = P.pipeline(frames, PC.options(r), ref)
    assert differences(right, right, r) == []
    late_despike = differences(P.pipeline(frames, PC.options(r), ref, order=("upsample", "despike", "accumulate")), right, r)
    assert late_despike[0] == "frame 0: despiked A" and "final 8-bit image" in late_despike and "comparison result" in late_despike
    late_glare = differences(P.pipeline(frames, PC.options(r), ref, display_order=("tonemap", "glare")), right, r)
    assert late_glare[0] == "glared radiance" and "final 8-bit image" in late_glare and "comparison result" not in late_glare
    half = differences(P.pipeline(frames, PC.options(r), ref, wa_value=0.5), right, r)
    assert half[0] == "frame 0: unfiltered image" and "filtered radiance" in half


@pytest.mark.parametrize("name", [k for k, r in PC.ROWS.items() if r.n % 2])
def test_an_odd_count_does_not_mix_by_halves(name):
    r, frames = _inputs(name)
    base = _result(name)
    assert base.wa != f32(0.5)
    half = P.pipeline(frames, PC.options(r), wa_value=0.5)
    assert not same(half.filtered, base.filtered) and not np.array_equal(half.final8, base.final8)


# ---- 4. the low camera ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("w,h", [(50, 47), (37, 21), (9, 7)])
def test_the_low_camera_is_another_camera(oracle, w, h, f):
    assert w % f or h % f
    cam = scenes.camera(oracle, w, h)
    low = np_upsample.low_camera(cam, f)
    assert (low.img_width_pix, low.img_height_pix) == (-(-w // f), -(-h // f)) != (w // f, h // f)
    assert list(low.img_center_point) != list(cam.img_center_point) and low.mm_per_pix_hor == f32(f) * f32(cam.mm_per_pix_hor)
    assert list(low.position) == list(cam.position) and list(low.right) == list(cam.right) and list(low.up) == list(cam.up)
