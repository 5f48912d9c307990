"""The frame pipeline restated in numpy: what a render with --despike, --upscale and --frames does between the traced samples
and the files, as ONE composition of the stages' own restatements (np_denoise, np_despike, np_upsample, np_temporal, np_guided,
np_glare, np_tonemap, np_compare). The order is the one of include/rbrt_hip.h and DESIGN.md "The frame pipeline together":

    per frame   halves -> despike (at the traced size) -> upsample -> [the unfiltered image] -> accumulate
    at the end  guided | non-local means | plain mix -> [the comparison reads this] -> glare -> display transform

The only arithmetic of its own, each float32 and step by step: the host's mix wa, the camera of frame k, the seed of frame k and
the two grey maps. Every intermediate is returned, so that a mismatch names its stage. `order` and `display_order` exist for
tests/test_np_pipeline.py alone: they show that a swapped order gives another image."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import np_adaptive
import np_compare
import np_denoise
import np_despike
import np_glare
import np_guided
import np_temporal
import np_tonemap
import np_upsample

f32 = np.float32
ORDER = ("despike", "upsample", "accumulate")
DISPLAY_ORDER = ("glare", "tonemap")
GLARE_DEFAULTS = dict(threshold=1.0, intensity=0.1, levels=5, spread=1.0)
TONEMAP_DEFAULTS = dict(curve=np_tonemap.LINEAR, exposure=1.0, key=0.18, white=0.0)


def options(upscale=0, upsample=None, despike=None, frames=0, temporal=None, end="mix", nlm=None, guided=None, glare=None, tonemap=None,
            epsilon=0.01):
    """upscale: 0 or the factor 2..4; despike: None or dict(radius, rank, threshold); frames: 0 (no accumulation) or the number of
    frames; end: "mix", "nlm" or "guided"; glare, tonemap: None or a dict of the stage's options; the other dicts override the
    stages' defaults."""
    assert end in ("mix", "nlm", "guided") and upscale in (0, 2, 3, 4)
    return SimpleNamespace(upscale=int(upscale), upsample=dict({k: v for k, v in np_upsample.DEFAULTS.items() if k != "factor"}, **(upsample or {})),
                           despike=None if despike is None else dict(np_despike.DEFAULTS, **despike), frames=int(frames),
                           temporal=dict(np_temporal.DEFAULTS, **(temporal or {})), end=end, nlm=dict(np_denoise.DEFAULTS, **(nlm or {})),
                           guided=dict(np_guided.DEFAULTS, **(guided or {})), glare=None if glare is None else dict(GLARE_DEFAULTS, **glare),
                           tonemap=None if tonemap is None else dict(TONEMAP_DEFAULTS, **tonemap), epsilon=float(epsilon))


# ---- the host's own arithmetic ---------------------------------------------------------------------------------------------------
def mix_weight(n):
    """wa of a one-round render of n samples: h = (n + 1) / 2 of them are in A."""
    return f32((int(n) + 1) // 2) * (f32(1) / f32(int(n)))


def frame_seed(seed, k):
    return int(seed) + int(k)


def frame_camera(cam, step, k):
    """The camera of frame k: position and img_center_point moved by float(k) * step."""
    out = type(cam).from_buffer_copy(cam)
    for c in range(3):
        shift = f32(k) * f32(step[c])
        out.position[c] = f32(cam.position[c]) + shift
        out.img_center_point[c] = f32(cam.img_center_point[c]) + shift
    return out


def spike_map(mask):
    """--spike-map: 0 none, 85 A, 170 B, 255 both."""
    return ((mask & np.uint8(3)) * np.uint8(85)).astype(np.uint8)


def history_map(length, max_history):
    """--history-map: length / max_history * 255, clamped to 0..255 and truncated; NaN is 0."""
    with np.errstate(all="ignore"):
        v = (length.astype(f32) / f32(max_history)) * f32(255)
        out = np.where(v >= f32(255), f32(255), v)
        out = np.where(np.isnan(v) | (v <= 0), f32(0), out)
    return out.astype(np.uint8)


# ---- the composition -----------------------------------------------------------------------------------------------------------------
def frame(samples, albedo, normal, depth, coverage, cam):
    """One frame's inputs: the per-sample radiance [n, h, w, 3] at the traced size, the feature buffers at the full size and the full
    camera."""
    return SimpleNamespace(samples=np.asarray(samples, f32), albedo=albedo, normal=normal, depth=depth, coverage=coverage, cam=cam)


def _display(x, o, display_order, exposure=None, white=None):
    """x through glare and the display transform: -> namespace(glared, out, rgb8, chosen); rgb8 None without either stage."""
    r = SimpleNamespace(glared=None, out=x, rgb8=None, chosen=None)
    for stage in display_order:
        if stage == "glare" and o.glare is not None:
            r.out, r.rgb8 = np_glare.glare(r.out, **o.glare)
            r.glared = r.out
        if stage == "tonemap" and o.tonemap is not None:
            t = dict(o.tonemap)
            curve = t.pop("curve")
            if exposure is not None:
                t["exposure"], t["white"] = exposure, white
            shape = r.out.shape
            out, rgb8, r.chosen = np_tonemap.tonemap(r.out.reshape(-1, 3), curve, **t)
            r.out, r.rgb8 = out.reshape(shape), rgb8.reshape(shape)
    return r


def pipeline(frames, o, reference=None, order=ORDER, display_order=DISPLAY_ORDER, wa_value=None):
    """frames: a list of frame(...), the last one is the image; o: options(...); reference: float32 [H, W, 3] or None.
    wa_value: another mix than the host's (test_np_pipeline.py). -> a namespace of every intermediate and every output."""
    assert sorted(order) == sorted(ORDER) and sorted(display_order) == sorted(DISPLAY_ORDER)
    assert len(frames) == max(o.frames, 1)
    H, W = frames[-1].depth.shape
    f = o.upscale if o.upscale else 1
    w, h = np_upsample.low_size(W, H, f)
    n = frames[0].samples.shape[0]
    wa_host = mix_weight(n) if wa_value is None else f32(wa_value)
    wa_full = np.full((H, W), wa_host, f32)
    out = SimpleNamespace(frames=[], wa=wa_host, width=W, height=H, render_width=w, render_height=h)
    hist = {"low": None, "full": None}
    prev = None
    for k, fr in enumerate(frames):
        assert fr.samples.shape == (n, h, w, 3) and fr.depth.shape == (H, W)
        counts = np.full(np_adaptive.tile_grid(h, w), n, np.uint32)  # one round that stops nothing
        a, b, wa = np_denoise.halves(*np_denoise.halves_from_samples(fr.samples, counts), counts)
        assert (wa == wa_host).all() or wa_value is not None
        own = np_adaptive.adaptive(fr.samples, 0.0, max(n, 2), max(n, 2))  # the render's own image
        s = SimpleNamespace(raw_a=a, raw_b=b, own=own.image, own8=own.rgb8, mask=None, spikes=None, valid=None, noisy=None, noisy8=None)
        feats = (fr.albedo, fr.normal, fr.depth, fr.coverage)
        low_cam = np_upsample.low_camera(fr.cam, f) if f > 1 else fr.cam
        for stage in order:
            if stage == "despike" and o.despike is not None:
                a, b, s.mask, s.spikes, _ = np_despike.despike(a, b, **o.despike)
                s.spike_a, s.spike_b = a, b
            if stage == "upsample" and f > 1:
                a, b, _, _ = np_upsample.upsample(a, b, None, *feats, factor=f, **o.upsample)
                s.up_a, s.up_b = a, b
                s.noisy = np_denoise.mix(a, b, wa_full)  # the unfiltered image of an upsampled render: in front of the accumulation
                s.noisy8 = np_adaptive.quantise(s.noisy)
            if stage == "accumulate" and o.frames:
                if a.shape[0] == H and a.shape[1] == W:
                    key, cam, (N, z, c) = "full", fr.cam, feats[1:]
                else:  # (only a swapped order accumulates at the low size: the features of the low pixels' blocks, the low camera)
                    L = np_upsample.reduce(a, b, None, *feats, f, np_upsample.NO_DEMODULATION)
                    key, cam, (N, z, c) = "low", low_cam, (L.n, L.z, L.c)
                a, b, s.length, hist[key], info = np_temporal.accumulate(a, b, N, z, c, cam, prev and prev[key], hist[key], **o.temporal)
                s.acc_a, s.acc_b, s.history = a, b, np_temporal.pack(hist[key])
                s.valid = None if info is None else float(info.valid.mean())
        if s.noisy is None:  # without upsampling: the render's own image, in front of spike removal
            s.noisy, s.noisy8 = s.own, s.own8
        s.a, s.b = a, b
        prev = {"full": fr.cam, "low": low_cam}
        out.frames.append(s)
    last, fr = out.frames[-1], frames[-1]
    assert last.a.shape == (H, W, 3)
    out.spike_map = None if last.mask is None else spike_map(last.mask)
    out.spikes_a = None if last.mask is None else float(np.mean([float(s.spikes[0]) for s in out.frames]))
    out.spikes_b = None if last.mask is None else float(np.mean([float(s.spikes[1]) for s in out.frames]))
    out.history_map = history_map(last.length, o.temporal["max_history"]) if o.frames else None
    if o.end == "guided":
        out.filtered, out.filtered8 = np_guided.denoise(last.a, last.b, wa_full, fr.albedo, fr.normal, fr.depth, fr.coverage, **o.guided)
    elif o.end == "nlm":
        out.filtered, out.filtered8 = np_denoise.denoise(last.a, last.b, wa_full, **o.nlm)
    else:
        out.filtered = np_denoise.mix(last.a, last.b, wa_full)
        out.filtered8 = np_adaptive.quantise(out.filtered)
    out.noisy, out.noisy8 = last.noisy, last.noisy8
    shown = _display(out.filtered, o, display_order)
    out.glared, out.chosen = shown.glared, shown.chosen
    out.exposure = None if shown.chosen is None else shown.chosen.exposure
    out.white = None if shown.chosen is None else shown.chosen.white
    out.final8 = shown.rgb8 if shown.rgb8 is not None else out.filtered8
    # the unfiltered image: the same glare, and the target's chosen exposure and white as manual values
    noisy_shown = _display(out.noisy, o, display_order, out.exposure, out.white)
    out.noisy_final8 = noisy_shown.rgb8 if noisy_shown.rgb8 is not None else out.noisy8
    out.compare = out.summary = None
    if reference is not None:  # the comparison reads the linear radiance in front of glare
        out.compare = np_compare.compare(out.filtered, np.ascontiguousarray(reference, f32), o.epsilon)
        out.summary = np_compare.summary(out.compare, W, H)
    return out
