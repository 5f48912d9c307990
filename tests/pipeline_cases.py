"""The frozen rows of the frame pipeline's tests (tests/test_np_pipeline.py on the CPU, tests/test_pipeline_gpu.py on the GPU):
sizes that are no multiple of the factor, odd sample counts (wa != 0.5), a thin lens that has to move with its camera, and every
combination of spike removal, upsampling and accumulation in front of each of the three ends and of the display stages.

Two scenes: the example spheres with the tiny bright emitter of test_despike_gpu.py, so that spikes and bright-pass pixels
exist, and full_scenes.all_features_scene for the row `mesh`. The camera drifts in x by `step` a frame."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import full_scenes
import np_lens
import np_pipeline as P
import np_tonemap
import np_upsample
import scenes
from rbrt_amd import abi

f32 = np.float32
FEATURE_SAMPLES = 3
LIGHT = ((2.0, 6.0, -8.0), 0.08, abi.material(abi.MAT_EMISSIVE, (3000.0, 2700.0, 2100.0)))
APERTURE_MM, FOCUS_DISTANCE = 20.0, 9.0  # the thin lens of the rows that have one (--aperture, --focus-distance)
REINHARD_AUTO = dict(curve=np_tonemap.REINHARD, exposure=0.0, white=0.0)


def _row(w, h, f, despike, frames, lens, n, end, seed, step, scene="spheres", **kw):
    d = None if despike is None else dict(radius=despike[0], rank=despike[1], threshold=despike[2])
    return SimpleNamespace(w=w, h=h, f=f, despike=d, frames=frames, lens=lens, n=n, end=end, seed=seed, step=(step, 0.0, 0.0), scene=scene, cli_seed=kw.get("cli_seed", seed),
                           nlm=kw.get("nlm"), guided=kw.get("guided"), glare=kw.get("glare"), tonemap=kw.get("tonemap"))


#                       W   H   f  despike r/k/t  frames lens  n  end      seed step
ROWS = {
    "all-3": _row(50, 47, 3, (1, 3, 1.5), 3, True, 5, "guided", 3, 0.03, glare=dict(threshold=0.5, intensity=0.3, levels=3), tonemap=REINHARD_AUTO),
    "all-2": _row(45, 27, 2, (2, 2, 4.0), 2, False, 7, "nlm", 7, 0.05, cli_seed=1, nlm=dict(window_radius=3, patch_radius=2), glare=dict(threshold=0.5, intensity=0.3),
                  tonemap=dict(curve=np_tonemap.ACES, exposure=0.5, white=1.0)),
    "all-4": _row(37, 21, 4, (1, 1, 1.5), 1, True, 6, "mix", 10, 0.01, cli_seed=1, tonemap=dict(curve=np_tonemap.LINEAR, exposure=0.0, white=1.0)),
    "frames-nlm": _row(45, 27, 0, (2, 2, 4.0), 3, True, 5, "nlm", 11, 0.02),
    "up-guided-raw": _row(50, 47, 3, None, 1, True, 7, "guided", 13, 0.01, guided=dict(flags=1), glare=dict(threshold=0.5, intensity=0.3)),
    "up-frames": _row(37, 21, 2, None, 2, False, 6, "mix", 17, 0.04),
    "despike-odd": _row(64, 48, 0, (1, 3, 1.5), 1, True, 5, "mix", 19, 0.01),
    "tiny": _row(9, 7, 4, (2, 4, 1.0), 2, True, 5, "guided", 23, 0.01, cli_seed=7, glare=dict(threshold=0.5, intensity=0.3), tonemap=REINHARD_AUTO),
    "mesh": _row(40, 24, 2, (1, 3, 1.5), 2, True, 5, "guided", 58, 0.02, scene="mesh", tonemap=dict(curve=np_tonemap.ACES, exposure=1.0, white=1.0)),
}
CLI_ROWS = ("all-3", "all-2", "all-4", "despike-odd", "tiny")


def options(r):
    return P.options(upscale=r.f, despike=r.despike, frames=r.frames, end=r.end, nlm=r.nlm, guided=r.guided, glare=r.glare, tonemap=r.tonemap,
                     epsilon=0.5)


def scene_of(oracle, r):
    return full_scenes.all_features_scene(oracle) if r.scene == "mesh" else scenes.spheres_scene(scenes.EXAMPLE_SPHERES + [LIGHT])


def opts_of(r, spp, seed):
    """The spheres under the default sky (its luminance, 0.68 to 1, is above the rows' glare threshold); the scene with a mesh as
    full_scenes has it, under a black one."""
    if r.scene == "mesh":
        return full_scenes.all_features_opts(spp, seed)
    return abi.default_opts(spp=spp, seed=seed)


def lens_of(r, cam):
    """The lens of every frame's camera: it depends on the camera's right vector alone, which the drift leaves as it is."""
    if not r.lens:
        return None
    return np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], APERTURE_MM, FOCUS_DISTANCE)


def cameras(r, cam0, k):
    """(the full camera of frame k, the camera that is traced)."""
    full = P.frame_camera(cam0, r.step, k)
    return full, (np_upsample.low_camera(full, r.f) if r.f else full)


def check_conditions(name, r, res, frames, few_spikes=True):
    """The conditions a row has to meet for its comparison to mean something, from the numpy side alone. `few_spikes`: the flagged
    pixels stay below 5 % of the traced ones -- asked of every row whose traced image has 20 pixels or more (below that one
    flagged pixel is 5 % already: the row `tiny` traces 3 x 2)."""
    for k, (s, fr) in enumerate(zip(res.frames, frames)):
        for x in (fr.albedo, fr.normal, fr.depth, fr.coverage):
            flat = x.reshape(x.shape[0] * x.shape[1], -1)
            assert (flat != 0).any(axis=1).any() and (flat == 0).all(axis=1).any(), (name, k, "a feature buffer is covered or uncovered everywhere")
        if k:
            assert 0.0 < s.valid < 1.0, (name, k, s.valid)
    traced = res.render_width * res.render_height
    if r.despike is not None:
        assert any(s.spikes[0] > 0 for s in res.frames) and any(s.spikes[1] > 0 for s in res.frames), (name, [s.spikes for s in res.frames])
        assert not few_spikes or traced < 20 or all(int((s.mask != 0).sum()) < 0.05 * traced for s in res.frames), (name, [int((s.mask != 0).sum()) for s in res.frames], traced)
    assert res.frames[-1].length.max() == r.frames, (name, float(res.frames[-1].length.max()))
    if r.glare is not None:
        import np_glare
        assert np_glare.bright_mask(res.filtered, dict(P.GLARE_DEFAULTS, **r.glare)["threshold"]).any(), (name, "no bright-pass pixel")
    if r.tonemap is not None and r.tonemap["exposure"] == 0.0:
        assert res.exposure != 1 and res.chosen.counted > 0, (name, res.exposure)
