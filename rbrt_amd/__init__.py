"""rbrt_amd — MI355X (gfx950) implementation of baurst/rbrt's path-tracing hot path.

The product is the C ABI in include/rbrt_hip.h (rbrt_amd/lib/librbrt_hip.so: hand-written HIP
kernels + host BVH builder) and the C++ host in rbrt_amd/host (CLI, YAML, .obj, PNG). This Python
package is a thin ctypes binding over those for tests and bench.py.

    render_scene(cam, num_samples, scene)  <->  rbrt_lib::render_scene (lib.rs:75-79)
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import (Camera, CameraLens, Material, RenderOpts, RbrtError, SceneData, MeshData, default_opts, load_hip,  # noqa: F401
                  material, MAT_DIELECTRIC, MAT_LAMBERTIAN, MAT_METAL)

__all__ = ["render_scene", "HipScene", "abi", "device_count"]


def device_count() -> int:
    return int(load_hip().rbrt_hip_device_count())


def _cam_arg(cam: abi.Camera, lens, opts: abi.RenderOpts):
    """(camera pointer, object to keep alive) for a render call. `lens`: None (pinhole), an abi.CameraLens or a tuple
    (lens_u, lens_v, focus_scale); with a lens the call gets `cam` inside an rbrt_camera_lens_t and RBRT_FLAG_THIN_LENS."""
    if lens is None:
        return C.byref(cam), cam
    if isinstance(lens, abi.CameraLens):
        lens = (tuple(lens.lens_u), tuple(lens.lens_v), lens.focus_scale)
    L = abi.camera_lens(cam, *lens)
    opts.flags |= abi.FLAG_THIN_LENS
    return C.byref(L.cam), L


def render_scene(cam: abi.Camera, num_samples: int, scene: abi.SceneData, seed: int = 1, want_radiance: bool = True,
                 lens=None, **opt_overrides):
    """One-shot render through rbrt_hip_render (host buffers in and out).

    Same contract as the reference's render_scene (lib.rs:75-79) plus the pre-gamma radiance:
    returns (radiance float32[H,W,3], rgb8 uint8[H,W,3]); want_radiance=False: (None, rgb8), exactly what the
    reference returns. `lens`: a thin lens (see _cam_arg), None for the reference's pinhole camera. A scene with smooth
    meshes (MeshData normals=, YAML `shading: smooth`) goes through rbrt_hip_render_shaded, every other one through
    rbrt_hip_render.
    """
    lib = load_hip()
    opts = default_opts(spp=num_samples, seed=seed, **opt_overrides)
    cam_p, _keep = _cam_arg(cam, lens, opts)
    H, W = cam.img_height_pix, cam.img_width_pix
    rad = np.zeros((H, W, 3), np.float32) if want_radiance else None
    rgb = np.empty((H, W, 3), np.uint8) if not want_radiance else np.zeros((H, W, 3), np.uint8)
    out = (rad.ctypes.data_as(abi.f32p) if want_radiance else None, rgb.ctypes.data_as(abi.u8p))
    shading, patterns = _shading_ptr(scene), _patterns_ptr(scene)
    if patterns is not None:
        rc = lib.rbrt_hip_render_patterned(cam_p, scene.ptr(), shading, patterns, C.byref(opts), *out)
    elif shading is None:
        rc = lib.rbrt_hip_render(cam_p, scene.ptr(), C.byref(opts), *out)
    else:
        rc = lib.rbrt_hip_render_shaded(cam_p, scene.ptr(), shading, C.byref(opts), *out)
    abi.check(rc)
    return rad, rgb


def _shading_ptr(scene):
    """The scene's rbrt_scene_shading_t*, None when no mesh carries corner normals."""
    f = getattr(scene, "shading_ptr", None)
    return f() if f is not None else None


def _patterns_ptr(scene):
    """The scene's rbrt_scene_patterns_t*, None when no object carries a solid pattern."""
    f = getattr(scene, "patterns_ptr", None)
    return f() if f is not None else None


def last_render_times() -> dict:
    """Where the time of this thread's last one-shot render_scene (rbrt_hip_render) went (rbrt_hip_last_render_times)."""
    t = abi.CallTimes()
    abi.check(load_hip().rbrt_hip_last_render_times(C.byref(t)))
    return t.as_dict()


class HipScene:
    """Device-resident scene (rbrt_hip_scene_create): upload + BVH build once, render many times."""

    def __init__(self, scene: abi.SceneData, device: int = 0):
        self._lib = load_hip()
        self._h = C.c_void_p()
        self.device = device
        self.scene = scene  # keep host arrays alive
        shading, patterns = _shading_ptr(scene), _patterns_ptr(scene)
        if patterns is not None:
            abi.check(self._lib.rbrt_hip_scene_create_patterned(scene.ptr(), shading, patterns, device, C.byref(self._h)))
        elif shading is None:
            abi.check(self._lib.rbrt_hip_scene_create(scene.ptr(), device, C.byref(self._h)))
        else:
            abi.check(self._lib.rbrt_hip_scene_create_shaded(scene.ptr(), shading, device, C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.rbrt_hip_scene_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def render_device(self, cam: abi.Camera, opts: abi.RenderOpts, d_radiance: int | None, d_rgb8: int | None = None,
                      stream: int | None = None, lens=None):
        """Asynchronous render into device pointers (ints, e.g. torch.Tensor.data_ptr()). `lens`: see _cam_arg (opts is
        not changed: the flag goes on a copy)."""
        opts = _opts_copy(opts)
        cam_p, _keep = _cam_arg(cam, lens, opts)
        abi.check(self._lib.rbrt_hip_render_device(self._h, cam_p, C.byref(opts), C.c_void_p(stream or 0),
                                                   C.c_void_p(d_radiance or 0), C.c_void_p(d_rgb8 or 0)))

    def render_pass(self, cam: abi.Camera, opts: abi.RenderOpts, sample_begin: int, sample_end: int, d_accum: int,
                    d_radiance: int | None = None, d_rgb8: int | None = None, stream: int | None = None, lens=None):
        """Samples [sample_begin, sample_end) of opts.spp, accumulated into d_accum (rbrt_hip_render_pass)."""
        opts = _opts_copy(opts)
        cam_p, _keep = _cam_arg(cam, lens, opts)
        abi.check(self._lib.rbrt_hip_render_pass(self._h, cam_p, C.byref(opts), C.c_void_p(stream or 0), sample_begin,
                                                 sample_end, C.c_void_p(d_accum), C.c_void_p(d_radiance or 0),
                                                 C.c_void_p(d_rgb8 or 0)))

    def render_adaptive(self, cam: abi.Camera, opts: abi.RenderOpts, threshold: float, min_samples: int = 16, step: int = 64,
                        d_radiance: int | None = None, d_rgb8: int | None = None, d_tile_samples: int | None = None,
                        d_tile_error: int | None = None, stream: int | None = None, lens=None, reserved: int = 0) -> dict:
        """Adaptive render into device pointers (rbrt_hip_render_adaptive): opts.spp is the upper limit, a tile stops once its
        error estimate is below `threshold`. Blocking: the outputs are complete on return. d_tile_samples (uint32) and
        d_tile_error (float32) take one entry per tile of the rank, in ascending tile number. Returns the call's totals:
        rounds, samples, samples_fixed."""
        opts = _opts_copy(opts)
        cam_p, _keep = _cam_arg(cam, lens, opts)
        a = abi.AdaptiveOpts(float(threshold), int(min_samples), int(step), int(reserved))
        res = abi.AdaptiveResult()
        abi.check(self._lib.rbrt_hip_render_adaptive(self._h, cam_p, C.byref(opts), C.byref(a), C.c_void_p(stream or 0),
                                                     C.c_void_p(d_radiance or 0), C.c_void_p(d_rgb8 or 0),
                                                     C.c_void_p(d_tile_samples or 0), C.c_void_p(d_tile_error or 0), C.byref(res)))
        return dict(rounds=int(res.rounds), samples=int(res.samples), samples_fixed=int(res.samples_fixed))

    def adaptive_rounds(self) -> list:
        """Tiles active at the start of each round of the last render_adaptive call (rbrt_hip_scene_adaptive_rounds)."""
        n = C.c_uint32()
        abi.check(self._lib.rbrt_hip_scene_adaptive_rounds(self._h, None, 0, C.byref(n)))
        buf = (C.c_uint32 * max(n.value, 1))()
        abi.check(self._lib.rbrt_hip_scene_adaptive_rounds(self._h, buf, n.value, C.byref(n)))
        return [int(buf[i]) for i in range(n.value)]

    def denoise(self, d_radiance: int | None = None, d_rgb8: int | None = None, d_half_a: int | None = None,
                d_half_b: int | None = None, window_radius: int | None = None, patch_radius: int | None = None,
                strength: float | None = None, stream: int | None = None, reserved: int = 0):
        """The denoised image of the last render_adaptive call into device pointers (rbrt_hip_scene_denoise): row-major
        float32 / uint8 [H, W, 3]; d_half_a, d_half_b take the two half images the filter worked on. Asynchronous on `stream`.
        A parameter left None takes the library's default (rbrt_denoise_opts_default: 5, 3, 0.7)."""
        d = denoise_opts(window_radius, patch_radius, strength, reserved)
        abi.check(self._lib.rbrt_hip_scene_denoise(self._h, C.byref(d), C.c_void_p(stream or 0), C.c_void_p(d_radiance or 0),
                                                   C.c_void_p(d_rgb8 or 0), C.c_void_p(d_half_a or 0), C.c_void_p(d_half_b or 0)))

    def denoise_guided(self, d_albedo: int, d_normal: int, d_depth: int, d_coverage: int, d_workspace: int,
                       d_radiance: int | None = None, d_rgb8: int | None = None, opts: abi.GuidedOpts | None = None,
                       stream: int | None = None):
        """The guided filter on the last render_adaptive call's image (rbrt_hip_scene_denoise_guided): the feature buffers are
        render_features' of the same camera, d_workspace guided_workspace_bytes(W, H) bytes of device memory. `opts`:
        guided_opts(...), None for the library's defaults. Asynchronous on `stream`."""
        g = opts if opts is not None else guided_opts()
        abi.check(self._lib.rbrt_hip_scene_denoise_guided(self._h, C.byref(g), C.c_void_p(stream or 0), C.c_void_p(d_albedo or 0),
                                                          C.c_void_p(d_normal or 0), C.c_void_p(d_depth or 0), C.c_void_p(d_coverage or 0),
                                                          C.c_void_p(d_workspace or 0), C.c_void_p(d_radiance or 0), C.c_void_p(d_rgb8 or 0)))

    def render_features(self, cam: abi.Camera, opts: abi.RenderOpts, samples: int | None = None, d_albedo: int | None = None,
                        d_normal: int | None = None, d_depth: int | None = None, d_coverage: int | None = None,
                        d_object: int | None = None, lens=None, stream: int | None = None, reserved=(0, 0, 0),
                        d_motion: int | None = None):
        """The feature buffers of the primary rays into device pointers (rbrt_hip_render_features): the means over `samples`
        samples a pixel (None: the library's default, 4) of the albedo and the normal, float32 [H, W, 3], of the depth and
        the coverage, float32 [H, W], and the object id of sample 0, int32 [H, W]; each may be None. Asynchronous on `stream`.
        `lens`: see _cam_arg (opts is not changed). `d_motion` (not None: rbrt_hip_render_features_motion; 0 is its NULL): the
        mean travel of what the samples hit, float32 [H, W, 3]."""
        opts = _opts_copy(opts)
        cam_p, _keep = _cam_arg(cam, lens, opts)
        f = feature_opts(samples, reserved)
        if d_motion is not None:
            abi.check(self._lib.rbrt_hip_render_features_motion(self._h, cam_p, C.byref(opts), C.byref(f), C.c_void_p(stream or 0),
                                                                C.c_void_p(d_albedo or 0), C.c_void_p(d_normal or 0), C.c_void_p(d_depth or 0),
                                                                C.c_void_p(d_coverage or 0), C.c_void_p(d_object or 0), C.c_void_p(d_motion or 0)))
            return
        abi.check(self._lib.rbrt_hip_render_features(self._h, cam_p, C.byref(opts), C.byref(f), C.c_void_p(stream or 0),
                                                     C.c_void_p(d_albedo or 0), C.c_void_p(d_normal or 0), C.c_void_p(d_depth or 0),
                                                     C.c_void_p(d_coverage or 0), C.c_void_p(d_object or 0)))

    def set_environment(self, nodes, *, n: int | None = None, reserved: int = 0):
        """Sets the handle's environment map (rbrt_hip_scene_set_environment): `nodes` float32 (N + 1, N + 1, 3), N taken
        from its shape; None clears it (rays that hit nothing see opts.bg again). Blocking. `n` and `reserved` put other
        values into the struct (tests of the refusals; with `n` given, nodes = None is a NULL pointer in a struct)."""
        if nodes is None and n is None:
            abi.check(self._lib.rbrt_hip_scene_set_environment(self._h, None))
            return
        env = abi.Environment()
        if nodes is not None:
            nodes = np.ascontiguousarray(nodes, np.float32)
            if n is None:
                if nodes.ndim != 3 or nodes.shape[0] != nodes.shape[1] or nodes.shape[2] != 3 or nodes.shape[0] < 2:
                    raise ValueError("set_environment: nodes must have shape (N + 1, N + 1, 3)")
                n = nodes.shape[0] - 1
            env.nodes = abi.fptr(nodes)
        env.n, env.reserved = int(n), int(reserved)
        abi.check(self._lib.rbrt_hip_scene_set_environment(self._h, C.byref(env)))

    def set_shutter(self, travel, *, reserved: int = 0):
        """Sets the handle's shutter (rbrt_hip_scene_set_shutter): `travel` = (dx, dy, dz), the camera's translation during
        the exposure in scene units; None clears it (no shutter: no draw is made for it). `reserved` puts another value into
        the struct (tests of the refusals)."""
        if travel is None:
            abi.check(self._lib.rbrt_hip_scene_set_shutter(self._h, None))
            return
        sh = abi.Shutter()
        sh.travel[:] = [float(np.float32(v)) for v in travel]
        sh.reserved = int(reserved)
        abi.check(self._lib.rbrt_hip_scene_set_shutter(self._h, C.byref(sh)))

    def set_motion(self, travels, *, n_spheres: int | None = None, reserved: int = 0, null_travel: bool = False):
        """Sets the handle's motion (rbrt_hip_scene_set_motion): `travels` = (n_spheres, 3), every sphere's translation during
        the exposure in scene units, in the order of the scene's spheres; None clears it. `n_spheres`, `reserved` and
        `null_travel` put other values into the struct (tests of the refusals)."""
        if travels is None:
            abi.check(self._lib.rbrt_hip_scene_set_motion(self._h, None))
            return
        tv = np.ascontiguousarray(np.asarray(travels, np.float32).reshape(-1, 3))
        mo = abi.Motion()
        mo.n_spheres = int(len(tv) if n_spheres is None else n_spheres)
        mo.reserved = int(reserved)
        mo.travel = None if null_travel else tv.ctypes.data_as(abi.f32p)
        abi.check(self._lib.rbrt_hip_scene_set_motion(self._h, C.byref(mo)))

    def set_mesh_motion(self, travels, *, n_meshes: int | None = None, reserved: int = 0, null_travel: bool = False):
        """Sets the handle's mesh motion (rbrt_hip_scene_set_mesh_motion): `travels` = (n_meshes, 3), every mesh's translation
        during the exposure in scene units, in the order of the scene's meshes; None clears it. `n_meshes`, `reserved` and
        `null_travel` put other values into the struct (tests of the refusals)."""
        if travels is None:
            abi.check(self._lib.rbrt_hip_scene_set_mesh_motion(self._h, None))
            return
        tv = np.ascontiguousarray(np.asarray(travels, np.float32).reshape(-1, 3))
        mo = abi.MeshMotion()
        mo.n_meshes = int(len(tv) if n_meshes is None else n_meshes)
        mo.reserved = int(reserved)
        mo.travel = None if null_travel else tv.ctypes.data_as(abi.f32p)
        abi.check(self._lib.rbrt_hip_scene_set_mesh_motion(self._h, C.byref(mo)))

    def set_motion_phase(self, phase: float):
        """Sets the phase of the handle's motion (rbrt_hip_scene_set_motion_phase): a sample with the draw t sees sphere i at
        center_i + (phase + t) * travel_i. 0 by default; it goes with the launches issued after the call."""
        abi.check(self._lib.rbrt_hip_scene_set_motion_phase(self._h, C.c_float(phase)))

    def environment_lookup(self, dirs):
        """The environment's radiance for each direction, used as it is (rbrt_hip_debug_environment; test hook): float32
        (n, 3)."""
        dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
        out = np.zeros((dirs.shape[0], 3), np.float32)
        abi.check(self._lib.rbrt_hip_debug_environment(self._h, abi.fptr(dirs), dirs.shape[0], abi.fptr(out)))
        return out

    def set_pipeline(self, depth: int):
        """Overlap consecutive trace launches over `depth` internal streams (rbrt_hip_scene_set_pipeline)."""
        abi.check(self._lib.rbrt_hip_scene_set_pipeline(self._h, int(depth)))

    def set_short_paths(self, mode: int = 1):
        """The short-path stage in front of the trace launches (rbrt_hip_scene_set_short_paths): 0 never, 1 automatic (the
        launches that run beside others), 2 every launch; same image."""
        abi.check(self._lib.rbrt_hip_scene_set_short_paths(self._h, int(mode)))

    def short_masks(self):
        """The finished masks of the last trace launch that had the short-path stage (rbrt_hip_debug_short_masks; test
        hook): uint64 (n_chunks,), chunk = work-list position * samples of the launch + sample; empty if there was none."""
        n = C.c_size_t()
        abi.check(self._lib.rbrt_hip_debug_short_masks(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, np.uint64)
        if n.value:
            abi.check(self._lib.rbrt_hip_debug_short_masks(self._h, out.ctypes.data_as(C.POINTER(C.c_uint64)), n.value, C.byref(n)))
        return out

    def set_timing(self, on: bool = True):
        abi.check(self._lib.rbrt_hip_scene_set_timing(self._h, int(on)))

    def kernel_ms(self):
        """(total trace-kernel ms, total resolve-kernel ms, number of trace launches) since set_timing(True)."""
        t, r, n = C.c_float(), C.c_float(), C.c_uint32()
        abi.check(self._lib.rbrt_hip_scene_kernel_ms(self._h, C.byref(t), C.byref(r), C.byref(n)))
        return t.value, r.value, n.value

    def launch_mix(self):
        """(full-grid, half-grid) trace launches since set_timing(True) (rbrt_hip_scene_launch_mix)."""
        a, b = C.c_uint32(), C.c_uint32()
        abi.check(self._lib.rbrt_hip_scene_launch_mix(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def helper_launches(self) -> int:
        """Helper launches since set_timing(True) (rbrt_hip_scene_helper_launches)."""
        n = C.c_uint32()
        abi.check(self._lib.rbrt_hip_scene_helper_launches(self._h, C.byref(n)))
        return n.value

    def last_trace_build(self) -> str:
        """The build of the trace kernel the last trace launch ran: "none", "general" or "plain"
        (rbrt_hip_scene_last_trace_build)."""
        b = C.c_int()
        abi.check(self._lib.rbrt_hip_scene_last_trace_build(self._h, C.byref(b)))
        return ("none", "general", "plain")[b.value]

    def create_times(self) -> dict:
        """Where the time of rbrt_hip_scene_create went (rbrt_hip_scene_create_times)."""
        t = abi.CallTimes()
        abi.check(self._lib.rbrt_hip_scene_create_times(self._h, C.byref(t)))
        return t.as_dict()

    def refine_wait(self, timeout_s: float = 60.0):
        """Waits for the background build of the host builder's trees and adopts them (rbrt_hip_scene_refine_wait).
        Returns (state, seconds): 0 none was started, 1 in use now, 2 failed / cancelled, 3 still at work."""
        st, sec = C.c_int(), C.c_double()
        abi.check(self._lib.rbrt_hip_scene_refine_wait(self._h, float(timeout_s), C.byref(st), C.byref(sec)))
        return st.value, sec.value

    def info(self) -> dict:
        i = abi.SceneInfo()
        abi.check(self._lib.rbrt_hip_scene_info(self._h, C.byref(i)))
        return {k: int(getattr(i, k)) for k, _ in abi.SceneInfo._fields_}

    def check(self):
        """Synchronise and raise RbrtError if a kernel flagged a NaN sphere discriminant (sphere.rs:33) or corrupt
        path state since the last check (rbrt_hip_scene_check)."""
        abi.check(self._lib.rbrt_hip_scene_check(self._h))

    def last_batches(self):
        """(samples per batch, number of batches) of the last render_device call."""
        b, n = C.c_uint32(), C.c_uint32()
        abi.check(self._lib.rbrt_hip_scene_last_batching(self._h, C.byref(b), C.byref(n)))
        return b.value, n.value

    def stats(self) -> dict:
        st = abi.Stats()
        abi.check(self._lib.rbrt_hip_scene_stats(self._h, C.byref(st)))
        return {k: int(getattr(st, k)) for k, _ in abi.Stats._fields_}

    def set_debug_counter(self, index: int, value: int):
        abi.check(self._lib.rbrt_hip_scene_debug_set_counter(self._h, int(index), int(value)))

    def raw_debug_counters(self) -> list:
        buf = (C.c_uint64 * 64)()
        abi.check(self._lib.rbrt_hip_scene_debug_counters(self._h, buf, 64))
        return [int(x) for x in buf]

    def debug_counters(self) -> dict:
        """Pass statistics of the megakernel from the last counting render (diagnostic)."""
        buf = (C.c_uint64 * 64)()
        abi.check(self._lib.rbrt_hip_scene_debug_counters(self._h, buf, 64))
        names = ("empty", "trav", "term", "lamb", "metal", "diel")
        d = {f"passes_{n}": int(buf[i]) for i, n in enumerate(names)}
        d.update({f"slots_{n}": int(buf[6 + i]) for i, n in enumerate(names)})
        d.update(trav_wave_steps=int(buf[12]), trav_lane_steps=int(buf[13]), refill_rounds=int(buf[14]),
                 sched_rounds=int(buf[15]), cycles_trav=int(buf[16]), cycles_shade=int(buf[17]),
                 cycles_total=int(buf[18]), leaf_rounds=int(buf[19]), leaf_lanes=int(buf[20]),
                 walk_rounds=int(buf[21]), walk_lanes=int(buf[22]), shading_pass_free_lanes=int(buf[23]),
                 rt_first_start=int(buf[24]), rt_last_workout=int(buf[25]), rt_last_end=int(buf[26]),
                 rt_sum_wave_time=int(buf[27]), rt_first_workout=int(buf[28]),
                 path_len_hist=[int(buf[32 + i]) for i in range(8)],     # bounces 0, 1, 2-3, 4-7, ... 64+
                 long_path_objects=[int(buf[40 + i]) for i in range(8)], # bounces of paths >= 16, per object id
                 long_path_total=int(buf[48]), long_path_dielectric=int(buf[47]), shade_extra_rounds=int(buf[29]),
                 drain_slowest=dict(us=int(buf[50]) >> 44, rounds=(int(buf[50]) >> 32) & 0xFFF,
                                    trav_steps=(int(buf[50]) >> 16) & 0xFFFF, passes=int(buf[50]) & 0xFFFF),
                 drain_sum=dict(rounds=int(buf[51]), trav_steps=int(buf[52]), passes=int(buf[53]),
                                lane_steps=int(buf[54])),
                 stack_pushes_beyond_lds=int(buf[30]), stack_deepest=int(buf[31]),
                 parked_at_burst_entry=int(buf[55]), fullest_shading_kind_at_burst_entry=int(buf[56]),
                 shared_entries_given=int(buf[59]), share_rounds=int(buf[60]), traversals_ending_at_root=int(buf[61]),
                 sphere_tail_runs=int(buf[62]), sphere_tail_lanes=int(buf[63]),
                 # what a pass of mixed kinds would pick up: passes (and lanes) where the fullest OTHER scatter kind has >= 8 / >= 16 waiting
                 mixed_pass_8=dict(passes=int(buf[49]) >> 32, lanes=int(buf[49]) & 0xFFFFFFFF),
                 mixed_pass_16=dict(passes=int(buf[58]) >> 32, lanes=int(buf[58]) & 0xFFFFFFFF))
        return d

    def primary_cull(self, cam, opts=None, lens=None):
        """The primary-ray culling table for `cam` (test hook): uint32 (tiles_y, tiles_x). Without `opts` the table of a render
        with the default options (rbrt_hip_debug_primary_cull); with an abi.RenderOpts the table of a render with those --
        its min_dist is part of the pad of the tree boxes the pass tests -- and, with `lens` (see _cam_arg), of its lens rays
        (rbrt_hip_debug_primary_cull_opts)."""
        tx, ty = (cam.img_width_pix + 7) // 8, (cam.img_height_pix + 7) // 8
        out = np.zeros(tx * ty, np.uint32)
        words = out.ctypes.data_as(C.POINTER(C.c_uint32))
        if opts is None and lens is None:
            abi.check(self._lib.rbrt_hip_debug_primary_cull(self._h, C.byref(cam), words, out.size))
        else:
            opts = _opts_copy(opts if opts is not None else abi.default_opts())
            cam_p, _keep = _cam_arg(cam, lens, opts)
            abi.check(self._lib.rbrt_hip_debug_primary_cull_opts(self._h, cam_p, C.byref(opts), words, out.size))
        return out.reshape(ty, tx)

    def primary_cull_lens(self, cam, lens):
        """The same table for the lens rays of `cam` with `lens` (rbrt_hip_debug_primary_cull_lens; test hook)."""
        if not isinstance(lens, abi.CameraLens):
            lens = abi.camera_lens(cam, *lens)
        else:
            lens = abi.camera_lens(cam, tuple(lens.lens_u), tuple(lens.lens_v), lens.focus_scale)
        tx, ty = (cam.img_width_pix + 7) // 8, (cam.img_height_pix + 7) // 8
        out = np.zeros(tx * ty, np.uint32)
        abi.check(self._lib.rbrt_hip_debug_primary_cull_lens(self._h, C.byref(lens), out.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                             out.size))
        return out.reshape(ty, tx)

    def primary_cull_shutter(self, cam, lens, travel):
        """The same table for the camera rays of `cam` -- with `lens` (None: a pinhole) -- on a handle whose shutter is
        `travel` (rbrt_hip_debug_primary_cull_shutter; test hook). The handle's own shutter is neither read nor changed."""
        if lens is not None:
            if not isinstance(lens, abi.CameraLens):
                lens = abi.camera_lens(cam, *lens)
            else:
                lens = abi.camera_lens(cam, tuple(lens.lens_u), tuple(lens.lens_v), lens.focus_scale)
        tv = (C.c_float * 3)(*[float(np.float32(v)) for v in travel])
        tx, ty = (cam.img_width_pix + 7) // 8, (cam.img_height_pix + 7) // 8
        out = np.zeros(tx * ty, np.uint32)
        abi.check(self._lib.rbrt_hip_debug_primary_cull_shutter(self._h, C.byref(cam), C.byref(lens) if lens is not None else None, tv,
                                                                out.ctypes.data_as(C.POINTER(C.c_uint32)), out.size))
        return out.reshape(ty, tx)

    def surface_albedo(self, rays, min_dist=0.001, max_dist=2000.0):
        """The attenuation scatter would record at each ray's closest hit, NaN for a miss (rbrt_hip_debug_surface_albedo;
        test hook): float32 (n, 3)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 3), np.float32)
        abi.check(self._lib.rbrt_hip_debug_surface_albedo(self._h, rays.ctypes.data_as(abi.f32p), rays.shape[0], min_dist,
                                                          max_dist, out.ctypes.data_as(abi.f32p)))
        return out

    def shading_normals(self, rays, min_dist=0.001, max_dist=2000.0):
        """The normal the scatter pass would use at each ray's closest hit, NaN for a miss (rbrt_hip_debug_shading_normals;
        test hook): float32 (n, 3)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        out = np.zeros((rays.shape[0], 3), np.float32)
        abi.check(self._lib.rbrt_hip_debug_shading_normals(self._h, rays.ctypes.data_as(abi.f32p), rays.shape[0], min_dist,
                                                           max_dist, out.ctypes.data_as(abi.f32p)))
        return out

    def trace_rays(self, rays, min_dist=0.001, max_dist=2000.0):
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 6)
        n = rays.shape[0]
        t = np.zeros(n, np.float32)
        dist = np.zeros(n, np.float32)
        obj = np.zeros(n, np.int32)
        tri = np.zeros(n, np.int32)
        abi.check(self._lib.rbrt_hip_trace_rays(self._h, rays.ctypes.data_as(abi.f32p), n, min_dist, max_dist,
                                                t.ctypes.data_as(abi.f32p), obj.ctypes.data_as(abi.i32p),
                                                tri.ctypes.data_as(abi.i32p), dist.ctypes.data_as(abi.f32p)))
        return t, obj, tri, dist


def _opts_copy(opts: abi.RenderOpts) -> abi.RenderOpts:
    o = abi.RenderOpts()
    C.memmove(C.byref(o), C.byref(opts), C.sizeof(o))
    return o


def supported_flags() -> int:
    """The RBRT_FLAG_* bits the library honours (rbrt_hip_supported_flags)."""
    return int(load_hip().rbrt_hip_supported_flags())


def debug_scatter(kind, albedo, param, in_dir, point, normal, rng_state):
    """n scatter events through the device functions the shading passes use (rbrt_hip_debug_scatter; test hook).
    Arrays of length n: kind int32, albedo (n,3), param, in_dir (n,3), point (n,3), normal (n,3), rng_state (n,2) uint32.
    Returns (out_dir (n,3) float32, ok (n,) uint8, state_after (n,2) uint32)."""
    n = len(kind)
    mats = (abi.Material * n)()
    for i in range(n):
        mats[i] = abi.material(int(kind[i]), tuple(float(x) for x in albedo[i]), float(param[i]))
    f = lambda a: np.ascontiguousarray(a, np.float32)  # noqa: E731
    in_dir, point, normal = f(in_dir), f(point), f(normal)
    st = np.ascontiguousarray(rng_state, np.uint32)
    out_dir, ok, st_out = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros((n, 2), np.uint32)
    u32p = C.POINTER(C.c_uint32)
    abi.check(load_hip().rbrt_hip_debug_scatter(mats, abi.fptr(in_dir), abi.fptr(point), abi.fptr(normal), st.ctypes.data_as(u32p), n,
                                                 abi.fptr(out_dir), ok.ctypes.data_as(abi.u8p), st_out.ctypes.data_as(u32p)))
    return out_dir, ok, st_out


def packed_pixels(width: int, height: int, rank: int, world: int) -> int:
    return int(load_hip().rbrt_hip_packed_pixels(width, height, rank, world))


def unpack_tiles(device: int, d_gathered: int, width: int, height: int, world: int, d_radiance: int | None,
                 d_rgb8: int | None = None, stream: int | None = None, rank_stride_pixels: int = 0):
    """De-interleave gathered per-rank tiles; rank_stride_pixels > 0: equal-size slot per rank."""
    abi.check(load_hip().rbrt_hip_unpack_tiles_strided(device, C.c_void_p(stream or 0), C.c_void_p(d_gathered), width,
                                                       height, world, rank_stride_pixels, C.c_void_p(d_radiance or 0),
                                                       C.c_void_p(d_rgb8 or 0)))


def denoise_opts(window_radius: int | None = None, patch_radius: int | None = None, strength: float | None = None,
                 reserved: int = 0) -> abi.DenoiseOpts:
    """rbrt_denoise_opts_default, with the parameters that are given put in."""
    d = abi.DenoiseOpts()
    load_hip().rbrt_denoise_opts_default(C.byref(d))
    if window_radius is not None:
        d.window_radius = int(window_radius)
    if patch_radius is not None:
        d.patch_radius = int(patch_radius)
    if strength is not None:
        d.strength = float(strength)
    d.reserved = int(reserved)
    return d


def denoise_halves(device: int, d_a: int, d_b: int, d_wa: int | None, width: int, height: int, d_radiance: int | None,
                   d_rgb8: int | None = None, window_radius: int | None = None, patch_radius: int | None = None,
                   strength: float | None = None, stream: int | None = None, reserved: int = 0):
    """The dual-buffer non-local-means filter on two half images in device memory (rbrt_hip_denoise_halves): d_a, d_b
    row-major float32 [H, W, 3], d_wa float32 [H, W] or None (0.5 everywhere). Asynchronous on `stream`."""
    d = denoise_opts(window_radius, patch_radius, strength, reserved)
    abi.check(load_hip().rbrt_hip_denoise_halves(device, C.c_void_p(stream or 0), C.c_void_p(d_a), C.c_void_p(d_b),
                                                 C.c_void_p(d_wa or 0), width, height, C.byref(d), C.c_void_p(d_radiance or 0),
                                                 C.c_void_p(d_rgb8 or 0)))


def guided_opts(levels: int | None = None, colour: float | None = None, normal: float | None = None, depth: float | None = None,
                albedo: float | None = None, flags: int | None = None, reserved=(0, 0)) -> abi.GuidedOpts:
    """rbrt_guided_opts_default (5 levels, colour 2, normal 0.35, depth 0.05, albedo 0.1, flags 0), with the parameters that are
    given put in."""
    g = abi.GuidedOpts()
    load_hip().rbrt_guided_opts_default(C.byref(g))
    for name, value, kind in (("levels", levels, int), ("colour", colour, float), ("normal", normal, float), ("depth", depth, float),
                              ("albedo", albedo, float), ("flags", flags, int)):
        if value is not None:
            setattr(g, name, kind(value))
    g.reserved[0], g.reserved[1] = int(reserved[0]), int(reserved[1])
    return g


def guided_workspace_bytes(width: int, height: int) -> int:
    """rbrt_hip_guided_workspace_bytes: the device memory denoise_guided() needs; 0 for sizes it refuses."""
    return int(load_hip().rbrt_hip_guided_workspace_bytes(width, height))


def denoise_guided(device: int, d_a: int, d_b: int, d_wa: int | None, d_albedo: int, d_normal: int, d_depth: int, d_coverage: int,
                   width: int, height: int, d_workspace: int, d_radiance: int | None, d_rgb8: int | None = None,
                   opts: abi.GuidedOpts | None = None, stream: int | None = None):
    """The feature-guided a-trous filter on two half images in device memory (rbrt_hip_denoise_guided): d_a, d_b, d_albedo,
    d_normal row-major float32 [H, W, 3]; d_wa (None: 0.5 everywhere), d_depth, d_coverage float32 [H, W]; d_workspace
    guided_workspace_bytes(width, height) bytes, 16-byte aligned. `opts`: guided_opts(...), None for the library's defaults.
    An output may be d_a or d_b. Asynchronous on `stream`."""
    g = opts if opts is not None else guided_opts()
    abi.check(load_hip().rbrt_hip_denoise_guided(device, C.c_void_p(stream or 0), C.c_void_p(d_a or 0), C.c_void_p(d_b or 0),
                                                 C.c_void_p(d_wa or 0), C.c_void_p(d_albedo or 0), C.c_void_p(d_normal or 0),
                                                 C.c_void_p(d_depth or 0), C.c_void_p(d_coverage or 0), width, height, C.byref(g),
                                                 C.c_void_p(d_workspace or 0), C.c_void_p(d_radiance or 0), C.c_void_p(d_rgb8 or 0)))


def guided_staging(max_step: int = -1) -> int:
    """rbrt_hip_debug_guided_staging (test and measurement hook): the levels with a step of at most `max_step` (0..4) stage
    their tile in LDS; -1 asks. Returns the value in force."""
    rc = int(load_hip().rbrt_hip_debug_guided_staging(int(max_step)))
    if rc < 0:
        abi.check(rc)
    return rc


def temporal_opts(max_history: float | None = None, depth: float | None = None, normal: float | None = None,
                  flags: int | None = None, reserved=(0, 0, 0, 0)) -> abi.TemporalOpts:
    """rbrt_temporal_opts_default (max_history 32, depth 0.05, normal 0.35, flags 0), with the parameters that are given put in."""
    t = abi.TemporalOpts()
    load_hip().rbrt_temporal_opts_default(C.byref(t))
    for name, value, kind in (("max_history", max_history, float), ("depth", depth, float), ("normal", normal, float), ("flags", flags, int)):
        if value is not None:
            setattr(t, name, kind(value))
    for k in range(4):
        t.reserved[k] = int(reserved[k])
    return t


def temporal_history_bytes(width: int, height: int) -> int:
    """rbrt_hip_temporal_history_bytes: the device memory of one history of temporal_accumulate(); 0 for sizes it refuses."""
    return int(load_hip().rbrt_hip_temporal_history_bytes(width, height))


def temporal_accumulate(device: int, d_a: int, d_b: int, d_normal: int, d_depth: int, d_coverage: int, cam: abi.Camera,
                        cam_prev: abi.Camera | None, d_history_in: int | None, d_history_out: int | None,
                        d_out_a: int | None = None, d_out_b: int | None = None, d_out_length: int | None = None,
                        opts: abi.TemporalOpts | None = None, stream: int | None = None, d_motion: int | None = None,
                        phase_step: float | None = None):
    """One frame of temporal accumulation in device memory (rbrt_hip_temporal_accumulate): d_a, d_b, d_normal row-major float32
    [H, W, 3]; d_depth, d_coverage and d_out_length float32 [H, W], W and H being `cam`'s; the histories
    temporal_history_bytes(W, H) bytes each, 16-byte aligned, two that alternate. d_history_in None: the first frame (cam_prev
    may then be None). d_out_a may be d_a and d_out_b may be d_b. `opts`: temporal_opts(...), None for the library's defaults.
    Asynchronous on `stream`. With `d_motion` or `phase_step` not None the call is rbrt_hip_temporal_accumulate_moving: d_motion
    this frame's motion buffer, float32 [H, W, 3] (None or 0: its NULL), phase_step this frame's phase minus the last one's."""
    t = opts if opts is not None else temporal_opts()
    if d_motion is not None or phase_step is not None:
        abi.check(load_hip().rbrt_hip_temporal_accumulate_moving(
            device, C.c_void_p(stream or 0), C.c_void_p(d_a or 0), C.c_void_p(d_b or 0), C.c_void_p(d_normal or 0), C.c_void_p(d_depth or 0),
            C.c_void_p(d_coverage or 0), C.c_void_p(d_motion or 0), C.c_float(0.0 if phase_step is None else phase_step),
            C.byref(cam) if cam is not None else None, C.byref(cam_prev) if cam_prev is not None else None, C.byref(t),
            C.c_void_p(d_history_in or 0), C.c_void_p(d_history_out or 0), C.c_void_p(d_out_a or 0), C.c_void_p(d_out_b or 0),
            C.c_void_p(d_out_length or 0)))
        return
    abi.check(load_hip().rbrt_hip_temporal_accumulate(device, C.c_void_p(stream or 0), C.c_void_p(d_a or 0), C.c_void_p(d_b or 0),
                                                      C.c_void_p(d_normal or 0), C.c_void_p(d_depth or 0), C.c_void_p(d_coverage or 0),
                                                      C.byref(cam) if cam is not None else None,
                                                      C.byref(cam_prev) if cam_prev is not None else None, C.byref(t),
                                                      C.c_void_p(d_history_in or 0), C.c_void_p(d_history_out or 0),
                                                      C.c_void_p(d_out_a or 0), C.c_void_p(d_out_b or 0), C.c_void_p(d_out_length or 0)))


def upsample_opts(factor: int | None = None, normal: float | None = None, depth: float | None = None, albedo: float | None = None,
                  flags: int | None = None, reserved=(0, 0, 0)) -> abi.UpsampleOpts:
    """rbrt_upsample_opts_default (factor 2, normal 0.5, depth 0.1, albedo 0.2, flags 0), with the parameters that are given put in."""
    t = abi.UpsampleOpts()
    load_hip().rbrt_upsample_opts_default(C.byref(t))
    for name, value, kind in (("factor", factor, int), ("normal", normal, float), ("depth", depth, float), ("albedo", albedo, float),
                              ("flags", flags, int)):
        if value is not None:
            setattr(t, name, kind(value))
    for k in range(3):
        t.reserved[k] = int(reserved[k])
    return t


def upsample_workspace_bytes(width: int, height: int, factor: int) -> int:
    """rbrt_hip_upsample_workspace_bytes: the workspace of upsample_halves() for a width x height full-size image; 0 for what it refuses."""
    return int(load_hip().rbrt_hip_upsample_workspace_bytes(width, height, factor))


def upsample_camera(cam: abi.Camera, factor: int) -> abi.Camera:
    """rbrt_hip_upsample_camera: the camera of the low image whose pixels' footprints are the unions of `cam`'s f x f blocks."""
    low = abi.Camera()
    abi.check(load_hip().rbrt_hip_upsample_camera(C.byref(cam) if cam is not None else None, factor, C.byref(low)))
    return low


def upsample_halves(device: int, d_a: int, d_b: int, d_wa: int | None, d_albedo: int, d_normal: int, d_depth: int, d_coverage: int,
                    width: int, height: int, d_workspace: int, d_out_a: int | None = None, d_out_b: int | None = None,
                    d_out_wa: int | None = None, opts: abi.UpsampleOpts | None = None, stream: int | None = None):
    """Guided upsampling in device memory (rbrt_hip_upsample_halves): d_a, d_b float32 [h, w, 3] and d_wa float32 [h, w] (None: 0.5
    everywhere) at the low size of opts.factor; the features and the outputs at the full size width x height; d_workspace
    upsample_workspace_bytes(width, height, factor) bytes, 16-byte aligned. `opts`: upsample_opts(...), None for the library's
    defaults. Asynchronous on `stream`."""
    t = opts if opts is not None else upsample_opts()
    abi.check(load_hip().rbrt_hip_upsample_halves(device, C.c_void_p(stream or 0), C.c_void_p(d_a or 0), C.c_void_p(d_b or 0),
                                                  C.c_void_p(d_wa or 0), C.c_void_p(d_albedo or 0), C.c_void_p(d_normal or 0),
                                                  C.c_void_p(d_depth or 0), C.c_void_p(d_coverage or 0), width, height, C.byref(t),
                                                  C.c_void_p(d_workspace or 0), C.c_void_p(d_out_a or 0), C.c_void_p(d_out_b or 0),
                                                  C.c_void_p(d_out_wa or 0)))


def despike_opts(radius: int | None = None, rank: int | None = None, threshold: float | None = None, floor: float | None = None,
                 flags: int | None = None, reserved=(0, 0, 0)) -> abi.DespikeOpts:
    """rbrt_despike_opts_default (radius 2, rank 2, threshold 4, floor 0.01, flags 0), with the parameters that are given put in."""
    t = abi.DespikeOpts()
    load_hip().rbrt_despike_opts_default(C.byref(t))
    for name, value, kind in (("radius", radius, int), ("rank", rank, int), ("threshold", threshold, float), ("floor", floor, float),
                              ("flags", flags, int)):
        if value is not None:
            setattr(t, name, kind(value))
    for k in range(3):
        t.reserved[k] = int(reserved[k])
    return t


def despike_halves(device: int, d_a: int, d_b: int, width: int, height: int, d_out_a: int | None = None, d_out_b: int | None = None,
                   d_mask: int | None = None, d_result: int | None = None, opts: abi.DespikeOpts | None = None, stream: int | None = None):
    """Spike removal in device memory (rbrt_hip_despike_halves): d_a, d_b and the outputs d_out_a, d_out_b float32 [height, width, 3],
    d_mask uint8 [height, width] (bit 0: A was limited, bit 1: B), d_result 16 bytes (an abi.DespikeResult, zeroed by the call).
    `opts`: despike_opts(...), None for the library's defaults. Asynchronous on `stream`."""
    t = opts if opts is not None else despike_opts()
    abi.check(load_hip().rbrt_hip_despike_halves(device, C.c_void_p(stream or 0), C.c_void_p(d_a or 0), C.c_void_p(d_b or 0), width, height,
                                                 C.byref(t), C.c_void_p(d_out_a or 0), C.c_void_p(d_out_b or 0), C.c_void_p(d_mask or 0),
                                                 C.c_void_p(d_result or 0)))


def compare_opts(epsilon: float | None = None, flags: int | None = None, reserved=(0, 0)) -> abi.CompareOpts:
    """rbrt_compare_opts_default (epsilon 0.01, flags 0), with the parameters that are given put in."""
    t = abi.CompareOpts()
    load_hip().rbrt_compare_opts_default(C.byref(t))
    if epsilon is not None:
        t.epsilon = float(epsilon)
    if flags is not None:
        t.flags = int(flags)
    for k in range(2):
        t.reserved[k] = int(reserved[k])
    return t


def compare_workspace_bytes(width: int, height: int) -> int:
    """The bytes of the workspace a compare_images call with a result needs at this size (rbrt_hip_compare_workspace_bytes)."""
    return int(load_hip().rbrt_hip_compare_workspace_bytes(width, height))


def compare_images(device: int, d_x: int, d_ref: int, width: int, height: int, d_workspace: int | None = None, d_rel_map: int | None = None,
                   d_ssim_map: int | None = None, d_result: int | None = None, opts: abi.CompareOpts | None = None, stream: int | None = None):
    """An image against a reference in device memory (rbrt_hip_compare_images): d_x and d_ref float32 [height, width, 3], the maps
    d_rel_map and d_ssim_map float32 [height, width], d_result 64 bytes (an abi.CompareResult), d_workspace compare_workspace_bytes
    of the caller's, needed with d_result. `opts`: compare_opts(...), None for the library's defaults. Asynchronous on `stream`."""
    t = opts if opts is not None else compare_opts()
    abi.check(load_hip().rbrt_hip_compare_images(device, C.c_void_p(stream or 0), C.c_void_p(d_x or 0), C.c_void_p(d_ref or 0), width, height,
                                                 C.byref(t), C.c_void_p(d_workspace or 0), C.c_void_p(d_rel_map or 0), C.c_void_p(d_ssim_map or 0),
                                                 C.c_void_p(d_result or 0)))


def compare_summary(result: abi.CompareResult, width: int, height: int, peak: float = 1.0) -> abi.CompareSummary:
    """The means of a result that was copied to the host (rbrt_compare_summary; needs no GPU): mse, mae, relmse, psnr_db, ssim."""
    out = abi.CompareSummary()
    load_hip().rbrt_compare_summary(C.byref(result), width, height, float(peak), C.byref(out))
    return out


def tonemap_opts(curve: int | None = None, exposure: float | None = None, key: float | None = None,
                 key_permille: int | None = None, white: float | None = None, white_permille: int | None = None,
                 reserved=(0, 0)) -> abi.TonemapOpts:
    """rbrt_tonemap_opts_default (LINEAR, exposure 1, key 0.18 at permille 500, automatic white at permille 990), with the
    parameters that are given put in. exposure or white 0: automatic."""
    t = abi.TonemapOpts()
    load_hip().rbrt_tonemap_opts_default(C.byref(t))
    for name, value, kind in (("curve", curve, int), ("exposure", exposure, float), ("key", key, float),
                              ("key_permille", key_permille, int), ("white", white, float), ("white_permille", white_permille, int)):
        if value is not None:
            setattr(t, name, kind(value))
    t.reserved[0], t.reserved[1] = int(reserved[0]), int(reserved[1])
    return t


def tonemap(device: int, d_radiance: int, n_pixels: int, opts: abi.TonemapOpts, d_workspace: int | None,
            d_out_radiance: int | None, d_rgb8: int | None = None, stream: int | None = None):
    """The display transform on n_pixels pixels in device memory (rbrt_hip_tonemap): exposure, automatic exposure and white
    point from the luminance histogram, and the tone curve. d_workspace: abi.TONEMAP_WORKSPACE_BYTES bytes of device memory
    (the histogram, then an abi.TonemapResult), or None when nothing is automatic. d_out_radiance may be d_radiance (in
    place). Asynchronous on `stream`."""
    abi.check(load_hip().rbrt_hip_tonemap(device, C.c_void_p(stream or 0), C.c_void_p(d_radiance or 0), n_pixels,
                                          C.byref(opts) if opts is not None else None, C.c_void_p(d_workspace or 0),
                                          C.c_void_p(d_out_radiance or 0), C.c_void_p(d_rgb8 or 0)))


def glare_opts(threshold: float | None = None, intensity: float | None = None, levels: int | None = None,
               spread: float | None = None, reserved=(0, 0, 0, 0)) -> abi.GlareOpts:
    """rbrt_glare_opts_default (threshold 1, intensity 0.1, 5 levels, spread 1), with the parameters that are given put in."""
    g = abi.GlareOpts()
    load_hip().rbrt_glare_opts_default(C.byref(g))
    for name, value, kind in (("threshold", threshold, float), ("intensity", intensity, float), ("levels", levels, int),
                              ("spread", spread, float)):
        if value is not None:
            setattr(g, name, kind(value))
    for k in range(4):
        g.reserved[k] = int(reserved[k])
    return g


def glare_workspace_bytes(width: int, height: int, levels: int) -> int:
    """rbrt_hip_glare_workspace_bytes: the device memory glare() needs for its pyramid; 0 for sizes or levels it refuses."""
    return int(load_hip().rbrt_hip_glare_workspace_bytes(width, height, levels))


def glare(device: int, d_radiance: int, width: int, height: int, opts: abi.GlareOpts, d_workspace: int | None,
          d_out_radiance: int | None, d_rgb8: int | None = None, stream: int | None = None):
    """The glare stage on a row-major image in device memory (rbrt_hip_glare): a share of every bright pixel's light is moved
    into its surroundings through a pyramid of blurs. d_workspace: glare_workspace_bytes(width, height, opts.levels) bytes
    of device memory, 16-byte aligned. d_out_radiance may be d_radiance (in place). Asynchronous on `stream`."""
    abi.check(load_hip().rbrt_hip_glare(device, C.c_void_p(stream or 0), C.c_void_p(d_radiance or 0), width, height,
                                        C.byref(opts) if opts is not None else None, C.c_void_p(d_workspace or 0),
                                        C.c_void_p(d_out_radiance or 0), C.c_void_p(d_rgb8 or 0)))


def feature_opts(samples: int | None = None, reserved=(0, 0, 0)) -> abi.FeatureOpts:
    """rbrt_feature_opts_default (4 samples), with `samples` put in when it is given."""
    return abi.feature_opts(samples, reserved)


def write_pfm(path, rgb) -> None:
    """abi.write_pfm: a float32 (H, W, 3) image as a colour PFM."""
    abi.write_pfm(path, rgb)
