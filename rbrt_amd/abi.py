"""ctypes mirror of include/rbrt_hip.h (the C ABI of the HIP hot path).

Python here is plumbing for tests and bench.py: it declares the same POD structs a Rust
`extern "C"` block or the C++ host would, loads `rbrt_amd/lib/librbrt_hip.so`, and checks return
codes. There is no Python or CPU implementation of the render path behind it: if the shared
library is missing, `load_hip()` raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
LIB_HIP = ROOT / "rbrt_amd" / "lib" / "librbrt_hip.so"
LIB_HOST = ROOT / "rbrt_amd" / "lib" / "librbrt_host.so"

RBRT_OK = 0
RBRT_ERR_INVALID_ARG = -1
RBRT_ERR_NO_DEVICE = -2
RBRT_ERR_HIP = -3
RBRT_ERR_OOM = -4
RBRT_ERR_UNSUPPORTED = -5
RBRT_ERR_NAN = -6

MAT_LAMBERTIAN = 0
MAT_METAL = 1
MAT_DIELECTRIC = 2
MAT_EMISSIVE = 3  # albedo = emitted radiance

FLAG_COLLECT_STATS = 1
FLAG_CONSTANT_BACKGROUND = 2  # rays that hit nothing return opts.bg instead of the sky gradient
FLAG_THIN_LENS = 4  # the camera argument is the `cam` member of a CameraLens: defocus blur (rbrt_camera_lens_t)
TILE = 8
TONE_LINEAR, TONE_REINHARD, TONE_ACES = 0, 1, 2  # rbrt_tonemap_opts_t::curve
TONEMAP_BINS = 4096
TONEMAP_RESULT_OFFSET = TONEMAP_BINS * 4
TONEMAP_WORKSPACE_BYTES = TONEMAP_RESULT_OFFSET + 32
TONEMAP_BLOCK_PIXELS = 1024  # rbrt_hip_debug.h: pixels a workgroup of the transform's kernels takes per stride
TONEMAP_MAX_BLOCKS = 512     # ... and the cap of their grid
GUIDED_NO_DEMODULATION = 1   # rbrt_hip.h: RBRT_GUIDED_NO_DEMODULATION
GUIDED_MAX_LEVELS = 6        # rbrt_hip.h: the most levels of the guided denoiser
TEMPORAL_HISTORY_BYTES_PER_PIXEL = 48  # rbrt_hip.h: three 16-byte records {A', len}, {B', c}, {N, z}
TEMPORAL_BLOCK = 256         # rbrt_hip_debug.h: consecutive pixels a workgroup of the temporal kernel takes
UPSAMPLE_MAX_FACTOR = 4      # rbrt_hip.h: RBRT_UPSAMPLE_MAX_FACTOR
UPSAMPLE_NO_DEMODULATION = 1  # rbrt_hip.h: RBRT_UPSAMPLE_NO_DEMODULATION
UPSAMPLE_WORKSPACE_BYTES_PER_LOW_PIXEL = 64  # rbrt_hip.h: four 16-byte records {a~, wa}, {b~, z_l}, {N_l, c_l}, {m_l, 0}
UPSAMPLE_TILE_W = 32         # rbrt_hip_debug.h: the tile of full pixels one workgroup of the upsampling's gather kernel makes
UPSAMPLE_TILE_H = 8
DESPIKE_MAX_RADIUS = 2       # rbrt_hip.h: RBRT_DESPIKE_MAX_RADIUS
DESPIKE_MAX_RANK = 4         # rbrt_hip.h: RBRT_DESPIKE_MAX_RANK
DESPIKE_TILE_W = 32          # rbrt_hip_debug.h: the tile of pixels one workgroup of the spike removal's kernel makes
DESPIKE_TILE_H = 8
COMPARE_TILE_W = 16          # rbrt_hip.h: RBRT_COMPARE_TILE_W, the tile of the image comparison's sums (part of its rule)
COMPARE_TILE_H = 16
GLARE_MAX_LEVELS = 8         # rbrt_hip.h: the most levels of the glare stage's pyramid
GLARE_TILE_W = 16            # rbrt_hip_debug.h: the tile of a pyramid level one workgroup of the REDUCE kernel makes
GLARE_TILE_H = 16

f32p = C.POINTER(C.c_float)
u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)


class Material(C.Structure):
    _fields_ = [("kind", C.c_int32), ("albedo", C.c_float * 3), ("param", C.c_float)]


class Sphere(C.Structure):
    _fields_ = [("center", C.c_float * 3), ("radius", C.c_float), ("mat", Material)]


class Mesh(C.Structure):
    _fields_ = [
        ("n_total", C.c_uint32),
        ("n_real", C.c_uint32),
        ("v0x", f32p), ("v0y", f32p), ("v0z", f32p),
        ("e1x", f32p), ("e1y", f32p), ("e1z", f32p),
        ("e2x", f32p), ("e2y", f32p), ("e2z", f32p),
        ("nx", f32p), ("ny", f32p), ("nz", f32p),
        ("is_padding", u8p),
        ("bbox_lo", C.c_float * 3),
        ("bbox_hi", C.c_float * 3),
        ("mat", Material),
    ]


class Triangle(C.Structure):
    _fields_ = [("corners", (C.c_float * 3) * 3), ("mat", Material)]


class Scene(C.Structure):
    _fields_ = [
        ("n_spheres", C.c_uint32),
        ("spheres", C.POINTER(Sphere)),
        ("n_meshes", C.c_uint32),
        ("meshes", C.POINTER(Mesh)),
        ("n_triangles", C.c_uint32),
        ("triangles", C.POINTER(Triangle)),
        ("element_order", C.POINTER(C.c_uint32)),
    ]


NORMAL_FIELDS = ("n0x", "n0y", "n0z", "n1x", "n1y", "n1z", "n2x", "n2y", "n2z")


class MeshNormals(C.Structure):
    """rbrt_mesh_normals_t: the corner normals of a smooth mesh's SoA entries (all NULL: flat)."""
    _fields_ = [(k, f32p) for k in NORMAL_FIELDS]


class SceneShading(C.Structure):
    """rbrt_scene_shading_t: one MeshNormals per mesh of the scene."""
    _fields_ = [("n_meshes", C.c_uint32), ("reserved", C.c_uint32), ("meshes", C.POINTER(MeshNormals))]


PATTERN_NONE, PATTERN_CHECKER = 0, 1


class Pattern(C.Structure):
    """rbrt_pattern_t: a solid pattern of one object (32 bytes)."""
    _fields_ = [("kind", C.c_uint32), ("albedo2", C.c_float * 3), ("origin", C.c_float * 3), ("size", C.c_float)]


class ScenePatterns(C.Structure):
    """rbrt_scene_patterns_t: one Pattern per object of the scene, by object id."""
    _fields_ = [("n_objects", C.c_uint32), ("reserved", C.c_uint32), ("objects", C.POINTER(Pattern))]


def checker(albedo2, size, origin=(0.0, 0.0, 0.0)) -> Pattern:
    """A RBRT_PATTERN_CHECKER: albedo2 in the odd cells, cells of edge `size` counted from `origin`."""
    return Pattern(PATTERN_CHECKER, _f3(albedo2), _f3(origin), float(size))


class Camera(C.Structure):
    _fields_ = [
        ("position", C.c_float * 3),
        ("right", C.c_float * 3),
        ("up", C.c_float * 3),
        ("img_center_point", C.c_float * 3),
        ("mm_per_pix_hor", C.c_float),
        ("mm_per_pix_vert", C.c_float),
        ("img_width_pix", C.c_uint32),
        ("img_height_pix", C.c_uint32),
    ]


class CameraLens(C.Structure):
    """rbrt_camera_lens_t: a Camera and the thin lens around its position (RBRT_FLAG_THIN_LENS). The render calls receive
    C.byref(lens.cam), which points into this struct."""
    _fields_ = [
        ("cam", Camera),
        ("lens_u", C.c_float * 3),  # lens half-axes in scene units (radius applied)
        ("lens_v", C.c_float * 3),
        ("focus_scale", C.c_float),  # focus surface = the image plane scaled about cam.position by this factor
        ("reserved", C.c_uint32),
    ]


def camera_lens(cam: Camera, lens_u, lens_v, focus_scale: float) -> CameraLens:
    """A CameraLens holding a copy of `cam`."""
    L = CameraLens()
    C.memmove(C.byref(L.cam), C.byref(cam), C.sizeof(Camera))
    L.lens_u = _f3(lens_u)
    L.lens_v = _f3(lens_v)
    L.focus_scale = float(focus_scale)
    L.reserved = 0
    return L


class RenderOpts(C.Structure):
    _fields_ = [
        ("spp", C.c_uint32),
        ("max_depth", C.c_uint32),
        ("min_dist", C.c_float),
        ("max_dist", C.c_float),
        ("bg", C.c_float * 3),
        ("seed", C.c_uint64),
        ("tile_rank", C.c_uint32),
        ("tile_world", C.c_uint32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class AdaptiveOpts(C.Structure):  # rbrt_adaptive_opts_t
    _fields_ = [("threshold", C.c_float), ("min_samples", C.c_uint32), ("step", C.c_uint32), ("reserved", C.c_uint32)]


class AdaptiveResult(C.Structure):  # rbrt_adaptive_result_t
    _fields_ = [("rounds", C.c_uint32), ("reserved", C.c_uint32), ("samples", C.c_uint64), ("samples_fixed", C.c_uint64)]


class DenoiseOpts(C.Structure):  # rbrt_denoise_opts_t
    _fields_ = [("window_radius", C.c_uint32), ("patch_radius", C.c_uint32), ("strength", C.c_float), ("reserved", C.c_uint32)]


class TonemapOpts(C.Structure):  # rbrt_tonemap_opts_t
    _fields_ = [("curve", C.c_uint32), ("exposure", C.c_float), ("key", C.c_float), ("key_permille", C.c_uint32),
                ("white", C.c_float), ("white_permille", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TonemapResult(C.Structure):  # rbrt_tonemap_result_t: behind the histogram in the workspace, in device memory
    _fields_ = [("exposure", C.c_float), ("white", C.c_float), ("l_key", C.c_float), ("l_white", C.c_float),
                ("counted", C.c_uint32), ("reserved", C.c_uint32), ("pixels", C.c_uint64)]


class GlareOpts(C.Structure):  # rbrt_glare_opts_t
    _fields_ = [("threshold", C.c_float), ("intensity", C.c_float), ("levels", C.c_uint32), ("spread", C.c_float),
                ("reserved", C.c_uint32 * 4)]


class FeatureOpts(C.Structure):  # rbrt_feature_opts_t
    _fields_ = [("samples", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class GuidedOpts(C.Structure):  # rbrt_guided_opts_t
    _fields_ = [("levels", C.c_uint32), ("colour", C.c_float), ("normal", C.c_float), ("depth", C.c_float), ("albedo", C.c_float),
                ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class TemporalOpts(C.Structure):  # rbrt_temporal_opts_t
    _fields_ = [("max_history", C.c_float), ("depth", C.c_float), ("normal", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class UpsampleOpts(C.Structure):  # rbrt_upsample_opts_t
    _fields_ = [("factor", C.c_uint32), ("normal", C.c_float), ("depth", C.c_float), ("albedo", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class DespikeOpts(C.Structure):  # rbrt_despike_opts_t
    _fields_ = [("radius", C.c_uint32), ("rank", C.c_uint32), ("threshold", C.c_float), ("floor", C.c_float), ("flags", C.c_uint32),
                ("reserved", C.c_uint32 * 3)]


class DespikeResult(C.Structure):  # rbrt_despike_result_t: in device memory
    _fields_ = [("spikes_a", C.c_uint32), ("spikes_b", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CompareOpts(C.Structure):  # rbrt_compare_opts_t
    _fields_ = [("epsilon", C.c_float), ("flags", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class CompareResult(C.Structure):  # rbrt_compare_result_t: in device memory, 64 bytes
    _fields_ = [("sum_se", C.c_double), ("sum_ae", C.c_double), ("sum_rel", C.c_double), ("sum_ssim", C.c_double), ("max_abs", C.c_float),
                ("usable", C.c_uint32), ("skipped", C.c_uint32), ("reserved", C.c_uint32 * 5)]


class CompareSummary(C.Structure):  # rbrt_compare_summary_t
    _fields_ = [("mse", C.c_double), ("mae", C.c_double), ("relmse", C.c_double), ("psnr_db", C.c_double), ("ssim", C.c_double)]


class Environment(C.Structure):  # rbrt_environment_t
    """An octahedral radiance map of (n + 1) x (n + 1) nodes: `nodes` points at host float32 [n + 1][n + 1][3]."""
    _fields_ = [("n", C.c_uint32), ("reserved", C.c_uint32), ("nodes", f32p)]


class Shutter(C.Structure):  # rbrt_shutter_t
    """The camera's translation between the opening and the closing of the shutter, in scene units."""
    _fields_ = [("travel", C.c_float * 3), ("reserved", C.c_uint32)]


class Motion(C.Structure):  # rbrt_motion_t
    """A travel per sphere between the opening and the closing of the shutter, in scene units: travel = float[n_spheres][3]."""
    _fields_ = [("n_spheres", C.c_uint32), ("reserved", C.c_uint32), ("travel", f32p)]


class MeshMotion(C.Structure):  # rbrt_mesh_motion_t
    """A travel per mesh between the opening and the closing of the shutter, in scene units: travel = float[n_meshes][3]."""
    _fields_ = [("n_meshes", C.c_uint32), ("reserved", C.c_uint32), ("travel", f32p)]


class Stats(C.Structure):
    _fields_ = [
        ("rays", C.c_uint64),
        ("mesh_gate_pass", C.c_uint64),
        ("nodes_visited", C.c_uint64),
        ("tris_tested", C.c_uint64),
        ("mesh_hits", C.c_uint64),
        ("samples", C.c_uint64),
        ("nan_discriminants", C.c_uint64),
        ("node_bytes", C.c_uint32),
        ("tri_bytes", C.c_uint32),
    ]


class SceneInfo(C.Structure):
    _fields_ = [
        ("n_spheres", C.c_uint32), ("n_meshes", C.c_uint32),
        ("n_meshes_device_built", C.c_uint32), ("bvh_stack_need", C.c_uint32),
        ("n_nodes", C.c_uint64), ("n_triangles", C.c_uint64),
        ("trace_waves", C.c_uint32), ("lds_bytes_per_wave", C.c_uint32),
        ("occupancy_api_waves_per_cu", C.c_uint32), ("n_cus", C.c_uint32),
    ]


class CallTimes(C.Structure):  # rbrt_hip_call_times_t (include/rbrt_hip_debug.h)
    _fields_ = [(k, C.c_double) for k in ("hip_init_s", "upload_s", "bvh_build_s", "lanes_s", "create_s", "render_s", "copy_s",
                                          "destroy_s", "total_s")] + [("meshes_device_built", C.c_uint32), ("meshes_host_built", C.c_uint32)]

    def as_dict(self) -> dict:
        return {k: getattr(self, k) for k, _ in self._fields_}


# every symbol include/rbrt_hip.h (the drop-in boundary) declares: name -> (restype, argtypes)
HIP_SYMBOLS = {
    "rbrt_hip_render": (C.c_int, [C.POINTER(Camera), C.POINTER(Scene), C.POINTER(RenderOpts), f32p, u8p]),
    "rbrt_hip_scene_create": (C.c_int, [C.POINTER(Scene), C.c_int, C.POINTER(C.c_void_p)]),
    "rbrt_hip_scene_destroy": (C.c_int, [C.c_void_p]),
    "rbrt_hip_packed_pixels": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    "rbrt_hip_tile_xy": (None, [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rbrt_hip_tile_number": (C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rbrt_hip_render_device": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p,
                                         C.c_void_p, C.c_void_p]),
    "rbrt_hip_render_pass": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.c_void_p, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_hip_unpack_tiles": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                        C.c_void_p, C.c_void_p]),
    "rbrt_hip_unpack_tiles_strided": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.c_size_t, C.c_void_p, C.c_void_p]),
    "rbrt_hip_scene_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "rbrt_hip_scene_check": (C.c_int, [C.c_void_p]),
    "rbrt_render_opts_default": (None, [C.POINTER(RenderOpts)]),
    "rbrt_hip_device_count": (C.c_int, []),
    "rbrt_hip_last_error": (C.c_char_p, []),
    "rbrt_hip_abi_version": (C.c_int, []),
    "rbrt_hip_scene_set_pipeline": (C.c_int, [C.c_void_p, C.c_uint32]),
    "rbrt_hip_scene_info": (C.c_int, [C.c_void_p, C.POINTER(SceneInfo)]),
    "rbrt_hip_supported_flags": (C.c_uint32, []),
    "rbrt_hip_scene_create_shaded": (C.c_int, [C.POINTER(Scene), C.POINTER(SceneShading), C.c_int, C.POINTER(C.c_void_p)]),
    "rbrt_hip_scene_create_patterned": (C.c_int, [C.POINTER(Scene), C.POINTER(SceneShading), C.POINTER(ScenePatterns), C.c_int,
                                                  C.POINTER(C.c_void_p)]),
    "rbrt_hip_render_patterned": (C.c_int, [C.POINTER(Camera), C.POINTER(Scene), C.POINTER(SceneShading), C.POINTER(ScenePatterns),
                                            C.POINTER(RenderOpts), f32p, u8p]),
    "rbrt_hip_render_shaded": (C.c_int, [C.POINTER(Camera), C.POINTER(Scene), C.POINTER(SceneShading), C.POINTER(RenderOpts),
                                         f32p, u8p]),
    "rbrt_hip_render_adaptive": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(AdaptiveOpts), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AdaptiveResult)]),
    "rbrt_denoise_opts_default": (None, [C.POINTER(DenoiseOpts)]),
    "rbrt_hip_denoise_halves": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                          C.POINTER(DenoiseOpts), C.c_void_p, C.c_void_p]),
    "rbrt_tonemap_opts_default": (None, [C.POINTER(TonemapOpts)]),
    "rbrt_hip_tonemap": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TonemapOpts), C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "rbrt_glare_opts_default": (None, [C.POINTER(GlareOpts)]),
    "rbrt_hip_glare_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rbrt_hip_glare": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(GlareOpts), C.c_void_p, C.c_void_p,
                                 C.c_void_p]),
    "rbrt_hip_scene_denoise": (C.c_int, [C.c_void_p, C.POINTER(DenoiseOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_hip_scene_set_environment": (C.c_int, [C.c_void_p, C.POINTER(Environment)]),
    "rbrt_hip_scene_set_shutter": (C.c_int, [C.c_void_p, C.POINTER(Shutter)]),
    "rbrt_hip_scene_set_motion": (C.c_int, [C.c_void_p, C.POINTER(Motion)]),
    "rbrt_hip_scene_set_motion_phase": (C.c_int, [C.c_void_p, C.c_float]),
    "rbrt_hip_scene_set_mesh_motion": (C.c_int, [C.c_void_p, C.POINTER(MeshMotion)]),
    "rbrt_hip_render_features_motion": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(FeatureOpts), C.c_void_p,
                                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_hip_temporal_accumulate_moving": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                       C.c_void_p, C.c_float, C.POINTER(Camera), C.POINTER(Camera), C.POINTER(TemporalOpts),
                                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_feature_opts_default": (None, [C.POINTER(FeatureOpts)]),
    "rbrt_hip_render_features": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(FeatureOpts), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_guided_opts_default": (None, [C.POINTER(GuidedOpts)]),
    "rbrt_hip_guided_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rbrt_hip_denoise_guided": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(GuidedOpts), C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_hip_scene_denoise_guided": (C.c_int, [C.c_void_p, C.POINTER(GuidedOpts), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_temporal_opts_default": (None, [C.POINTER(TemporalOpts)]),
    "rbrt_hip_temporal_history_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rbrt_hip_temporal_accumulate": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(Camera), C.POINTER(Camera), C.POINTER(TemporalOpts), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_upsample_opts_default": (None, [C.POINTER(UpsampleOpts)]),
    "rbrt_hip_upsample_camera": (C.c_int, [C.POINTER(Camera), C.c_uint32, C.POINTER(Camera)]),
    "rbrt_hip_upsample_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32, C.c_uint32]),
    "rbrt_hip_upsample_halves": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(UpsampleOpts), C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "rbrt_despike_opts_default": (None, [C.POINTER(DespikeOpts)]),
    "rbrt_hip_despike_halves": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(DespikeOpts), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_compare_opts_default": (None, [C.POINTER(CompareOpts)]),
    "rbrt_hip_compare_workspace_bytes": (C.c_size_t, [C.c_uint32, C.c_uint32]),
    "rbrt_hip_compare_images": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(CompareOpts), C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "rbrt_compare_summary": (None, [C.POINTER(CompareResult), C.c_uint32, C.c_uint32, C.c_double, C.POINTER(CompareSummary)]),
}
# ... and include/rbrt_hip_debug.h (test hooks and diagnostics, same library)
DEBUG_SYMBOLS = {
    "rbrt_hip_debug_guided_staging": (C.c_int, [C.c_int]),
    "rbrt_hip_scene_last_batching": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rbrt_hip_trace_rays": (C.c_int, [C.c_void_p, f32p, C.c_size_t, C.c_float, C.c_float, f32p, i32p, i32p, f32p]),
    "rbrt_hip_selftest_ieee": (C.c_int, [C.c_uint64, C.c_size_t, C.POINTER(C.c_uint64)]),
    "rbrt_hip_debug_ieee": (C.c_int, [f32p, C.c_size_t, f32p, C.c_size_t, f32p, u8p, f32p, u8p]),
    "rbrt_hip_selftest_sqrt_sweep": (C.c_int, [C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "rbrt_hip_selftest_gate": (C.c_int, [f32p, f32p, f32p, C.c_size_t, u8p, u8p]),
    "rbrt_hip_bvh_build_host": (C.c_int, [C.POINTER(Mesh), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                          C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                          f32p]),
    "rbrt_hip_free_host": (None, [C.c_void_p]),
    "rbrt_hip_bvh_build_host_records": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32), f32p]),
    "rbrt_hip_bvh_build_device": (C.c_int, [C.POINTER(Mesh), C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                            C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(C.c_uint32),
                                            f32p, C.POINTER(C.c_int)]),
    "rbrt_hip_scene_debug_counters": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t]),
    "rbrt_hip_scene_set_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "rbrt_hip_scene_kernel_ms": (C.c_int, [C.c_void_p, f32p, f32p, C.POINTER(C.c_uint32)]),
    "rbrt_hip_scene_debug_set_counter": (C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64]),
    "rbrt_hip_scene_launch_mix": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "rbrt_hip_debug_scatter": (C.c_int, [C.POINTER(Material), f32p, f32p, f32p, C.POINTER(C.c_uint32), C.c_size_t, f32p, u8p,
                                        C.POINTER(C.c_uint32)]),
    "rbrt_hip_debug_primary_cull": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(C.c_uint32), C.c_size_t]),
    "rbrt_hip_debug_primary_cull_lens": (C.c_int, [C.c_void_p, C.POINTER(CameraLens), C.POINTER(C.c_uint32), C.c_size_t]),
    "rbrt_hip_debug_primary_cull_shutter": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(CameraLens), C.POINTER(C.c_float),
                                                      C.POINTER(C.c_uint32), C.c_size_t]),
    "rbrt_hip_debug_primary_cull_opts": (C.c_int, [C.c_void_p, C.POINTER(Camera), C.POINTER(RenderOpts), C.POINTER(C.c_uint32), C.c_size_t]),
    "rbrt_hip_scene_helper_launches": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "rbrt_hip_scene_last_trace_build": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "rbrt_hip_scene_create_times": (C.c_int, [C.c_void_p, C.POINTER(CallTimes)]),
    "rbrt_hip_last_render_times": (C.c_int, [C.POINTER(CallTimes)]),
    "rbrt_hip_scene_refine_wait": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "rbrt_hip_debug_shading_normals": (C.c_int, [C.c_void_p, f32p, C.c_size_t, C.c_float, C.c_float, f32p]),
    "rbrt_hip_debug_surface_albedo": (C.c_int, [C.c_void_p, f32p, C.c_size_t, C.c_float, C.c_float, f32p]),
    "rbrt_hip_scene_adaptive_rounds": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32)]),
    "rbrt_hip_debug_environment": (C.c_int, [C.c_void_p, f32p, C.c_size_t, f32p]),
    "rbrt_hip_scene_set_short_paths": (C.c_int, [C.c_void_p, C.c_int]),
    "rbrt_hip_debug_short_masks": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(C.c_size_t)]),
}


class RbrtError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"rbrt_hip error {code}: {msg}")
        self.code = code


_hip = None


def _preload_torch_hip_runtime() -> None:
    """One HIP runtime per process.

    The PyTorch wheel bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and finds it by file
    name, so a process that loaded /opt/rocm's copy first ends up with two HIP/HSA runtimes and
    torch then reports "No HIP GPUs are available". bench.py and some tests use torch for device
    buffers and torch.distributed next to this library, so when torch is installed its runtime is
    loaded first and librbrt_hip.so's NEEDED libamdhip64.so.7 binds to that same copy. Without
    torch (the C++ host, a Rust host) the system runtime under /opt/rocm is used as usual.
    """
    if os.environ.get("RBRT_NO_TORCH_PRELOAD"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = Path(spec.origin).parent / "lib" / "libamdhip64.so"
        if cand.exists():
            C.CDLL(str(cand), mode=getattr(os, "RTLD_GLOBAL", 0x100) | getattr(os, "RTLD_NOW", 2))
    except OSError:
        pass


def load_hip() -> C.CDLL:
    """Load the product library. Fails loudly when it has not been built: no fallback exists."""
    global _hip
    if _hip is not None:
        return _hip
    lib_path = Path(os.environ.get("RBRT_HIP_LIB", LIB_HIP))  # override: A/B builds of the same ABI
    if not lib_path.exists():
        raise FileNotFoundError(
            f"{lib_path} is missing: build it with `make` (or __graft_entry__.build()). "
            "rbrt_amd has no CPU or pure-Python render path.")
    _preload_torch_hip_runtime()
    lib = C.CDLL(str(lib_path), mode=getattr(os, "RTLD_NOW", 2))
    for name, (res, args) in {**HIP_SYMBOLS, **DEBUG_SYMBOLS}.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _hip = lib
    return lib


def check(code: int) -> None:
    if code != RBRT_OK:
        raise RbrtError(code, load_hip().rbrt_hip_last_error().decode(errors="replace"))


# ------------------------------------------------------------------------------------------
# helpers to build the POD structs from Python values (keeping the backing arrays alive)
# ------------------------------------------------------------------------------------------

def _f3(v):
    return (C.c_float * 3)(*[float(x) for x in v])


def material(kind: int, albedo=(0.0, 0.0, 0.0), param: float = 0.0) -> Material:
    return Material(kind, _f3(albedo), float(param))


def fptr(a: np.ndarray):
    assert a.dtype == np.float32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(f32p)


class SceneData:
    """Owns the numpy arrays and ctypes arrays a `Scene` struct points into."""

    def __init__(self, spheres=(), meshes=(), triangles=(), element_order=None, patterns=None):
        # spheres: iterable of (center, radius, Material); meshes: iterable of MeshData; triangles: iterable of
        # (corners (3,3), Material); element_order: None or entries as in rbrt_scene_t.element_order;
        # patterns: None or {object id: Pattern} (rbrt_scene_t's numbering: elements in their order, then meshes)
        self.spheres = list(spheres)
        self.meshes = list(meshes)
        self.triangles = list(triangles)
        self.element_order = None if element_order is None else [int(x) for x in element_order]
        self._sph = (Sphere * max(1, len(self.spheres)))()
        for i, (c, r, m) in enumerate(self.spheres):
            self._sph[i] = Sphere(_f3(c), float(r), m)
        self._msh = (Mesh * max(1, len(self.meshes)))()
        for i, md in enumerate(self.meshes):
            self._msh[i] = md.struct
        self._tri = (Triangle * max(1, len(self.triangles)))()
        for i, (corners, m) in enumerate(self.triangles):
            for a in range(3):
                for b in range(3):
                    self._tri[i].corners[a][b] = float(corners[a][b])
            self._tri[i].mat = m
        self._order = None if self.element_order is None else (C.c_uint32 * len(self.element_order))(*self.element_order)
        self.struct = Scene(len(self.spheres), self._sph, len(self.meshes), self._msh, len(self.triangles), self._tri,
                            self._order if self._order is not None else C.POINTER(C.c_uint32)())
        # smooth shading: an rbrt_scene_shading_t only when some mesh has corner normals
        self._nrm = (MeshNormals * max(1, len(self.meshes)))()
        for i, md in enumerate(self.meshes):
            if md.normals is not None:
                self._nrm[i] = md.normals_struct
        self.shading = (SceneShading(len(self.meshes), 0, self._nrm)
                        if any(md.normals is not None for md in self.meshes) else None)
        # solid patterns: an rbrt_scene_patterns_t only when some object carries one
        self.pattern_of = dict(patterns or {})
        n_obj = len(self.spheres) + len(self.triangles) + len(self.meshes)
        self._pat = (Pattern * max(1, n_obj))()
        for k, p in self.pattern_of.items():
            self._pat[int(k)] = p
        self.patterns = ScenePatterns(n_obj, 0, self._pat) if self.pattern_of else None

    def ptr(self):
        return C.byref(self.struct)

    def shading_ptr(self):
        """The rbrt_scene_shading_t* of the *_shaded entry points, or None when every mesh is flat."""
        return None if self.shading is None else C.byref(self.shading)

    def patterns_ptr(self):
        """The rbrt_scene_patterns_t* of the *_patterned entry points, or None when no object carries a pattern."""
        return None if self.patterns is None else C.byref(self.patterns)


class MeshData:
    """SoA arrays of one mesh in the reference's layout (mesh.rs:12-25)."""

    FIELDS = ("v0x", "v0y", "v0z", "e1x", "e1y", "e1z", "e2x", "e2y", "e2z", "nx", "ny", "nz")

    def __init__(self, arrays: dict, is_padding: np.ndarray, n_real: int, bbox_lo, bbox_hi, mat: Material, normals=None):
        """normals: None (flat) or a dict of the nine corner normal arrays n0x .. n2z (n_total each): a smooth mesh."""
        self.arrays = {k: np.ascontiguousarray(arrays[k], dtype=np.float32) for k in self.FIELDS}
        self.is_padding = np.ascontiguousarray(is_padding, dtype=np.uint8)
        n_total = len(self.is_padding)
        for k in self.FIELDS:
            assert len(self.arrays[k]) == n_total, k
        self.n_total, self.n_real = n_total, int(n_real)
        self.bbox_lo, self.bbox_hi = np.float32(bbox_lo), np.float32(bbox_hi)
        self.struct = Mesh()
        self.struct.n_total = n_total
        self.struct.n_real = self.n_real
        for k in self.FIELDS:
            setattr(self.struct, k, fptr(self.arrays[k]))
        self.struct.is_padding = self.is_padding.ctypes.data_as(u8p)
        self.struct.bbox_lo = _f3(bbox_lo)
        self.struct.bbox_hi = _f3(bbox_hi)
        self.struct.mat = mat
        self.normals = None
        self.normals_struct = MeshNormals()
        if normals is not None:
            self.normals = {k: np.ascontiguousarray(normals[k], dtype=np.float32) for k in NORMAL_FIELDS}
            for k in NORMAL_FIELDS:
                assert len(self.normals[k]) == n_total, k
                setattr(self.normals_struct, k, fptr(self.normals[k]))

    def with_normals(self, normals):
        """A copy of this mesh with corner normals (None: flat), sharing nothing mutable with it."""
        return MeshData(self.arrays, self.is_padding, self.n_real, self.bbox_lo, self.bbox_hi, self.struct.mat, normals)


def default_opts(spp: int = 5, seed: int = 1, **kw) -> RenderOpts:
    o = RenderOpts()
    o.spp, o.max_depth, o.min_dist, o.max_dist = spp, 50, 0.001, 2000.0
    o.bg = _f3((0.05, 0.05, 0.8))
    o.seed, o.tile_rank, o.tile_world, o.flags, o.reserved = seed, 0, 1, 0, 0
    for k, v in kw.items():
        if k == "bg":
            o.bg = _f3(v)
        else:
            setattr(o, k, v)
    return o


def feature_opts(samples: int | None = None, reserved=(0, 0, 0)) -> FeatureOpts:
    """rbrt_feature_opts_default (4 samples a pixel), with `samples` put in when it is given."""
    f = FeatureOpts()
    load_hip().rbrt_feature_opts_default(C.byref(f))
    if samples is not None:
        f.samples = int(samples)
    for k in range(3):
        f.reserved[k] = int(reserved[k])
    return f


# ------------------------------------------------------------------------------------------
# C++ host library (rbrt_amd/host): YAML scene -> camera + SoA meshes, PNG writer
# ------------------------------------------------------------------------------------------
_host = None


def load_host() -> C.CDLL:
    global _host
    if _host is not None:
        return _host
    if not LIB_HOST.exists():
        raise FileNotFoundError(f"{LIB_HOST} is missing: build it with `make`")
    lib = C.CDLL(str(LIB_HOST))
    lib.rbrt_host_last_error.restype = C.c_char_p
    lib.rbrt_host_scene_load.restype = C.c_int
    lib.rbrt_host_scene_load.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
    lib.rbrt_host_scene_camera.restype = C.POINTER(Camera)
    lib.rbrt_host_scene_camera.argtypes = [C.c_void_p]
    lib.rbrt_host_scene_lens.restype = C.POINTER(CameraLens)
    lib.rbrt_host_scene_lens.argtypes = [C.c_void_p]
    lib.rbrt_host_scene_shutter_travel.restype = f32p
    lib.rbrt_host_scene_shutter_travel.argtypes = [C.c_void_p]
    lib.rbrt_host_shutter_fingerprint.restype = C.c_uint64
    lib.rbrt_host_shutter_fingerprint.argtypes = [f32p, C.c_uint64]
    lib.rbrt_host_scene_motion.restype = f32p
    lib.rbrt_host_scene_motion.argtypes = [C.c_void_p]
    lib.rbrt_host_scene_mesh_motion.restype = f32p
    lib.rbrt_host_scene_mesh_motion.argtypes = [C.c_void_p]
    lib.rbrt_host_mesh_motion_fingerprint.restype = C.c_uint64
    lib.rbrt_host_mesh_motion_fingerprint.argtypes = [f32p, C.c_uint32, C.c_uint64]
    lib.rbrt_host_motion_fingerprint.restype = C.c_uint64
    lib.rbrt_host_motion_fingerprint.argtypes = [f32p, C.c_uint32, C.c_uint64]
    lib.rbrt_host_scene_scene.restype = C.POINTER(Scene)
    lib.rbrt_host_scene_scene.argtypes = [C.c_void_p]
    lib.rbrt_host_scene_shading.restype = C.POINTER(SceneShading)
    lib.rbrt_host_scene_shading.argtypes = [C.c_void_p]
    lib.rbrt_host_scene_patterns.restype = C.POINTER(ScenePatterns)
    lib.rbrt_host_scene_patterns.argtypes = [C.c_void_p]
    lib.rbrt_host_scene_environment.restype = f32p
    lib.rbrt_host_scene_environment.argtypes = [C.c_void_p, C.POINTER(C.c_uint32)]
    lib.rbrt_host_read_pfm.restype = C.c_int
    lib.rbrt_host_read_pfm.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), f32p]
    lib.rbrt_host_read_pfm_any.restype = C.c_int
    lib.rbrt_host_read_pfm_any.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), f32p]
    lib.rbrt_host_write_pfm.restype = C.c_int
    lib.rbrt_host_write_pfm.argtypes = [C.c_char_p, f32p, C.c_uint32, C.c_uint32]
    lib.rbrt_host_environment_nodes.restype = C.c_int
    lib.rbrt_host_environment_nodes.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_double, f32p]
    lib.rbrt_host_environment_fingerprint.restype = C.c_uint64
    lib.rbrt_host_environment_fingerprint.argtypes = [f32p, C.c_uint32, C.c_uint64]
    lib.rbrt_host_scene_free.restype = None
    lib.rbrt_host_scene_free.argtypes = [C.c_void_p]
    lib.rbrt_host_save_image.restype = C.c_int
    lib.rbrt_host_save_image.argtypes = [C.c_char_p, u8p, C.c_uint32, C.c_uint32]
    lib.rbrt_host_write_png.restype = C.c_int
    lib.rbrt_host_write_png.argtypes = [C.c_char_p, u8p, C.c_uint32, C.c_uint32]
    lib.rbrt_host_camera_new.restype = None
    lib.rbrt_host_camera_new.argtypes = [f32p, f32p, f32p, C.c_uint32, C.c_uint32, C.c_float, C.POINTER(Camera)]
    lib.rbrt_host_yaml_dump.restype = C.c_int
    lib.rbrt_host_yaml_dump.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(C.c_void_p)]
    lib.rbrt_host_free.restype = None
    lib.rbrt_host_free.argtypes = [C.c_void_p]
    _host = lib
    return lib


def yaml_dump(text) -> str:
    """Test hook: the tree the C++ host's YAML reader builds from `text` (str or bytes), as JSON (rbrt_host_yaml_dump in
    host/c_api.cpp describes the format). Raises RuntimeError with the reader's message when it refuses the text."""
    lib = load_host()
    raw = text.encode() if isinstance(text, str) else bytes(text)
    out = C.c_void_p()
    if lib.rbrt_host_yaml_dump(raw, len(raw), C.byref(out)) != 0:
        raise RuntimeError(lib.rbrt_host_last_error().decode(errors="replace"))
    try:
        return C.string_at(out).decode(errors="replace")
    finally:
        lib.rbrt_host_free(out)


class HostScene:
    """A scene loaded by the C++ host from a YAML file (src/main.rs:70-80). Quacks like SceneData:
    `.ptr()` gives the rbrt_scene_t*, `.camera` the rbrt_camera_t for the requested image size."""

    def __init__(self, yaml_path, height: int, width: int):
        self._lib = load_host()
        self._h = C.c_void_p()
        rc = self._lib.rbrt_host_scene_load(str(yaml_path).encode(), height, width, C.byref(self._h))
        if rc != 0:
            raise RuntimeError("rbrt_host_scene_load: " + self._lib.rbrt_host_last_error().decode(errors="replace"))
        self.camera = Camera()
        C.memmove(C.byref(self.camera), self._lib.rbrt_host_scene_camera(self._h), C.sizeof(Camera))
        # the camera's thin lens (camera_aperture_mm > 0 in the YAML), else None
        lp = self._lib.rbrt_host_scene_lens(self._h)
        self.lens = None
        if lp:
            self.lens = CameraLens()
            C.memmove(C.byref(self.lens), lp, C.sizeof(CameraLens))
        # the YAML's camera_shutter_travel as a tuple of three floats (what HipScene.set_shutter takes), else None
        tp = self._lib.rbrt_host_scene_shutter_travel(self._h)
        self.shutter_travel = (float(tp[0]), float(tp[1]), float(tp[2])) if tp else None
        self.struct = self._lib.rbrt_host_scene_scene(self._h).contents
        # the spheres' shutter_travel keys as float32 (n_spheres, 3) (what HipScene.set_motion takes), else None
        mp = self._lib.rbrt_host_scene_motion(self._h)
        self.motion = np.ctypeslib.as_array(mp, shape=(self.struct.n_spheres, 3)).astype(np.float32).copy() if mp else None
        # the meshes' shutter_travel keys as float32 (n_meshes, 3) (what HipScene.set_mesh_motion takes), else None
        mm = self._lib.rbrt_host_scene_mesh_motion(self._h)
        self.mesh_motion = np.ctypeslib.as_array(mm, shape=(self.struct.n_meshes, 3)).astype(np.float32).copy() if mm else None
        sp = self._lib.rbrt_host_scene_shading(self._h)  # NULL unless some mesh is smooth
        self.shading = sp.contents if sp else None
        pp = self._lib.rbrt_host_scene_patterns(self._h)  # NULL unless some object carries a checker
        self.patterns = pp.contents if pp else None

    def ptr(self):
        return C.byref(self.struct)

    def shading_ptr(self):
        return None if self.shading is None else C.byref(self.shading)

    def patterns_ptr(self):
        return None if self.patterns is None else C.byref(self.patterns)

    def environment(self):
        """The nodes the host made of the scene's environment_blueprint (rbrt_host_scene_environment): float32
        (N + 1, N + 1, 3), what HipScene.set_environment takes; None when the scene has no environment."""
        n = C.c_uint32()
        p = self._lib.rbrt_host_scene_environment(self._h, C.byref(n))
        if not p:
            return None
        return np.ctypeslib.as_array(p, (n.value + 1, n.value + 1, 3)).copy()

    def mesh_arrays(self, i: int) -> dict:
        m = self.struct.meshes[i]
        out = {k: np.ctypeslib.as_array(getattr(m, k), (m.n_total,)).copy() for k in MeshData.FIELDS}
        out["is_padding"] = np.ctypeslib.as_array(m.is_padding, (m.n_total,)).copy()
        out["bbox_lo"] = np.array(list(m.bbox_lo), np.float32)
        out["bbox_hi"] = np.array(list(m.bbox_hi), np.float32)
        out["n_real"] = m.n_real
        if self.shading is not None and self.shading.meshes[i].n0x:  # a smooth mesh: its corner normals
            mn = self.shading.meshes[i]
            out.update({k: np.ctypeslib.as_array(getattr(mn, k), (m.n_total,)).copy() for k in NORMAL_FIELDS})
        return out

    def close(self):
        if self._h:
            self._lib.rbrt_host_scene_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_pfm(path, any_value: bool = False) -> np.ndarray:
    """The host's PFM reader (rbrt_host_read_pfm): float32 (H, W, 3), top row first. RuntimeError with the reader's
    message for anything it refuses. any_value: texels that are not finite or are negative are read too, bit for bit (what
    write_pfm wrote); without it they are refused, as an environment map's are."""
    lib = load_host()
    read = lib.rbrt_host_read_pfm_any if any_value else lib.rbrt_host_read_pfm
    w, h = C.c_uint32(), C.c_uint32()
    if read(str(path).encode(), C.byref(w), C.byref(h), None) != 0:
        raise RuntimeError(lib.rbrt_host_last_error().decode(errors="replace"))
    out = np.zeros((h.value, w.value, 3), np.float32)
    if read(str(path).encode(), C.byref(w), C.byref(h), fptr(out)) != 0:
        raise RuntimeError(lib.rbrt_host_last_error().decode(errors="replace"))
    return out


def write_pfm(path, rgb: np.ndarray) -> None:
    """The host's PFM writer (rbrt_host_write_pfm; the CLI's --radiance): float32 (H, W, 3), top row first."""
    rgb = np.ascontiguousarray(rgb, np.float32)
    h, w, _ = rgb.shape
    lib = load_host()
    if lib.rbrt_host_write_pfm(str(path).encode(), fptr(rgb), w, h) != 0:
        raise RuntimeError(lib.rbrt_host_last_error().decode(errors="replace"))


def environment_nodes(rgb: np.ndarray, n: int, rotation_deg: float = 0.0, intensity: float = 1.0) -> np.ndarray:
    """The host's conversion of a latitude/longitude image (H, W, 3; top row first) into the (n + 1, n + 1, 3) nodes of
    rbrt_environment_t (rbrt_host_environment_nodes)."""
    lib = load_host()
    rgb = np.ascontiguousarray(rgb, np.float32)
    out = np.zeros((max(int(n), 0) + 1, max(int(n), 0) + 1, 3), np.float32)
    if lib.rbrt_host_environment_nodes(fptr(rgb), rgb.shape[1], rgb.shape[0], int(n), float(rotation_deg), float(intensity), fptr(out)) != 0:
        raise RuntimeError(lib.rbrt_host_last_error().decode(errors="replace"))
    return out


def environment_fingerprint(nodes, h: int) -> int:
    """What an environment adds to the checkpoint fingerprint `h` (rbrt_host_environment_fingerprint); nodes None: no
    environment."""
    lib = load_host()
    if nodes is None:
        return int(lib.rbrt_host_environment_fingerprint(None, 0, h))
    nodes = np.ascontiguousarray(nodes, np.float32)
    return int(lib.rbrt_host_environment_fingerprint(fptr(nodes), nodes.shape[0] - 1, h))


def shutter_fingerprint(travel, h: int) -> int:
    """What a shutter adds to the checkpoint fingerprint `h` (rbrt_host_shutter_fingerprint); travel None: no shutter."""
    lib = load_host()
    if travel is None:
        return int(lib.rbrt_host_shutter_fingerprint(None, h))
    tv = (C.c_float * 3)(*[float(np.float32(v)) for v in travel])
    return int(lib.rbrt_host_shutter_fingerprint(tv, h))


def motion_fingerprint(travels, h: int) -> int:
    """What a motion adds to the checkpoint fingerprint `h` (rbrt_host_motion_fingerprint); travels None: no motion."""
    lib = load_host()
    if travels is None:
        return int(lib.rbrt_host_motion_fingerprint(None, 0, h))
    tv = np.ascontiguousarray(np.asarray(travels, np.float32).reshape(-1, 3))
    return int(lib.rbrt_host_motion_fingerprint(tv.ctypes.data_as(f32p), len(tv), h))


def mesh_motion_fingerprint(travels, h: int) -> int:
    """What a mesh motion adds to the checkpoint fingerprint `h` (rbrt_host_mesh_motion_fingerprint); travels None: none."""
    lib = load_host()
    if travels is None:
        return int(lib.rbrt_host_mesh_motion_fingerprint(None, 0, h))
    tv = np.ascontiguousarray(np.asarray(travels, np.float32).reshape(-1, 3))
    return int(lib.rbrt_host_mesh_motion_fingerprint(tv.ctypes.data_as(f32p), len(tv), h))


def save_image(path, rgb8: np.ndarray) -> None:
    """rbrt::ImageBuffer::save: encoder by file extension (src/main.rs:86)."""
    h, w, _ = rgb8.shape
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    lib = load_host()
    if lib.rbrt_host_save_image(str(path).encode(), rgb8.ctypes.data_as(u8p), w, h) != 0:
        raise RuntimeError(lib.rbrt_host_last_error().decode(errors="replace"))


def write_png(path, rgb8: np.ndarray) -> None:
    rgb8 = np.ascontiguousarray(rgb8, np.uint8)
    h, w, _ = rgb8.shape
    if load_host().rbrt_host_write_png(str(path).encode(), rgb8.ctypes.data_as(u8p), w, h) != 0:
        raise RuntimeError(load_host().rbrt_host_last_error().decode(errors="replace"))
