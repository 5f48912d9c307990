"""The animation's three entry points at the boundary, without a GPU: the C header declares them with the arguments the ctypes
prototypes pass (a C program that assigns each to a typed function pointer compiles without a warning), the symbols are the
capability -- no flag bit, no struct, ABI version 2 -- and the arguments the library rejects before it touches a device."""
import ctypes as C
import subprocess
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
NEW = ("rbrt_hip_scene_set_motion_phase", "rbrt_hip_render_features_motion", "rbrt_hip_temporal_accumulate_moving")

POINTERS = """
#include <stdio.h>
#include "rbrt_hip.h"
int (*phase)(rbrt_hip_scene_t*, float) = rbrt_hip_scene_set_motion_phase;
int (*features)(rbrt_hip_scene_t*, const rbrt_camera_t*, const rbrt_render_opts_t*, const rbrt_feature_opts_t*, void*, float*, float*, float*,
                float*, int32_t*, float*) = rbrt_hip_render_features_motion;
int (*moving)(int, void*, const float*, const float*, const float*, const float*, const float*, const float*, float, const rbrt_camera_t*,
              const rbrt_camera_t*, const rbrt_temporal_opts_t*, const void*, void*, float*, float*, float*) = rbrt_hip_temporal_accumulate_moving;
/* the calls they extend, argument for argument */
int (*features_old)(rbrt_hip_scene_t*, const rbrt_camera_t*, const rbrt_render_opts_t*, const rbrt_feature_opts_t*, void*, float*, float*, float*,
                    float*, int32_t*) = rbrt_hip_render_features;
int (*plain)(int, void*, const float*, const float*, const float*, const float*, const float*, const rbrt_camera_t*, const rbrt_camera_t*,
             const rbrt_temporal_opts_t*, const void*, void*, float*, float*, float*) = rbrt_hip_temporal_accumulate;
int main(void) { printf("abi %d\\n", RBRT_ABI_VERSION); return 0; }
"""


def test_the_header_declares_what_the_prototypes_pass(tmp_path):
    (tmp_path / "anim.c").write_text(POINTERS)
    r = subprocess.run(["gcc", "-Wall", "-Wextra", "-Werror", "-c", "-I", str(ROOT / "include"), "-o", str(tmp_path / "anim.o"), str(tmp_path / "anim.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    res, args = abi.HIP_SYMBOLS["rbrt_hip_scene_set_motion_phase"]
    assert res is C.c_int and args == [C.c_void_p, C.c_float]
    res, args = abi.HIP_SYMBOLS["rbrt_hip_render_features_motion"]
    old = abi.HIP_SYMBOLS["rbrt_hip_render_features"][1]
    assert res is C.c_int and args == old + [C.c_void_p]  # the old call's arguments, then d_motion
    res, args = abi.HIP_SYMBOLS["rbrt_hip_temporal_accumulate_moving"]
    old = abi.HIP_SYMBOLS["rbrt_hip_temporal_accumulate"][1]
    assert res is C.c_int and args == old[:7] + [C.c_void_p, C.c_float] + old[7:]  # d_motion and phase_step behind d_coverage
    assert C.sizeof(abi.TemporalOpts) == 32 and abi.load_hip().rbrt_hip_temporal_history_bytes(3, 5) == 3 * 5 * 48  # (no struct or layout changed)


def test_the_symbols_are_the_capability_and_no_flag_bit_was_added():
    import rbrt_amd
    lib = abi.load_hip()
    for name in NEW:
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name), name
    assert rbrt_amd.supported_flags() == 7
    assert lib.rbrt_hip_abi_version() == 2
    assert hasattr(rbrt_amd.HipScene, "set_motion_phase")


def test_null_and_non_finite_arguments_are_rejected_before_the_device():
    lib = abi.load_hip()
    assert lib.rbrt_hip_scene_set_motion_phase(None, C.c_float(1.0)) == abi.RBRT_ERR_INVALID_ARG
    assert b"null scene" in lib.rbrt_hip_last_error()
    cam, opts, fo, to = abi.Camera(), abi.default_opts(), abi.FeatureOpts(), abi.TemporalOpts()
    assert lib.rbrt_hip_render_features_motion(None, C.byref(cam), C.byref(opts), C.byref(fo), None, None, None, None, None, None, None) == abi.RBRT_ERR_INVALID_ARG
    # the plain call's refusals come first (here: no inputs at all), with a motion buffer or without
    for motion in (None, C.c_void_p(64)):
        assert lib.rbrt_hip_temporal_accumulate_moving(0, None, None, None, None, None, None, motion, C.c_float(1.0), C.byref(cam), None, C.byref(to),
                                                       None, None, None, None, None) == abi.RBRT_ERR_INVALID_ARG
        assert b"null argument" in lib.rbrt_hip_last_error()


def test_the_rust_binding_and_the_guide_name_them():
    rs = (ROOT / "integration" / "rust" / "hip_ffi.rs").read_text()
    guide = (ROOT / "INTEGRATION.md").read_text()
    for name in NEW:
        assert f"pub fn {name}(" in rs and name in guide, name
