"""rbrt_motion_t and rbrt_hip_scene_set_motion at the boundary, without a GPU: the struct's layout against the C header, the
symbol as the capability, and the arguments the library rejects before it touches a device."""
import ctypes as C
import subprocess
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent


def test_motion_layout_matches_the_c_header(tmp_path):
    names = [f for f, _ in abi.Motion._fields_]
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){'
           'printf("size %zu\\n", sizeof(rbrt_motion_t));'
           + "".join(f'printf("{f} %zu\\n", offsetof(rbrt_motion_t, {f}));' for f in names)
           + 'printf("abi %d\\n", RBRT_ABI_VERSION); return 0;}')
    (tmp_path / "motion.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "motion"), str(tmp_path / "motion.c")], check=True)
    out = subprocess.run([str(tmp_path / "motion")], check=True, capture_output=True, text=True).stdout
    got = dict(line.split() for line in out.strip().splitlines())
    assert names == ["n_spheres", "reserved", "travel"]
    assert int(got["size"]) == C.sizeof(abi.Motion) == 16
    for f in names:
        assert int(got[f]) == getattr(abi.Motion, f).offset, f
    assert got["abi"] == "2"


def test_the_symbol_is_the_capability_and_no_flag_bit_was_added():
    import rbrt_amd
    assert "rbrt_hip_scene_set_motion" in abi.HIP_SYMBOLS
    assert hasattr(abi.load_hip(), "rbrt_hip_scene_set_motion")
    assert rbrt_amd.supported_flags() == 7
    assert abi.load_hip().rbrt_hip_abi_version() == 2


def test_a_null_scene_is_rejected_before_the_device():
    lib = abi.load_hip()
    mo = abi.Motion()
    assert lib.rbrt_hip_scene_set_motion(None, C.byref(mo)) == abi.RBRT_ERR_INVALID_ARG
    assert b"null scene" in lib.rbrt_hip_last_error()
    assert lib.rbrt_hip_scene_set_motion(None, None) == abi.RBRT_ERR_INVALID_ARG


def test_the_rust_binding_and_the_guide_name_it():
    rs = (ROOT / "integration" / "rust" / "hip_ffi.rs").read_text()
    assert "pub struct RbrtMotion" in rs and "pub fn rbrt_hip_scene_set_motion(scene: *mut c_void, motion: *const RbrtMotion) -> c_int;" in rs
    assert "rbrt_hip_scene_set_motion" in (ROOT / "INTEGRATION.md").read_text()
