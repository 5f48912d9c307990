"""The short-path stage's two debug entry points (include/rbrt_hip_debug.h), without a GPU: they are declared in the header
and in the symbol table, the ABI version stays 2, and bad arguments come back as codes before a device is touched."""
import ctypes as C
import re
from pathlib import Path

from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("rbrt_hip_scene_set_short_paths", "rbrt_hip_debug_short_masks")


def test_entry_points_are_declared_and_exported():
    header = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
    lib = abi.load_hip()
    for name in NAMES:
        assert name in abi.DEBUG_SYMBOLS and name not in abi.HIP_SYMBOLS
        assert re.search(rf"\bint {name}\(rbrt_hip_scene_t\* scene,", header), name
        assert getattr(lib, name) is not None
    assert lib.rbrt_hip_abi_version() == 2


def test_refusals_without_a_gpu():
    lib = abi.load_hip()
    n = C.c_size_t(7)
    words = (C.c_uint64 * 4)()
    assert lib.rbrt_hip_scene_set_short_paths(None, 1) == abi.RBRT_ERR_INVALID_ARG  # (before the mode is looked at)
    assert b"null" in lib.rbrt_hip_last_error()
    assert lib.rbrt_hip_debug_short_masks(None, words, 4, C.byref(n)) == abi.RBRT_ERR_INVALID_ARG
    assert b"null" in lib.rbrt_hip_last_error()
    assert n.value == 7  # (nothing was written)
