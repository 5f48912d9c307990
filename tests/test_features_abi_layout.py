"""The feature buffers' additions to the C ABI, without a GPU: rbrt_feature_opts_t has the layout a C compiler gives
include/rbrt_hip.h in its ctypes mirror (rbrt_amd/abi.py), the entry points are in the symbol table, the ABI version stays 2,
and every RBRT_ERR_INVALID_ARG row of rbrt_hip_render_features comes back before a device is touched."""
import ctypes as C
import subprocess
from pathlib import Path

import rbrt_amd
from rbrt_amd import abi

ROOT = Path(__file__).resolve().parent.parent


def test_feature_opts_layout_matches_the_c_header(tmp_path):
    structs = {"rbrt_feature_opts_t": abi.FeatureOpts}
    lines = []
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rbrt_hip.h"\nint main(void){' + "".join(lines) + "return 0;}"
    (tmp_path / "ft.c").write_text(src)
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(tmp_path / "ft"), str(tmp_path / "ft.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "ft")], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, cls in structs.items():
        assert int(got[cname]) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert int(got[f"{cname}.{f}"]) == getattr(cls, f).offset, f"{cname}.{f}"
    assert C.sizeof(abi.FeatureOpts) == 16 and abi.FeatureOpts.reserved.offset == 4
    assert [f for f, _ in abi.FeatureOpts._fields_] == ["samples", "reserved"]


def test_symbols_version_and_defaults():
    lib = abi.load_hip()
    assert lib.rbrt_hip_abi_version() == 2
    for name in ("rbrt_hip_render_features", "rbrt_feature_opts_default"):
        assert name in abi.HIP_SYMBOLS and hasattr(lib, name)
    assert len(abi.HIP_SYMBOLS["rbrt_hip_render_features"][1]) == 10
    d = abi.FeatureOpts(9, (9, 9, 9))
    lib.rbrt_feature_opts_default(C.byref(d))
    assert (d.samples, list(d.reserved)) == (4, [0, 0, 0])
    lib.rbrt_feature_opts_default(None)  # (a NULL is ignored, as by the other *_default calls)
    f = rbrt_amd.feature_opts(7)
    assert (f.samples, list(f.reserved)) == (7, [0, 0, 0]) and rbrt_amd.feature_opts().samples == 4
    header = (ROOT / "include" / "rbrt_hip.h").read_text()
    assert "int rbrt_hip_render_features(" in header and "#define RBRT_ABI_VERSION 2" in header
    assert hasattr(rbrt_amd.HipScene, "render_features")


def call(lib, scene, cam, opts, feat, out):
    ref = lambda x: C.byref(x) if x is not None else None  # noqa: E731
    return lib.rbrt_hip_render_features(C.c_void_p(scene), ref(cam), ref(opts), ref(feat), None, C.c_void_p(out), C.c_void_p(out),
                                        C.c_void_p(out), C.c_void_p(out), C.c_void_p(out))


def test_every_invalid_argument_is_refused_before_a_device_is_touched():
    """Host memory stands in for the scene handle and the outputs: a refused call reads neither. The last row shows that the
    checks are what refuses: the same call with valid arguments but no output returns RBRT_OK, still without a device."""
    lib = abi.load_hip()
    fake = (C.c_uint8 * 4096)()  # never dereferenced by a refused call
    s, out = C.addressof(fake), C.addressof(fake) + 1024
    cam = abi.Camera()
    cam.img_width_pix, cam.img_height_pix = 16, 8
    O, T = abi.default_opts, rbrt_amd.feature_opts
    nan, inf = float("nan"), float("inf")

    def lens(**kw):
        L = abi.camera_lens(cam, kw.pop("lens_u", (0.1, 0.0, 0.0)), kw.pop("lens_v", (0.0, 0.1, 0.0)), kw.pop("focus_scale", 300.0))
        L.reserved = kw.pop("reserved", 0)
        return L

    def no_pixels(w, h):
        c = abi.Camera()
        c.img_width_pix, c.img_height_pix = w, h
        return c

    rows = {
        "null scene": (0, cam, O(), T()),
        "null cam": (s, None, O(), T()),
        "null opts": (s, cam, None, T()),
        "null features": (s, cam, O(), None),
        "samples 0": (s, cam, O(), T(0)),
        "samples 65537": (s, cam, O(), T(65537)),
        "reserved[0]": (s, cam, O(), T(4, (1, 0, 0))),
        "reserved[1]": (s, cam, O(), T(4, (0, 1, 0))),
        "reserved[2]": (s, cam, O(), T(4, (0, 0, 1))),
        "collect stats": (s, cam, O(flags=abi.FLAG_COLLECT_STATS), T()),
        "width 0": (s, no_pixels(0, 8), O(), T()),
        "height 0": (s, no_pixels(8, 0), O(), T()),
        "tile_rank >= tile_world": (s, cam, O(tile_rank=2, tile_world=2), T()),
        "tile_rank 1 of one": (s, cam, O(tile_rank=1), T()),
        "lens_u nan": (s, lens(lens_u=(nan, 0, 0)).cam, O(flags=abi.FLAG_THIN_LENS), T()),
        "lens_v inf": (s, lens(lens_v=(0, inf, 0)).cam, O(flags=abi.FLAG_THIN_LENS), T()),
        "focus_scale 0": (s, lens(focus_scale=0.0).cam, O(flags=abi.FLAG_THIN_LENS), T()),
        "focus_scale nan": (s, lens(focus_scale=nan).cam, O(flags=abi.FLAG_THIN_LENS), T()),
        "lens reserved": (s, lens(reserved=1).cam, O(flags=abi.FLAG_THIN_LENS), T()),
    }
    keep = []
    for name, (scene, c, o, f) in rows.items():
        keep.append((c, o, f))
        rc = call(lib, scene, c, o, f, out)
        assert rc == abi.RBRT_ERR_INVALID_ARG, (name, rc, lib.rbrt_hip_last_error())
        assert lib.rbrt_hip_last_error(), name
    assert not any(fake)
    # tile_world > 1 and an image of 2^32 pixels are UNSUPPORTED, not invalid
    assert call(lib, s, cam, O(tile_rank=1, tile_world=2), T(), out) == abi.RBRT_ERR_UNSUPPORTED
    assert call(lib, s, no_pixels(1 << 16, 1 << 16), O(), T(), out) == abi.RBRT_ERR_UNSUPPORTED
    # the largest sample count passes the checks; with no output asked for, the call is done before it needs a device
    assert call(lib, s, cam, O(), T(65536), 0) == abi.RBRT_OK
    assert call(lib, s, cam, O(spp=0, max_depth=1000), T(1), 0) == abi.RBRT_OK  # (spp and max_depth are not read)
    assert not any(fake)
