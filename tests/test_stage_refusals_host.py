"""The refusals of the frame pipeline's image stages, pinned word for word: return code and the full rbrt_hip_last_error() text
of every refusal a stage call can make before it needs a device, which of two refusals wins where one call provokes both, the
sizes the *_workspace_bytes / *_history_bytes functions answer with 0, and the bit patterns of the *_opts_default values and of
rbrt_compare_summary. tests/golden/stage_refusals.json has the expected values; `python tests/test_stage_refusals_host.py
--record` writes that file from the library that is loaded (the test never does).

Host memory stands in for every device pointer, and the test asserts that none of it was written. The message is read after
every call, so a refusal that left rbrt_hip_last_error() with an earlier call's text fails here."""
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))

from rbrt_amd import abi  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "stage_refusals.json"
NAN, INF = float("nan"), float("inf")
FAKE_BYTES = 16384


def camera(width=8, height=4, **kw):
    cam = abi.Camera((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, -0.05), 0.5, 0.5, width, height)
    for name, v in kw.items():
        setattr(cam, name, (C.c_float * 3)(*v) if isinstance(v, tuple) else v)
    return cam


def ref(x):
    return C.byref(x) if x is not None else None


def made(maker, kw):  # a struct by reference, or a null pointer for kw None
    return None if kw is None else C.byref(maker(**kw))


def vp(*addresses):
    return [C.c_void_p(a) for a in addresses]


# ---- the nine entry points: a call that passes every check (it would go on to the device), changed by a row's keywords ---------
def denoise_halves(lib, p, a=1, b=1, wa=1, w=8, h=4, opts=(5, 3, 0.7, 0), rad=1, rgb=1):
    a, b, wa, rad, rgb = (x and p + 256 * i for i, x in enumerate((a, b, wa, rad, rgb)))
    return lib.rbrt_hip_denoise_halves(0, None, *vp(a, b, wa), w, h, ref(opts and abi.DenoiseOpts(*opts)), *vp(rad, rgb))


def guided_opts(levels=5, colour=2.0, normal=0.35, depth=0.05, albedo=0.1, flags=0, reserved=(0, 0)):
    return abi.GuidedOpts(levels, colour, normal, depth, albedo, flags, reserved)


def denoise_guided(lib, p, a=1, b=1, wa=1, albedo=1, normal=1, depth=1, coverage=1, w=8, h=4, opts={}, ws=4096, rad=1, rgb=1):
    a, b, wa, albedo, normal, depth, coverage, rad, rgb = (x and p + 256 * i for i, x in enumerate((a, b, wa, albedo, normal, depth, coverage, rad, rgb)))
    return lib.rbrt_hip_denoise_guided(0, None, *vp(a, b, wa, albedo, normal, depth, coverage), w, h, made(guided_opts, opts),
                                       *vp(ws and p + ws, rad, rgb))


def temporal_opts(max_history=32.0, depth=0.05, normal=0.35, flags=0, reserved=(0, 0, 0, 0)):
    return abi.TemporalOpts(max_history, depth, normal, flags, reserved)


def temporal_accumulate(lib, p, a=1, b=1, normal=1, depth=1, coverage=1, cam={}, prev={}, opts={}, hin=4096, hout=8192, oa=1, ob=1, ol=1):
    a, b, normal, depth, coverage, oa, ob, ol = (x and p + 256 * i for i, x in enumerate((a, b, normal, depth, coverage, oa, ob, ol)))
    return lib.rbrt_hip_temporal_accumulate(0, None, *vp(a, b, normal, depth, coverage), made(camera, cam),
                                            made(camera, prev), made(temporal_opts, opts),
                                            *vp(hin and p + hin, hout and p + hout, oa, ob, ol))


def upsample_camera(lib, p, full={}, factor=2, low=1):
    return lib.rbrt_hip_upsample_camera(made(camera, full), factor, C.cast(C.c_void_p(low and p), C.POINTER(abi.Camera)))


def upsample_opts(factor=2, normal=0.5, depth=0.1, albedo=0.2, flags=0, reserved=(0, 0, 0)):
    return abi.UpsampleOpts(factor, normal, depth, albedo, flags, reserved)


def upsample_halves(lib, p, a=1, b=1, wa=1, albedo=1, normal=1, depth=1, coverage=1, w=8, h=4, opts={}, ws=4096, oa=1, ob=1, owa=1):
    a, b, wa, albedo, normal, depth, coverage, oa, ob, owa = (x and p + 256 * i for i, x in enumerate((a, b, wa, albedo, normal, depth, coverage, oa, ob, owa)))
    return lib.rbrt_hip_upsample_halves(0, None, *vp(a, b, wa, albedo, normal, depth, coverage), w, h, made(upsample_opts, opts),
                                        *vp(ws and p + ws, oa, ob, owa))


def despike_opts(radius=2, rank=2, threshold=4.0, floor=0.01, flags=0, reserved=(0, 0, 0)):
    return abi.DespikeOpts(radius, rank, threshold, floor, flags, reserved)


def despike_halves(lib, p, a=256, b=512, w=8, h=4, opts={}, oa=1024, ob=1280, mask=1536, res=1792):
    return lib.rbrt_hip_despike_halves(0, None, *vp(a and p + a, b and p + b), w, h, made(despike_opts, opts),
                                       *vp(oa and p + oa, ob and p + ob, mask and p + mask, res and p + res))


def compare_images(lib, p, x=256, r=512, w=8, h=4, opts=(0.01, 0, (0, 0)), ws=4096, rel=1024, ssim=1280, res=1536):
    return lib.rbrt_hip_compare_images(0, None, *vp(x and p + x, r and p + r), w, h, ref(opts and abi.CompareOpts(*opts)),
                                       *vp(ws and p + ws, rel and p + rel, ssim and p + ssim, res and p + res))


def tonemap_opts(curve=0, exposure=1.0, key=0.18, key_permille=500, white=0.0, white_permille=990, reserved=(0, 0)):
    return abi.TonemapOpts(curve, exposure, key, key_permille, white, white_permille, reserved)


def tonemap(lib, p, rad=256, n=32, opts={}, ws=4096, out=1024, rgb=1280):
    return lib.rbrt_hip_tonemap(0, None, C.c_void_p(rad and p + rad), n, made(tonemap_opts, opts),
                                *vp(ws and p + ws, out and p + out, rgb and p + rgb))


def glare_opts(threshold=1.0, intensity=0.1, levels=5, spread=1.0, reserved=(0, 0, 0, 0)):
    return abi.GlareOpts(threshold, intensity, levels, spread, reserved)


def glare(lib, p, rad=256, w=8, h=4, opts={}, ws=4096, out=1024, rgb=1280):
    return lib.rbrt_hip_glare(0, None, C.c_void_p(rad and p + rad), w, h, made(glare_opts, opts),
                              *vp(ws and p + ws, out and p + out, rgb and p + rgb))


def guided_staging(lib, p, max_step):
    return lib.rbrt_hip_debug_guided_staging(max_step)


BIG = dict(w=1 << 16, h=1 << 15)  # 2^31 pixels
BIG_CAM = dict(width=1 << 16, height=1 << 15)
O = lambda **kw: dict(opts=kw)  # noqa: E731

# (entry point, row name, keywords). Within an entry point the rows follow the order of its checks; a row named "A + B" provokes
# two refusals that are neighbours in that order and pins which one is reported.
ROWS = []


def rows(fn, *named):
    ROWS.extend((fn, name, kw) for name, kw in named)


rows(denoise_halves,
     ("null a", dict(a=0)), ("null b", dict(b=0)), ("null opts", dict(opts=None)),
     ("reserved", dict(opts=(5, 3, 0.7, 2))), ("window_radius 11", dict(opts=(11, 3, 0.7, 0))), ("patch_radius 5", dict(opts=(5, 5, 0.7, 0))),
     ("strength nan", dict(opts=(5, 3, NAN, 0))), ("strength inf", dict(opts=(5, 3, INF, 0))), ("strength 0", dict(opts=(5, 3, 0.0, 0))),
     ("strength negative", dict(opts=(5, 3, -1.0, 0))),
     ("width 0", dict(w=0)), ("height 0", dict(h=0)), ("2^32 pixels", dict(w=1 << 16, h=1 << 16)), ("2^32 pixels, no output", dict(w=1 << 16, h=1 << 16, rad=0, rgb=0)),
     ("null + reserved", dict(a=0, opts=(5, 3, 0.7, 2))), ("reserved + window_radius", dict(opts=(11, 3, 0.7, 2))),
     ("window_radius + patch_radius", dict(opts=(11, 5, 0.7, 0))), ("patch_radius + strength", dict(opts=(5, 5, NAN, 0))),
     ("strength + width 0", dict(opts=(5, 3, 0.0, 0), w=0)))
# (left out: width 0 + 2^32 pixels -- two tests of the same product)

rows(denoise_guided,
     ("null a", dict(a=0)), ("null b", dict(b=0)),
     ("null opts", dict(opts=None)), ("null albedo", dict(albedo=0)), ("null normal", dict(normal=0)), ("null depth", dict(depth=0)),
     ("null coverage", dict(coverage=0)), ("null workspace", dict(ws=0)),
     ("levels 0", O(levels=0)), ("levels 7", O(levels=7)),
     ("colour 0", O(colour=0.0)), ("normal nan", O(normal=NAN)), ("depth inf", O(depth=INF)), ("albedo negative", O(albedo=-0.1)),
     ("flag 2", O(flags=2)), ("high flag", O(flags=1 << 31)), ("reserved[0]", O(reserved=(1, 0))), ("reserved[1]", O(reserved=(0, 1))),
     ("workspace off by 8", dict(ws=4104)), ("width 0", dict(w=0)), ("height 0", dict(h=0)), ("2^31 pixels", BIG),
     ("null albedo + levels", dict(albedo=0, opts=dict(levels=0))), ("levels + colour", O(levels=0, colour=0.0)), ("albedo + flag", O(albedo=NAN, flags=2)),
     ("flag + reserved", O(flags=2, reserved=(0, 1))), ("reserved + workspace alignment", dict(opts=dict(reserved=(1, 0)), ws=4100)),
     ("workspace alignment + width 0", dict(ws=4100, w=0)))
# (left out: null a + null albedo -- the two statements have the same text; width 0 + 2^31 pixels -- the same product)

rows(temporal_accumulate,
     ("null a", dict(a=0)), ("null b", dict(b=0)), ("null normal", dict(normal=0)), ("null depth", dict(depth=0)), ("null coverage", dict(coverage=0)),
     ("null cam", dict(cam=None)), ("null opts", dict(opts=None)),
     ("history without cam_prev", dict(prev=None)), ("history in == out", dict(hout=4096)),
     ("misaligned history in", dict(hin=4100)), ("misaligned history out", dict(hout=8200)), ("misaligned history out, first frame", dict(hin=0, prev=None, hout=8200)),
     ("width 0", dict(cam=dict(width=0), prev=dict(width=0))), ("height 0", dict(cam=dict(height=0), prev=dict(height=0))),
     ("cam_prev's width", dict(prev=dict(width=9))), ("cam_prev's height", dict(prev=dict(height=5))),
     ("max_history 0.5", O(max_history=0.5)), ("max_history nan", O(max_history=NAN)), ("max_history inf", O(max_history=INF)),
     ("depth negative", O(depth=-0.5)), ("depth nan", O(depth=NAN)), ("normal inf", O(normal=INF)),
     ("flag", O(flags=1)), ("reserved[0]", O(reserved=(1, 0, 0, 0))), ("reserved[3]", O(reserved=(0, 0, 0, 1))),
     ("cam mm_per_pix_hor 0", dict(cam=dict(mm_per_pix_hor=0.0))), ("cam mm_per_pix_vert nan", dict(cam=dict(mm_per_pix_vert=NAN))),
     ("cam mm_per_pix_hor inf", dict(cam=dict(mm_per_pix_hor=INF))), ("cam mm_per_pix_vert negative", dict(cam=dict(mm_per_pix_vert=-1.0))),
     ("cam_prev mm_per_pix_hor 0", dict(prev=dict(mm_per_pix_hor=0.0))), ("cam_prev mm_per_pix_vert inf", dict(prev=dict(mm_per_pix_vert=INF))),
     ("degenerate cam_prev: right 0", dict(prev=dict(right=(0.0, 0.0, 0.0)))), ("degenerate cam_prev: right parallel to up", dict(prev=dict(right=(0.0, 2.0, 0.0)))),
     ("degenerate cam_prev: image plane through the position", dict(prev=dict(img_center_point=(0.0, 0.0, 0.0)))),
     ("degenerate cam_prev: nan", dict(prev=dict(up=(NAN, 1.0, 0.0)))),
     ("2^31 pixels", dict(cam=BIG_CAM, prev=BIG_CAM)), ("2^31 pixels, first frame", dict(cam=BIG_CAM, prev=None, hin=0)),
     ("null + history without cam_prev", dict(a=0, prev=None)), ("history without cam_prev + in == out", dict(prev=None, hout=4096)),
     ("in == out + misaligned", dict(hin=4100, hout=4100)), ("misaligned + width 0", dict(hin=4100, cam=dict(width=0))),
     ("width 0 + cam_prev's size", dict(cam=dict(width=0))), ("cam_prev's size + max_history", dict(prev=dict(width=9), opts=dict(max_history=0.0))),
     ("max_history + depth", O(max_history=0.0, depth=-1.0)), ("normal + flag", O(normal=NAN, flags=1)), ("flag + reserved", O(flags=1, reserved=(0, 1, 0, 0))),
     ("reserved + cam mm_per_pix", dict(opts=dict(reserved=(0, 0, 1, 0)), cam=dict(mm_per_pix_hor=0.0))),
     ("cam mm_per_pix + cam_prev mm_per_pix", dict(cam=dict(mm_per_pix_hor=0.0), prev=dict(mm_per_pix_hor=0.0))),
     ("cam_prev mm_per_pix + degenerate", dict(prev=dict(mm_per_pix_hor=0.0, right=(0.0, 0.0, 0.0)))),
     ("degenerate + 2^31 pixels", dict(cam=BIG_CAM, prev=dict(right=(0.0, 0.0, 0.0), **BIG_CAM))))

rows(upsample_camera,
     ("null full", dict(full=None)), ("null low", dict(low=0)), ("factor 0", dict(factor=0)), ("factor 5", dict(factor=5)),
     ("width 0", dict(full=dict(width=0))), ("height 0", dict(full=dict(height=0))),
     ("mm_per_pix_hor nan", dict(full=dict(mm_per_pix_hor=NAN))), ("mm_per_pix_vert inf", dict(full=dict(mm_per_pix_vert=INF))),
     ("null + factor", dict(low=0, factor=0)), ("factor + width 0", dict(factor=5, full=dict(width=0))),
     ("height 0 + mm_per_pix", dict(full=dict(height=0, mm_per_pix_hor=NAN))))

rows(upsample_halves,
     ("null a", dict(a=0)), ("null b", dict(b=0)), ("null albedo", dict(albedo=0)), ("null normal", dict(normal=0)), ("null depth", dict(depth=0)),
     ("null coverage", dict(coverage=0)), ("null opts", dict(opts=None)), ("null workspace", dict(ws=0)),
     ("width 0", dict(w=0)), ("height 0", dict(h=0)), ("factor 0", O(factor=0)), ("factor 5", O(factor=5)),
     ("normal 0", O(normal=0.0)), ("depth nan", O(depth=NAN)), ("albedo inf", O(albedo=INF)), ("albedo negative", O(albedo=-0.2)),
     ("flag 2", O(flags=2)), ("reserved[0]", O(reserved=(1, 0, 0))), ("reserved[2]", O(reserved=(0, 0, 1))),
     ("workspace off by 4", dict(ws=4100)), ("2^31 pixels", BIG),
     ("null + width 0", dict(a=0, w=0)), ("width 0 + factor", dict(w=0, opts=dict(factor=0))), ("factor + normal", O(factor=5, normal=0.0)),
     ("albedo + flag", O(albedo=NAN, flags=2)), ("flag + reserved", O(flags=2, reserved=(0, 1, 0))),
     ("reserved + workspace alignment", dict(opts=dict(reserved=(0, 0, 1)), ws=4100)), ("workspace alignment + 2^31 pixels", dict(ws=4100, **BIG)))

rows(despike_halves,
     ("null a", dict(a=0)), ("null b", dict(b=0)), ("null opts", dict(opts=None)), ("width 0", dict(w=0)), ("height 0", dict(h=0)),
     ("radius 0", O(radius=0)), ("radius 3", O(radius=3)), ("rank 0", O(rank=0)), ("rank 5", O(rank=5)),
     ("threshold 0.5", O(threshold=0.5)), ("threshold nan", O(threshold=NAN)), ("threshold inf", O(threshold=INF)),
     ("floor negative", O(floor=-0.01)), ("floor nan", O(floor=NAN)), ("floor inf", O(floor=INF)),
     ("flag", O(flags=1)), ("reserved[0]", O(reserved=(1, 0, 0))), ("reserved[2]", O(reserved=(0, 0, 1))),
     ("out_a is a", dict(oa=256)), ("out_b is a", dict(ob=256)), ("mask is b", dict(mask=512)), ("result is b", dict(res=512)),
     ("2^31 pixels", BIG), ("2^31 pixels, no output", dict(oa=0, ob=0, mask=0, res=0, **BIG)),
     ("null + width 0", dict(a=0, w=0)), ("height 0 + radius", dict(h=0, opts=dict(radius=0))), ("radius + rank", O(radius=3, rank=0)),
     ("rank + threshold", O(rank=5, threshold=NAN)), ("threshold + floor", O(threshold=0.5, floor=-1.0)), ("floor + flag", O(floor=NAN, flags=1)),
     ("flag + reserved", O(flags=1, reserved=(0, 1, 0))), ("reserved + output is input", dict(opts=dict(reserved=(0, 1, 0)), oa=256)),
     ("output is input + 2^31 pixels", dict(mask=256, **BIG)))

rows(compare_images,
     ("null x", dict(x=0)), ("null ref", dict(r=0)), ("null opts", dict(opts=None)),
     ("result without workspace", dict(ws=0)), ("result alone without workspace", dict(ws=0, rel=0, ssim=0)),
     ("workspace off by 4", dict(ws=4100)), ("result off by 4", dict(res=1540)), ("width 0", dict(w=0)), ("height 0", dict(h=0)),
     ("epsilon 0", dict(opts=(0.0, 0, (0, 0)))), ("epsilon -0", dict(opts=(-0.0, 0, (0, 0)))), ("epsilon negative", dict(opts=(-0.01, 0, (0, 0)))),
     ("epsilon nan", dict(opts=(NAN, 0, (0, 0)))), ("epsilon inf", dict(opts=(INF, 0, (0, 0)))),
     ("flag", dict(opts=(0.01, 1, (0, 0)))), ("reserved[0]", dict(opts=(0.01, 0, (1, 0)))), ("reserved[1]", dict(opts=(0.01, 0, (0, 7)))),
     ("rel is x", dict(rel=256)), ("ssim is ref", dict(ssim=512)), ("result is x", dict(res=256)), ("workspace is ref", dict(ws=512)),
     ("ssim is rel", dict(ssim=1024)), ("result is ssim", dict(res=1280)), ("workspace is the result", dict(ws=1536)),
     ("workspace is x, no result", dict(ws=256, res=0, w=1 << 16, h=1 << 15)),  # (not an output then: the size is what is refused)
     ("2^31 pixels", BIG), ("2^31 pixels, no output", dict(ws=0, rel=0, ssim=0, res=0, **BIG)),
     ("null + result without workspace", dict(x=0, ws=0)), ("result without workspace + alignment", dict(ws=0, res=1540)),
     ("alignment + width 0", dict(ws=4100, w=0)), ("height 0 + epsilon", dict(h=0, opts=(0.0, 0, (0, 0)))), ("epsilon + flag", dict(opts=(NAN, 1, (0, 0)))),
     ("flag + reserved", dict(opts=(0.01, 1, (0, 1)))), ("reserved + output is input", dict(opts=(0.01, 0, (1, 0)), rel=256)),
     ("rel is x + ssim is rel", dict(rel=256, ssim=256)), ("ssim is rel + result is x", dict(ssim=1024, res=256)),
     ("another output + 2^31 pixels", dict(ssim=1024, **BIG)))

rows(tonemap,
     ("null radiance", dict(rad=0)), ("null opts", dict(opts=None)), ("n_pixels 0", dict(n=0)), ("curve 3", O(curve=3)),
     ("reserved[0]", O(reserved=(1, 0))), ("reserved[1]", O(reserved=(0, 1))),
     ("exposure nan", O(exposure=NAN)), ("key inf", O(key=INF)), ("white -inf", O(white=-INF)),
     ("exposure negative", O(exposure=-1.0)), ("white negative", O(white=-1.0)),
     ("key 0 with automatic exposure", O(exposure=0.0, key=0.0)), ("key negative with exposure -0", O(exposure=-0.0, key=-1.0)),
     ("key_permille 1001", O(key_permille=1001)), ("white_permille 1001", O(white=1.0, white_permille=1001)),
     ("automatic white without workspace", dict(ws=0)), ("automatic exposure without workspace", dict(ws=0, opts=dict(exposure=0.0, white=1.0))),
     ("workspace off by 8", dict(ws=4104)), ("workspace off by 8, nothing automatic", dict(ws=4104, opts=dict(white=1.0))),
     ("2^32 pixels", dict(n=1 << 32)),
     ("null + n_pixels 0", dict(rad=0, n=0)), ("n_pixels 0 + curve", dict(n=0, opts=dict(curve=3))), ("curve + reserved", O(curve=3, reserved=(1, 0))),
     ("reserved + not finite", O(reserved=(0, 1), key=NAN)), ("not finite + negative", O(exposure=NAN, white=-1.0)),
     ("negative + key", O(exposure=0.0, key=0.0, white=-1.0)), ("key + permille", O(exposure=0.0, key=0.0, key_permille=1001)),
     ("permille + no workspace", dict(ws=0, opts=dict(white_permille=1001))), ("workspace alignment + 2^32 pixels", dict(ws=4104, n=1 << 32)))
# (left out: no workspace + workspace alignment -- a null workspace is aligned)

rows(glare,
     ("null radiance", dict(rad=0)), ("null opts", dict(opts=None)), ("null workspace", dict(ws=0)), ("width 0", dict(w=0)), ("height 0", dict(h=0)),
     ("levels 0", O(levels=0)), ("levels 9", O(levels=9)), ("reserved[0]", O(reserved=(1, 0, 0, 0))), ("reserved[3]", O(reserved=(0, 0, 0, 1))),
     ("threshold nan", O(threshold=NAN)), ("intensity inf", O(intensity=INF)), ("spread -inf", O(spread=-INF)),
     ("threshold negative", O(threshold=-1.0)), ("intensity 0", O(intensity=0.0)), ("intensity negative", O(intensity=-0.1)), ("intensity 1.5", O(intensity=1.5)),
     ("spread negative", O(spread=-1.0)), ("workspace off by 4", dict(ws=4100)), ("2^31 pixels", BIG),
     ("null + width 0", dict(rad=0, w=0)), ("height 0 + levels", dict(h=0, opts=dict(levels=0))), ("levels + reserved", O(levels=9, reserved=(0, 1, 0, 0))),
     ("reserved + not finite", O(reserved=(0, 0, 1, 0), spread=NAN)), ("not finite + threshold", O(intensity=NAN, threshold=-1.0)),
     ("threshold + intensity", O(threshold=-1.0, intensity=0.0)), ("intensity + spread", O(intensity=1.5, spread=-1.0)),
     ("spread + workspace alignment", dict(opts=dict(spread=-1.0), ws=4100)), ("workspace alignment + 2^31 pixels", dict(ws=4100, **BIG)))

rows(guided_staging, ("max_step -2", dict(max_step=-2)), ("max_step 5", dict(max_step=5)))


def refusals(lib):
    """{"entry: row": [return code, message]}, and the host memory that stood in for the device pointers."""
    fake = (C.c_uint8 * FAKE_BYTES)()
    p = (C.addressof(fake) + 63) & ~63
    got = {}
    for fn, name, kw in ROWS:
        rc = fn(lib, p, **kw)
        key = f"{fn.__name__}: {name}"
        assert key not in got, key
        got[key] = [rc, lib.rbrt_hip_last_error().decode()]
    return got, fake


# ---- sizes ----------------------------------------------------------------------------------------------------------------------
SIZES = [(w, h) for w, h in ((0, 5), (7, 0), (1 << 16, 1 << 15), (1 << 31, 1), (7, 5))]


def sizes(lib):
    got = {}
    for w, h in SIZES:
        for name in ("guided_workspace", "temporal_history", "compare_workspace"):
            got[f"{name}_bytes({w}, {h})"] = int(getattr(lib, f"rbrt_hip_{name}_bytes")(w, h))
        got[f"upsample_workspace_bytes({w}, {h}, 2)"] = int(lib.rbrt_hip_upsample_workspace_bytes(w, h, 2))
        got[f"glare_workspace_bytes({w}, {h}, 3)"] = int(lib.rbrt_hip_glare_workspace_bytes(w, h, 3))
    for f in (0, 1, 3, 4, 5):
        got[f"upsample_workspace_bytes(7, 5, {f})"] = int(lib.rbrt_hip_upsample_workspace_bytes(7, 5, f))
    for l in (0, 1, 8, 9):
        got[f"glare_workspace_bytes(7, 5, {l})"] = int(lib.rbrt_hip_glare_workspace_bytes(7, 5, l))
    return got


# ---- numeric outputs, as bit patterns ---------------------------------------------------------------------------------------------
def words(struct, kind=C.c_uint32):
    n = C.sizeof(struct) // C.sizeof(kind)
    return [f"{v:0{2 * C.sizeof(kind)}x}" for v in (kind * n).from_buffer_copy(struct)]


def numbers(lib):
    got = {}
    for name in ("Denoise", "Guided", "Temporal", "Upsample", "Despike", "Compare", "Tonemap", "Glare"):
        o = getattr(abi, name + "Opts")()
        C.memset(C.byref(o), 0xA5, C.sizeof(o))
        getattr(lib, f"rbrt_{name.lower()}_opts_default")(C.byref(o))
        got[f"rbrt_{name.lower()}_opts_default"] = words(o)
    # (peak^2 / mse = 6.25 / 0.0625 = 100 exactly: the one logarithm is of a power of ten)
    result = abi.CompareResult(0.75, 1.5, 3.0, 17.5, 0.5, 4, 31, (0, 0, 0, 0, 0))
    for name, r in (("usable 4", result), ("usable 0", abi.CompareResult(0.75, 1.5, 3.0, 17.5, 0.5, 0, 35, (0, 0, 0, 0, 0))), ("null result", None)):
        out = abi.CompareSummary()
        C.memset(C.byref(out), 0xA5, C.sizeof(out))
        lib.rbrt_compare_summary(ref(r), 7, 5, 2.5, C.byref(out))
        got[f"rbrt_compare_summary, {name}"] = words(out, C.c_uint64)
    low, full = abi.Camera(), camera(7, 5, right=(0.5, 0.25, 0.0), up=(0.0, 0.75, 0.125), mm_per_pix_hor=0.3, mm_per_pix_vert=0.7)
    for f in (1, 2, 3, 4):
        assert lib.rbrt_hip_upsample_camera(C.byref(full), f, C.byref(low)) == abi.RBRT_OK
        got[f"rbrt_hip_upsample_camera, factor {f}"] = words(low)
    return got


def everything(lib):
    r, fake = refusals(lib)
    return {"refusals": r, "sizes": sizes(lib), "numbers": numbers(lib)}, fake


def test_every_stage_refusal_size_and_default_is_what_was_recorded():
    expected = json.loads(GOLDEN.read_text())
    got, fake = everything(abi.load_hip())
    assert not any(fake)  # a refused call wrote nothing
    for part in ("refusals", "sizes", "numbers"):
        assert got[part].keys() == expected[part].keys(), part
        for key, value in expected[part].items():
            assert got[part][key] == value, (key, got[part][key], value)
    for key, (rc, msg) in expected["refusals"].items():  # (what was recorded are refusals, each with a text)
        assert rc in (abi.RBRT_ERR_INVALID_ARG, abi.RBRT_ERR_UNSUPPORTED) and msg, key


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: test_stage_refusals_host.py --record")
    recorded, memory = everything(abi.load_hip())
    assert not any(memory)
    for row, (code, text) in recorded["refusals"].items():
        assert code in (abi.RBRT_ERR_INVALID_ARG, abi.RBRT_ERR_UNSUPPORTED) and text, (row, code, text)
    GOLDEN.write_text(json.dumps(recorded, indent=1) + "\n")
    print(f"recorded {len(recorded['refusals'])} refusals, {len(recorded['sizes'])} sizes, {len(recorded['numbers'])} bit patterns in {GOLDEN}")
