"""The trace kernel's two product builds (include/rbrt_hip_debug.h rbrt_hip_scene_last_trace_build): the general one, and
the PLAIN one with the default lab knobs and the plain scene -- spheres and one mesh -- built in as constants.

Selection: the debug query says which build a handle's last trace launch ran; the PLAIN build must run for the plain scene
at the default knobs and for nothing else. Same bits: every case is rendered once as the library chooses (auto) and once
with the general build forced (RBRT_TRACE_BUILD=general, a lab control read at scene creation); the fp32 radiance and the
RGB8 image must be equal byte for byte, and the first case must also be the committed golden's, which pins both builds to
the oracle."""
from __future__ import annotations

import ctypes as C
import hashlib
from pathlib import Path

import numpy as np
import pytest

import scenes
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "mesh2000_160x120x4_seed2.npz"
T = scenes.T


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _set_build(monkeypatch, build, env=None):
    """The environment of the next scene creation: the build control and the case's own lab knobs."""
    for k in ("RBRT_TRACE_BUILD", "RBRT_Y_LOW", "RBRT_HELPERS"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RBRT_HIP_LAB", "1")
    if build is not None:
        monkeypatch.setenv("RBRT_TRACE_BUILD", build)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)


def _frames(hip, torch, sc, cams, opts, *, pipeline=None, check_helpers=False, count=False):
    """Renders one frame per (camera, options) on a fresh handle, back to back. Returns the frames' bytes (radiance, then
    RGB8, as uint8 arrays: a packed rank's buffer keeps its NaN filler, which compares as bytes), the build the last launch
    ran, and the counters of a counting launch of the first frame (count=True; run last)."""
    out = []
    with hip.HipScene(sc) as hs:
        hs.refine_wait(60.0)  # (one tree for the handle's whole life: the counters below belong to the frames above)
        assert hs.last_trace_build() == "none"
        if pipeline is not None:
            hs.set_pipeline(pipeline)
        if check_helpers:
            hs.set_timing(True)
        bufs = []
        for cam, o in zip(cams, opts):
            n = hip.packed_pixels(cam.img_width_pix, cam.img_height_pix, o.tile_rank, o.tile_world) if o.tile_world > 1 \
                else cam.img_width_pix * cam.img_height_pix
            rad = torch.full((n * 3,), float("nan"), dtype=torch.float32, device="cuda")
            rgb = torch.full((n * 3,), 7, dtype=torch.uint8, device="cuda")
            hs.render_device(cam, o, rad.data_ptr(), rgb.data_ptr())
            bufs.append((rad, rgb))
        torch.cuda.synchronize()
        build = hs.last_trace_build()
        if check_helpers:
            assert hs.helper_launches() > 0  # (RBRT_HELPERS=2: a helper launch with every overlapped launch)
        for rad, rgb in bufs:
            out.append((rad.cpu().numpy().view(np.uint8).copy(), rgb.cpu().numpy().copy()))
        counters = None
        if count:
            o = opts[0]
            oc = abi.default_opts(spp=o.spp, seed=o.seed, max_depth=o.max_depth, flags=o.flags | abi.FLAG_COLLECT_STATS)
            rad, rgb = bufs[0]
            rad.fill_(float("nan"))
            hs.render_device(cams[0], oc, rad.data_ptr(), rgb.data_ptr())
            torch.cuda.synchronize()
            assert hs.last_trace_build() == "general"  # the counting build is general
            counters = hs.debug_counters()
            got = (rad.cpu().numpy().view(np.uint8), rgb.cpu().numpy())
            assert np.array_equal(got[0], out[0][0]) and np.array_equal(got[1], out[0][1]), "counting launch: other bits"
        hs.check()
    return out, build, counters


def _same_bits(hip, monkeypatch, sc, cams, opts, *, expect_auto="plain", env=None, **kw):
    """Both builds on the same frames; returns auto's frames and counters."""
    import torch
    _set_build(monkeypatch, "auto", env)
    auto, build_auto, counters = _frames(hip, torch, sc, cams, opts, **kw)
    assert build_auto == expect_auto, (build_auto, expect_auto)
    _set_build(monkeypatch, "general", env)
    gen, build_gen, _ = _frames(hip, torch, sc, cams, opts, **{**kw, "count": False})
    assert build_gen == "general", build_gen
    assert len(auto) == len(gen) == len(cams)
    for k, ((ra, ia), (rg, ig)) in enumerate(zip(auto, gen)):
        assert np.array_equal(ra, rg), f"frame {k}: radiance of the two builds differs in {int((ra != rg).sum())} bytes"
        assert np.array_equal(ia, ig), f"frame {k}: RGB8 of the two builds differs in {int((ia != ig).sum())} bytes"
        if opts[k].tile_world == 1:  # (a packed rank's slot may end in filler; a frame has a sample in every pixel)
            assert not np.isnan(ra.view(np.float32)).any(), f"frame {k}: pixels nobody wrote"
    return auto, counters


@pytest.fixture(scope="module")
def plain_scene(oracle):
    return scenes.example_scene(oracle, 2000)  # four spheres and one 2,000-triangle mesh


# ---- selection ------------------------------------------------------------------------------------------------------
def _one_frame_build(hip, monkeypatch, sc, oracle, build=None, env=None, flags=0):
    import torch
    _set_build(monkeypatch, build, env)
    cam = scenes.camera(oracle, 48, 32)
    _, used, _ = _frames(hip, torch, sc, [cam], [abi.default_opts(spp=2, seed=3, flags=flags)])
    return used


def test_plain_build_runs_for_the_plain_scene_at_default_knobs(hip, oracle, monkeypatch, plain_scene):
    assert _one_frame_build(hip, monkeypatch, plain_scene, oracle) == "plain"  # (no control set at all)
    assert _one_frame_build(hip, monkeypatch, plain_scene, oracle, "auto") == "plain"


def test_general_build_runs_for_everything_else(hip, oracle, monkeypatch, plain_scene):
    mesh = lambda n, **over: scenes.standin_mesh(oracle, n, **{**scenes.EXAMPLE_MESH, **over})  # noqa: E731
    two_meshes = abi.SceneData(spheres=scenes.EXAMPLE_SPHERES, meshes=[mesh(2000), mesh(500, translation=(-4.0, -1.0, -7.0), scale=20.0)])
    one_element = abi.SceneData(spheres=scenes.EXAMPLE_SPHERES, meshes=[mesh(2000)], triangles=scenes.TRIANGLES[:1],
                                element_order=[0, 1, T | 0, 2, 3])
    assert _one_frame_build(hip, monkeypatch, two_meshes, oracle) == "general"
    assert _one_frame_build(hip, monkeypatch, one_element, oracle) == "general"
    assert _one_frame_build(hip, monkeypatch, plain_scene, oracle, env={"RBRT_Y_LOW": "20"}) == "general"
    assert _one_frame_build(hip, monkeypatch, plain_scene, oracle, flags=abi.FLAG_COLLECT_STATS) == "general"
    assert _one_frame_build(hip, monkeypatch, plain_scene, oracle, "general") == "general"
    assert _one_frame_build(hip, monkeypatch, scenes.spheres_scene(), oracle) == "general"  # (no mesh at all)


def test_the_build_control_is_validated_at_scene_creation(hip, monkeypatch, plain_scene):
    lib = abi.load_hip()

    def create():
        h = C.c_void_p()
        rc = lib.rbrt_hip_scene_create(plain_scene.ptr(), 0, C.byref(h))
        if rc == abi.RBRT_OK:
            lib.rbrt_hip_scene_destroy(h)
        return rc, lib.rbrt_hip_last_error().decode(errors="replace")

    refused = ["", "plain", "AUTO", "general ", "1", "auto,general"]
    for v in ("auto", "general"):
        _set_build(monkeypatch, v)
        assert create()[0] == abi.RBRT_OK, v
    for v in refused:
        _set_build(monkeypatch, v)
        rc, msg = create()
        assert rc == abi.RBRT_ERR_INVALID_ARG and "RBRT_TRACE_BUILD" in msg, (v, rc, msg)
    monkeypatch.delenv("RBRT_HIP_LAB")  # outside lab mode the string is not read at all
    for v in refused:
        monkeypatch.setenv("RBRT_TRACE_BUILD", v)
        assert create()[0] == abi.RBRT_OK, v


# ---- same bits ------------------------------------------------------------------------------------------------------
def test_golden_frame_both_builds(hip, oracle, monkeypatch, plain_scene):
    """160 x 120 x 4 spp, seed 2: both builds, and the golden the oracle made."""
    cam = scenes.camera(oracle, 160, 120)
    auto, _ = _same_bits(hip, monkeypatch, plain_scene, [cam], [abi.default_opts(spp=4, seed=2)])
    g = np.load(GOLDEN)
    rad = auto[0][0].view(np.float32).reshape(120, 160, 3)
    rgb = auto[0][1].reshape(120, 160, 3)
    assert _sha(rad) == str(g["radiance_sha256"]) and _sha(rgb) == str(g["rgb8_sha256"])


def test_ragged_tiles_both_builds(hip, oracle, monkeypatch, plain_scene):
    _same_bits(hip, monkeypatch, plain_scene, [scenes.camera(oracle, 70, 50)], [abi.default_opts(spp=3, seed=5)])


@pytest.mark.parametrize("max_depth", [0, 1, 50])
def test_max_depth_both_builds(hip, oracle, monkeypatch, plain_scene, max_depth):
    _same_bits(hip, monkeypatch, plain_scene, [scenes.camera(oracle, 96, 64)], [abi.default_opts(spp=3, seed=8, max_depth=max_depth)])


def test_every_rank_of_three_both_builds(hip, oracle, monkeypatch, plain_scene):
    cam = scenes.camera(oracle, 100, 61)
    opts = [abi.default_opts(spp=3, seed=4, tile_rank=r, tile_world=3) for r in range(3)]
    _same_bits(hip, monkeypatch, plain_scene, [cam] * 3, opts)


def _moving_cameras(oracle, n):
    return [scenes.camera(oracle, 160, 120, position=(0.4 * k - 1.0, 5.0 + 0.1 * k, 4.0)) for k in range(n)]


@pytest.mark.parametrize("helpers", [False, True], ids=["stream", "stream_with_helpers"])
def test_six_frames_at_pipeline_depth_four_both_builds(hip, oracle, monkeypatch, plain_scene, helpers):
    """A camera that changes per frame: overlapped grids, the short-path stage's masks and the tile pass; with RBRT_HELPERS=2
    a helper launch -- the helper twin of each build -- joins every overlapped launch."""
    cams = _moving_cameras(oracle, 6)
    opts = [abi.default_opts(spp=4, seed=20 + k) for k in range(6)]
    _same_bits(hip, monkeypatch, plain_scene, cams, opts, pipeline=4, check_helpers=helpers,
               env={"RBRT_HELPERS": "2"} if helpers else None)


def test_tree_deeper_than_the_lds_stack_both_builds(hip, oracle, monkeypatch):
    """The rough stand-in's tree is deeper than the stack entries a lane keeps in LDS: the global-stack arm runs in both
    builds (the counting launch's counter says so for this tree and these rays)."""
    sc = scenes.example_scene(oracle, 6003, kind="rough")
    cam = scenes.camera(oracle, 128, 96)
    _, counters = _same_bits(hip, monkeypatch, sc, [cam], [abi.default_opts(spp=4, seed=6)], count=True)
    assert counters["stack_pushes_beyond_lds"] > 0, counters["stack_pushes_beyond_lds"]
