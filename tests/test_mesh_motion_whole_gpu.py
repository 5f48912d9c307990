"""Moving meshes together with every other per-sample feature, in the manner of test_all_features_gpu.py and test_whole_gpu.py:
whole_scenes.fuzz_case -- emitters, backgrounds, the lens, smooth and flat meshes with decorated normals, shuffled
BasicTriangles, distance windows, solid patterns, a shutter, moving spheres, a phase, an environment -- with a travel on
every mesh, bit for bit against the joined restatement with the mesh rule added (np_mesh_motion.restated_image, whose colorize
is np_whole's on the per-mesh origin: with all travels zero it IS np_whole's image, which this file checks case by case)."""
from __future__ import annotations

import numpy as np
import pytest

import np_mesh_motion as MM
import np_whole as NW
import test_motion_gpu as MG
import test_whole_gpu as TW
import whole_scenes as WS
from rbrt_amd import tiles

pytestmark = pytest.mark.gpu

f32 = np.float32
bits, render = MG.bits, MG.render
# the first 16 seeds of whole_scenes.fuzz_case whose scene has a mesh and whose restated image the travels below change (the
# tiny cases' meshes cover a pixel or two: in most of them no sample meets a mesh at all), chosen on the CPU
SEEDS = [10, 26, 31, 39, 40, 44, 45, 47, 51, 54, 59, 62, 72, 81, 86, 88]


def mesh_travels_of(case, seed):
    """A travel per mesh: one in four stays, most move up to 1.5 units, one in six far enough to leave the frame."""
    rng = np.random.default_rng(197000 + seed)
    out = np.zeros((len(case.sc.meshes), 3), f32)
    for m in range(len(out)):
        u = rng.random()
        if u >= 0.25:
            out[m] = (WS.log_uniform(rng, 20.0, 60.0) if u > 0.83 else WS.log_uniform(rng, 1e-3, 1.5)) * WS.unit(rng)
    return out


def restate(case, mw, **kw):
    return MM.restated_image(case.cam, case.sc, case.opts, mw, travels=case.travels, phase=case.phase, lens=case.lens, shutter=case.shutter,
                             nodes=case.nodes, **kw)


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzzed_scenes_with_every_feature_and_moving_meshes(hip, oracle, monkeypatch, seed):
    """render_device against the restatement; then, against that image, the short-path stage off and forced, the tile pass off,
    render_pass one sample at a time, render_adaptive with threshold 0 and the two ranks of tile_world = 2."""
    import torch
    case = WS.fuzz_case(oracle, seed)
    assert case.sc.meshes, case.what
    cam, lens, opts = case.cam, case.lens, case.opts
    w, h = cam.img_width_pix, cam.img_height_pix
    mw = mesh_travels_of(case, seed)
    if case.builder:
        monkeypatch.setenv("RBRT_BVH_BUILDER", case.builder)
    else:
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    # the restatement with the mesh rule reduces to the joined one: zero mesh travels on a handle whose spheres draw
    zero, _ = restate(case, np.zeros_like(mw))
    tv0 = case.travels if case.travels is not None else np.zeros((len(case.sc.spheres), 3), f32)
    joined, _ = NW.restated_image(cam, case.sc, opts, lens=lens, shutter=case.shutter, travels=tv0, phase=case.phase, nodes=case.nodes)
    assert TW.same(zero, joined), case.what
    exp, exp8 = restate(case, mw)
    assert not TW.same(exp, zero), case.what  # (the travels do something in this case)
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        hs.set_mesh_motion(mw)
        got, got8 = render(hs, cam, opts, lens)
        hs.check()
        assert TW.same(got, exp), (case.what, mw.tolist(), TW.where(got, exp))
        assert np.array_equal(got8, exp8), case.what
        for mode in (0, 2):
            hs.set_short_paths(mode)
            again, _ = render(hs, cam, opts, lens)
            assert TW.same(again, got), (case.what, f"set_short_paths({mode})", TW.where(again, got))
        hs.set_short_paths(1)
        acc, out = TW.frame(torch, cam), TW.frame(torch, cam)
        for s in range(opts.spp):
            hs.render_pass(cam, opts, s, s + 1, acc.data_ptr(), out.data_ptr() if s + 1 == opts.spp else None, lens=lens)
        torch.cuda.synchronize()
        assert TW.same(out.cpu().numpy(), got), (case.what, "render_pass", TW.where(out.cpu().numpy(), got))
        out = TW.frame(torch, cam)
        hs.render_adaptive(cam, opts, 0.0, 2, 1, out.data_ptr(), lens=lens)
        torch.cuda.synchronize()
        assert TW.same(out.cpu().numpy(), got), (case.what, "render_adaptive", TW.where(out.cpu().numpy(), got))
        packed = []
        for rank in range(2):
            buf = torch.full((max(1, hip.packed_pixels(w, h, rank, 2)), 3), float("nan"), dtype=torch.float32, device="cuda")
            hs.render_device(cam, TW.copy_opts(opts, tile_rank=rank, tile_world=2), buf.data_ptr(), lens=lens)
            torch.cuda.synchronize()
            packed.append(buf.cpu().numpy()[:tiles.packed_pixels(w, h, rank, 2)])
        merged = tiles.unpack(packed, w, h)
        assert TW.same(merged, got), (case.what, "tile_world 2", TW.where(merged, got))
    monkeypatch.setenv("RBRT_PRIMARY_CULL", "0")
    with WS.configure(hip.HipScene(case.sc), case) as hs:
        hs.set_mesh_motion(mw)
        off, _ = render(hs, cam, opts, lens)
        hs.check()
    assert TW.same(off, got), (case.what, "without the tile pass", TW.where(off, got))
