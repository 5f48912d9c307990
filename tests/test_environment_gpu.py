"""Environment lighting on the GPU (rbrt_hip.h "Environment lighting"): the lookup through the debug hook, whole images, the
constant map, background-only tiles, scaling, the handle's state, the refusals and the CLI -- bit for bit against np_env's
numpy restatement unless a test says otherwise. Images are small so that the restatement (a Python loop) stays fast."""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import np_env
import np_lens
import np_smooth
import scenes
import test_emissive as E
from rbrt_amd import abi

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
W, H = E.W, E.H
FLAG = abi.FLAG_CONSTANT_BACKGROUND
bits = E.bits


def render(hs, cam, opts, lens=None, how="device"):
    """(radiance, rgb8) of one blocking render on the handle, whatever environment it has."""
    import torch
    h, w = cam.img_height_pix, cam.img_width_pix
    rad = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
    rgb = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    if how == "device":
        hs.render_device(cam, opts, rad.data_ptr(), rgb.data_ptr(), lens=lens)
    elif how == "passes":  # a series cut in the middle
        acc = torch.full((abi.load_hip().rbrt_hip_packed_pixels(w, h, 0, 1) * 3,), float("nan"), dtype=torch.float32, device="cuda")
        cut = max(1, opts.spp // 2)
        hs.render_pass(cam, opts, 0, cut, acc.data_ptr(), lens=lens)
        hs.render_pass(cam, opts, cut, opts.spp, acc.data_ptr(), rad.data_ptr(), rgb.data_ptr(), lens=lens)
    elif how == "adaptive":  # threshold 0 stops nothing early: the fixed render
        hs.render_adaptive(cam, opts, 0.0, min_samples=2, step=1, d_radiance=rad.data_ptr(), d_rgb8=rgb.data_ptr(), lens=lens)
    torch.cuda.synchronize()
    hs.check()
    return rad.cpu().numpy(), rgb.cpu().numpy()


# ---- the lookup ------------------------------------------------------------------------------------------------------------
def lookup_directions(n):
    rng = np.random.default_rng(100 + n)
    d = rng.normal(size=(4000, 3))
    unit = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)
    # the hemisphere seam: dy = +-0 and +-1e-7, all around
    ring = unit[:64].copy()
    seam = np.concatenate([ring * np.array([1, 0, 1], f32) + np.array([0, y, 0], f32) for y in (0.0, -0.0, 1e-7, -1e-7)])
    seam[64:128, 1] = -0.0
    # the sign rule: px = 0 and pz = 0 (both signs of zero) in the lower hemisphere
    t = np.linspace(-1.0, 1.0, 33, dtype=f32)
    signs = np.concatenate([np.stack([np.full_like(t, z), -np.abs(t) - f32(0.1), t], 1) for z in (0.0, -0.0)] +
                           [np.stack([t, -np.abs(t) - f32(0.1), np.full_like(t, z)], 1) for z in (0.0, -0.0)]).astype(f32)
    # directions that land exactly on nodes, the last row and column included (float32 of the node's own direction), and on
    # the cell centres
    nodes = np_env.node_directions(n).reshape(-1, 3).astype(f32)
    k = (2.0 * (np.arange(n) + 0.5) - n) / n
    cu, cv = np.meshgrid(k, k)
    cy = 1.0 - np.abs(cu) - np.abs(cv)
    centres = np.stack([cu, cy, cv], -1).reshape(-1, 3)[cy.reshape(-1) >= 0].astype(f32)
    scaled = np.concatenate([unit[:500] * f32(1e-20), unit[:500] * f32(1e18), unit[:200] * f32(1e-42), unit[:200] * f32(3.0)])
    return np.concatenate([unit, axes, seam, signs, nodes, centres, scaled]).astype(f32)


BAD_DIRECTIONS = np.array([(np.nan, 0, 0), (0, np.nan, 0), (0, 0, np.nan), (np.nan, np.nan, np.nan), (np.inf, 0, 0), (0, -np.inf, 0),
                           (1, 1, np.inf), (np.inf, np.inf, np.inf), (-np.inf, 1, -np.inf), (0, 0, 0), (-0.0, -0.0, -0.0), (0, -0.0, 0),
                           (3e38, 3e38, 3e38), (-3e38, 3e38, 1)], f32)


@pytest.mark.parametrize("n", [1, 2, 3, 64])
def test_lookup_against_the_restatement(hip, n):
    nodes = np_env.noise_map(n, 40 + n)
    dirs = lookup_directions(n)
    with hip.HipScene(scenes.spheres_scene()) as hs:
        hs.set_environment(nodes)
        got = hs.environment_lookup(dirs)
        bad = hs.environment_lookup(BAD_DIRECTIONS)  # the call returns ...
        hs.check()                                   # ... and nothing was flagged
    exp = np_env.lookup(nodes, dirs)
    assert np.isfinite(exp).all() and exp.min() >= 0.0 and exp.max() <= 8.0
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    i, j, fx, fy = np_env.cell(dirs, n)
    assert i.min() == 0 and j.min() == 0 and i.max() == n - 1 and j.max() == n - 1  # (every row and column of cells is visited)
    assert fx.min() >= 0 and fy.min() >= 0 and fx.max() <= 1 and fy.max() <= 1
    exp_bad = np_env.lookup(nodes, BAD_DIRECTIONS)
    assert np.array_equal(np.isnan(bad), np.isnan(exp_bad))
    assert np.array_equal(bits(bad)[~np.isnan(exp_bad)], bits(exp_bad)[~np.isnan(exp_bad)])
    # a NaN or a zero direction gives a NaN colour (an infinite one need not: (0, -inf, 0) folds to the corner node)
    assert np.isnan(exp_bad[[0, 1, 2, 3, 9, 10, 11]]).all(axis=1).all()


def test_lookup_needs_an_environment(hip):
    with hip.HipScene(scenes.spheres_scene()) as hs:
        with pytest.raises(abi.RbrtError) as e:
            hs.environment_lookup(np.array([[0, 1, 0]], f32))
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG


# ---- images ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lit(oracle):
    return E.lit_scene(oracle)


@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("max_depth,spp", [(0, 2), (1, 2), (50, 3)])
def test_images_against_the_restatement(hip, oracle, lit, max_depth, spp, lensed):
    cam = scenes.camera(oracle, W, H)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 60.0, 9.0) if lensed else None
    nodes = np_env.noise_map(16, 5) if max_depth else np_env.smooth_map(16, 5)
    # (bg and the flag are ignored while the handle has a map: the restatement never reads them)
    opts = abi.default_opts(spp=spp, seed=3, max_depth=max_depth, flags=FLAG if lensed else 0, bg=(9.0, 9.0, 9.0))
    with hip.HipScene(lit) as hs:
        hs.set_environment(nodes)
        got, got8 = render(hs, cam, opts, lens)
    exp, exp8 = np_env.restated_image(cam, lit, opts, nodes, lens)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    assert len(np.unique(bits(got).reshape(-1, 3), axis=0)) > 50  # (not one colour: the map is in the picture)


def test_smooth_sphere_mesh_against_the_restatement(hip, oracle):
    cam = scenes.camera(oracle, W, H)
    _, ball = np_smooth.sphere_mesh(oracle, (0.5, 1.6, -7.0), 1.6, 3, abi.material(abi.MAT_METAL, (0.9, 0.8, 0.7), 0.0))
    sc = abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES), meshes=[ball])
    nodes = np_env.noise_map(7, 9)
    opts = abi.default_opts(spp=2, seed=11)
    with hip.HipScene(sc) as hs:
        hs.set_environment(nodes)
        got, got8 = render(hs, cam, opts)
    exp, exp8 = np_env.restated_image(cam, sc, opts, nodes)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)


# ---- a constant map is the constant background ---------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["device", "passes", "adaptive", "ranks"])
def test_a_constant_map_is_the_constant_background(hip, oracle, lit, how):
    import torch
    w, h = 70, 45  # ragged tiles on both edges
    cam = scenes.camera(oracle, w, h)
    c = (0.375, 1.25, 0.0625)
    nodes = np.broadcast_to(np.array(c, f32), (6, 6, 3)).copy()
    opts = abi.default_opts(spp=4, seed=2, flags=FLAG, bg=c)
    plain = abi.default_opts(spp=4, seed=2)  # (with the map set: neither the flag nor bg)

    def ranks(hs, o):
        world = 3
        slot = hip.packed_pixels(w, h, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            ro = abi.default_opts(spp=o.spp, seed=o.seed, flags=o.flags, bg=tuple(o.bg), tile_rank=r, tile_world=world)
            hs.render_device(cam, ro, slots[r * slot * 3:].data_ptr())
        merged = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        merged8 = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
        hip.unpack_tiles(0, slots.data_ptr(), w, h, world, merged.data_ptr(), merged8.data_ptr(), None, rank_stride_pixels=slot)
        torch.cuda.synchronize()
        hs.check()
        return merged.cpu().numpy(), merged8.cpu().numpy()

    with hip.HipScene(lit) as hs:
        exp, exp8 = render(hs, cam, opts)
        hs.set_environment(nodes)
        got, got8 = ranks(hs, plain) if how == "ranks" else render(hs, cam, plain, how=how)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)


# ---- background-only tiles --------------------------------------------------------------------------------------------------
def test_background_only_tiles(hip, oracle, tmp_path):
    import torch
    w, h = 64, 48
    cam = scenes.camera(oracle, w, h)  # the example camera: the top tiles see the sky only
    sc = E.lit_scene(oracle, with_triangles=False)
    nodes = np_env.noise_map(32, 21)
    opts = abi.default_opts(spp=2, seed=4)
    with hip.HipScene(sc) as hs:
        hs.set_environment(nodes)
        sky = (hs.primary_cull(cam) >> 31) & 1
        assert sky.any() and not sky.all(), sky
        got, got8 = render(hs, cam, opts)
        ada, ada8 = render(hs, cam, opts, how="adaptive")  # sky_resolve_even_kernel
        den = torch.full((h, w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.denoise(den.data_ptr())
        torch.cuda.synchronize()
        hs.check()
        assert torch.isfinite(den).all()
    exp, exp8 = np_env.restated_image(cam, sc, opts, nodes)
    assert np.array_equal(bits(got), bits(exp)), np.argwhere(bits(got) != bits(exp))[:5]
    assert np.array_equal(got8, exp8)
    assert np.array_equal(bits(ada), bits(got)) and np.array_equal(ada8, got8)
    for ty, tx in np.argwhere(sky):  # (noise: a sky tile is not one colour)
        assert len(np.unique(bits(got[ty * 8:(ty + 1) * 8, tx * 8:(tx + 1) * 8]).reshape(-1, 3), axis=0)) > 32
    # without the tile pass (a lab knob, read when the library is loaded: a fresh process) the trace kernel renders those tiles
    np.save(tmp_path / "nodes.npy", nodes)
    script = tmp_path / "no_cull.py"
    script.write_text(f"""
import sys
sys.path[:0] = [{str(ROOT)!r}, {str(ROOT / 'tests')!r}]
import numpy as np, torch
import rbrt_amd, scenes, test_emissive as E
from oracle import pyoracle
from rbrt_amd import abi
cam = scenes.camera(pyoracle, {w}, {h})
out = torch.full(({h}, {w}, 3), float("nan"), dtype=torch.float32, device="cuda")
with rbrt_amd.HipScene(E.lit_scene(pyoracle, with_triangles=False)) as hs:
    hs.set_environment(np.load({str(tmp_path / 'nodes.npy')!r}))
    hs.render_device(cam, abi.default_opts(spp=2, seed=4), out.data_ptr())
    torch.cuda.synchronize()
    hs.check()
np.save({str(tmp_path / 'off.npy')!r}, out.cpu().numpy())
""")
    env = dict(os.environ, RBRT_HIP_LAB="1", RBRT_PRIMARY_CULL="0")
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(bits(np.load(tmp_path / "off.npy")), bits(got))


# ---- scaling ----------------------------------------------------------------------------------------------------------------
def test_doubling_every_node_doubles_every_radiance(hip, oracle):
    cam = scenes.camera(oracle, 64, 48)
    sc = scenes.example_scene(oracle, 61)  # no emitters: every path ends in the map or in black
    nodes = np_env.noise_map(24, 8)
    opts = abi.default_opts(spp=4, seed=8, max_depth=16)
    with hip.HipScene(sc) as hs:
        hs.set_environment(nodes)
        one, _ = render(hs, cam, opts)
        hs.set_environment(nodes * f32(2.0))
        two, _ = render(hs, cam, opts)
    assert (one > 0).any(axis=2).mean() > 0.5
    assert np.array_equal(bits(two), bits(one * f32(2.0)))


# ---- the handle's state ------------------------------------------------------------------------------------------------------
def test_set_and_cleared_renders_the_golden(hip, oracle):
    import test_golden as G
    name = "cfg1_spheres_400x300x8_seed1"
    case = G.make_golden.CASES[name]
    cam = scenes.camera(oracle, case["w"], case["h"])
    opts = abi.default_opts(spp=case["spp"], seed=case["seed"])
    with hip.HipScene(G.make_golden.build_scene(case)) as hs:
        hs.set_environment(np_env.noise_map(64, 1))
        lit_img, _ = render(hs, cam, opts)
        hs.set_environment(None)
        rad, rgb = render(hs, cam, opts)
        hs.set_environment(None)  # (clearing twice is fine)
    G.check(name, rad, rgb)
    assert not np.array_equal(bits(lit_img), bits(rad))


def test_replacing_the_map(hip, oracle, lit):
    cam = scenes.camera(oracle, 64, 48)
    opts = abi.default_opts(spp=2, seed=5)
    maps = {64: np_env.noise_map(64, 2), 3: np_env.noise_map(3, 3)}
    fresh = {}
    for n, nodes in maps.items():
        with hip.HipScene(lit) as hs:
            hs.set_environment(nodes)
            fresh[n] = render(hs, cam, opts)[0]
    assert not np.array_equal(bits(fresh[64]), bits(fresh[3]))
    with hip.HipScene(lit) as hs:
        for n in (64, 3, 64):
            hs.set_environment(maps[n])
            assert np.array_equal(bits(render(hs, cam, opts)[0]), bits(fresh[n])), n
            assert np.array_equal(bits(hs.environment_lookup(np.array([[0.3, 0.5, -0.2]], f32))),
                                  bits(np_env.lookup(maps[n], np.array([[0.3, 0.5, -0.2]], f32))))


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was(hip, oracle, lit):
    cam = scenes.camera(oracle, W, H)
    opts = abi.default_opts(spp=2, seed=6)
    good = np_env.noise_map(5, 6)
    nan_map, neg_map, inf_map = good.copy(), good.copy(), good.copy()
    nan_map[3, 2, 1], neg_map[5, 5, 2], inf_map[0, 0, 0] = np.nan, -1e-30, np.inf
    big = np.zeros((2, 2, 3), f32)
    cases = [dict(nodes=good, n=0), dict(nodes=big, n=4097), dict(nodes=good, reserved=1), dict(nodes=None, n=5),
             dict(nodes=nan_map), dict(nodes=neg_map), dict(nodes=inf_map)]
    with hip.HipScene(lit) as hs:
        for state in ("no map", "a map"):
            if state == "a map":
                hs.set_environment(good)
            before, _ = render(hs, cam, opts)
            for kw in cases:
                with pytest.raises(abi.RbrtError) as e:
                    hs.set_environment(kw["nodes"], n=kw.get("n"), reserved=kw.get("reserved", 0))
                assert e.value.code == abi.RBRT_ERR_INVALID_ARG, (state, kw.get("n"), kw.get("reserved"))
            after, _ = render(hs, cam, opts)
            assert np.array_equal(bits(after), bits(before)), state
    assert abi.load_hip().rbrt_hip_scene_set_environment(None, None) == abi.RBRT_ERR_INVALID_ARG


# ---- the CLI -----------------------------------------------------------------------------------------------------------------
def _png(path):
    from PIL import Image
    return np.array(Image.open(path))


def test_cli_matches_the_python_path(hip, tmp_path):
    img = np.random.default_rng(12).uniform(0.0, 4.0, (16, 32, 3)).astype(f32)
    np_env.write_pfm(tmp_path / "map.pfm", img)
    shipped = (ROOT / "scenes" / "environment" / "environment_spheres.yaml").read_text()
    # the Python path: the same scene file with the test's map and resolution in its blueprint
    text = shipped.replace("scenes/environment/standin_sky.pfm", str(tmp_path / "map.pfm")).replace("resolution: 1024", "resolution: 16")
    assert text != shipped and "resolution: 16" in text
    (tmp_path / "scene.yaml").write_text(text)
    hs_host = abi.HostScene(tmp_path / "scene.yaml", H, W)
    nodes = hs_host.environment()
    assert nodes.shape == (17, 17, 3)
    with hip.HipScene(hs_host) as hs:
        hs.set_environment(nodes)
        _, exp8 = render(hs, hs_host.camera, abi.default_opts(spp=4, seed=1))
        hs.set_environment(None)
        _, sky8 = render(hs, hs_host.camera, abi.default_opts(spp=4, seed=1))
    rot = float(f32(20.0))
    assert np.array_equal(bits(nodes), bits(abi.environment_nodes(img, 16, rot, 1.0)))
    common = ["-c", str(ROOT / "scenes" / "environment" / "environment_spheres.yaml"), "--height", str(H), "-w", str(W), "-s", "4"]
    for gpus in ("1", "3"):  # (the N-rank host on one GPU: every rank's handle gets the map)
        out, rep = tmp_path / f"g{gpus}.png", tmp_path / f"g{gpus}.json"
        r = subprocess.run([str(EXE), *common, "--environment", str(tmp_path / "map.pfm"), "--environment-resolution", "16", "-t", str(out),
                            "--gpus", gpus, "--oversubscribe", "--report", str(rep)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == 0, r.stderr[-2000:]
        assert np.array_equal(_png(out), exp8), gpus
        j = json.loads(rep.read_text())
        assert j["environment_file"] == str(tmp_path / "map.pfm") and j["environment_resolution"] == 16
    out = tmp_path / "none.png"
    r = subprocess.run([str(EXE), *common, "--environment", "none", "-t", str(out)], capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(_png(out), sky8) and not np.array_equal(sky8, exp8)
