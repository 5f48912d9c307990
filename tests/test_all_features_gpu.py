"""Emitters, the constant background, the thin lens and smooth shading together on the GPU, against the CPU oracle's
extended path (rbrt_oracle_render_ext, pinned to the numpy restatements by test_oracle_extensions.py), bit for bit.

A fuzz over every feature at once; scenes at the object limit (255 objects) with a pinhole and with a lens; a scene at the
boundary where a lens launch's 32 extra bytes of LDS cost a resident wave per CU; every entry point, schedule and lab-knob
row on one scene with everything; the shipped feature scenes through the product's host path."""
from __future__ import annotations

import os
from pathlib import Path

import numpy as np
import pytest
import yaml

import full_scenes as F
import np_lens
import np_smooth
import scenes
import test_lab_knobs as K
from rbrt_amd import abi, standin, tiles
from test_gpu_parity import assert_same_image

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
N_FUZZ = int(os.environ.get("RBRT_FUZZ_FULL_SCENES", "24"))


def opts_kw(opts):
    """The render_scene overrides that reproduce `opts` (spp and seed aside)."""
    return dict(max_depth=opts.max_depth, min_dist=opts.min_dist, max_dist=opts.max_dist, bg=tuple(opts.bg), flags=opts.flags)


def copy_opts(opts, **kw):
    o = abi.default_opts(spp=opts.spp, seed=opts.seed, **opts_kw(opts))
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def frame(torch, cam, fill=float("nan")):
    return torch.full((cam.img_height_pix, cam.img_width_pix, 3), fill, dtype=torch.float32, device="cuda")


def same_frame(torch, t, exp, what):
    torch.cuda.synchronize()
    assert_same_image(t.cpu().numpy(), exp, what)


# ---- the fuzz ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(N_FUZZ))
def test_fuzzed_scenes_with_every_feature(hip, oracle, monkeypatch, seed):
    """full_scenes.fuzz_case: four material kinds, emitters from L = 0 to large, gradient or constant backgrounds, pinhole or
    lens (apertures from 0 to past the focus distance), flat and smooth meshes with decorated normals, BasicTriangles in a
    shuffled order, distance windows, depth 0 / 1 / 3 / 50, 1-5 spp, ragged sizes, both builders. Every third seed also
    compares the debug hook's shading normals with the oracle's."""
    case = F.fuzz_case(oracle, seed)
    cam, lens, sc, opts = case["cam"], case["lens"], case["sc"], case["opts"]
    if case["builder"]:
        monkeypatch.setenv("RBRT_BVH_BUILDER", case["builder"])
    else:
        monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    nan0 = oracle.lib().rbrt_oracle_nan_discriminants()
    exp, exp8, _ = oracle.render(cam, sc, opts, lens=lens)
    try:
        got, got8 = hip.render_scene(cam, opts.spp, sc, seed=opts.seed, lens=lens, **opts_kw(opts))
    except abi.RbrtError as e:  # the reference would have panicked (sphere.rs:33): the oracle must have met it too
        assert e.code == abi.RBRT_ERR_NAN and oracle.lib().rbrt_oracle_nan_discriminants() > nan0, case["what"]
        return
    assert_same_image(got, exp, case["what"])
    assert np.array_equal(got8, exp8)
    if seed % 3 == 0 and sc.meshes:
        rays = F.mesh_rays(sc, np.random.default_rng(seed), per_mesh=300)
        with hip.HipScene(sc) as hs:
            g = hs.shading_normals(rays, opts.min_dist, opts.max_dist)
        e = oracle.shading_normals(sc, rays, opts.min_dist, opts.max_dist)
        assert F.same_bits(g, e), case["what"]


# ---- the object limit ---------------------------------------------------------------------------------------------------------
def last_object_rays(sc, rng):
    """Rays down onto the last element sphere, or at the entries of the last mesh."""
    if sc.meshes:
        return F.mesh_rays(abi.SceneData(meshes=[sc.meshes[-1]]), rng, per_mesh=400)
    c, r, _ = sc.spheres[-1]
    o = np.array(c) + np.array([0.0, 4.0, 0.0]) + np.concatenate([rng.uniform(-0.5 * r, 0.5 * r, (200, 1)), np.zeros((200, 1)),
                                                                  rng.uniform(-0.5 * r, 0.5 * r, (200, 1))], 1)
    return np.concatenate([o, np.tile([0.0, -1.0, 0.0], (200, 1))], 1).astype(f32)


@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("mix", ["spheres", "smooth_last", "mixed"])
def test_scenes_at_the_object_limit(hip, oracle, mix, lensed):
    sc = F.limit_scene(oracle, mix)
    assert len(sc.spheres) + len(sc.triangles) + len(sc.meshes) == F.N_MAX
    cam = scenes.camera(oracle, 72, 52)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 30.0, 10.0) if lensed else None
    opts = abi.default_opts(spp=2, seed=5, max_depth=12)
    exp, exp8, _ = oracle.render(cam, sc, opts, lens=lens)
    got, got8 = hip.render_scene(cam, 2, sc, seed=5, lens=lens, max_depth=12)
    assert_same_image(got, exp, f"{mix} lens={lensed}")
    assert np.array_equal(got8, exp8)
    assert (got > 1.0).any()  # (emitters in view)
    rng = np.random.default_rng(len(mix))
    z = ((0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 1.0)
    cam_rays = np_lens.lens_rays(cam, lens or z, rng.random((52, 72)).astype(f32), rng.random((52, 72)).astype(f32),
                                 f32(0.3) if lensed else f32(0.0), f32(-0.5) if lensed else f32(0.0))
    rays = np.concatenate([cam_rays, last_object_rays(sc, rng)])
    with hip.HipScene(sc) as hs:
        gt, go, gi, _ = hs.trace_rays(rays)
        hs.check()
    et, eo, ei, _ = oracle.trace_rays(sc, rays)
    assert np.array_equal(go, eo) and np.array_equal(gi, ei) and F.same_bits(gt, et)
    assert (eo == F.N_MAX - 1).sum() > 20 and len(np.unique(eo)) > 30


# ---- the lens LDS boundary ------------------------------------------------------------------------------------------------------
LDS_CU = 160 * 1024


def boundary_scene(oracle, n_spheres, n_tris):
    rng = np.random.default_rng(n_spheres * 1000 + n_tris)
    sph = F.sphere_grid(rng, n_spheres)
    tris = [(((-3.0 + 0.4 * k, 0.2, -6.0), (-2.7 + 0.4 * k, 0.25, -6.3), (-2.9 + 0.4 * k, 0.9, -6.6)), F.mat(rng)) for k in range(n_tris)]
    order = list(range(n_spheres)) + [F.T | i for i in range(n_tris)]
    rng.shuffle(order)
    md = F.smooth_standin(oracle, rng, 200, 25.0, (1.0, -0.5, -9.0), abi.material(abi.MAT_METAL, (0.9, 0.8, 0.7), 0.05), "computed")
    return abi.SceneData(spheres=sph, meshes=[md], triangles=tris, element_order=order)


def test_a_lens_at_the_lds_boundary(hip, oracle):
    """Sphere and triangle counts where floor(160 KiB / lds) != floor(160 KiB / (lds + 32)): the handle's resident waves per
    CU are sized for the pinhole, and a lens launch's 32 bytes more leave one of them waiting for another to end."""
    import torch

    def lds_of(ns, nt):
        with hip.HipScene(boundary_scene(oracle, ns, nt)) as hs:
            return hs.info()["lds_bytes_per_wave"]
    l11, l21, l12 = lds_of(1, 1), lds_of(2, 1), lds_of(1, 2)
    ds, dt = l21 - l11, l12 - l11
    assert ds > 0 and dt > 0
    pick = None
    for nt in range(1, 40):
        for ns in range(1, F.N_MAX - nt):
            lds = l11 + (ns - 1) * ds + (nt - 1) * dt
            if LDS_CU // lds <= 20 and LDS_CU // lds != LDS_CU // (lds + 32):
                pick = (ns, nt, lds)
                break
        if pick:
            break
    assert pick, (l11, ds, dt)
    ns, nt, lds = pick
    sc = boundary_scene(oracle, ns, nt)
    cam = scenes.camera(oracle, 64, 48)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 25.0, 9.0)
    opts = abi.default_opts(spp=2, seed=3, max_depth=16)
    exp_pin = oracle.render(cam, sc, opts)[0]
    exp_lens = oracle.render(cam, sc, opts, lens=lens)[0]
    with hip.HipScene(sc) as hs:
        info = hs.info()
        assert info["lds_bytes_per_wave"] == lds, (info, pick)
        assert info["trace_waves"] == info["n_cus"] * (LDS_CU // lds), info
        print(f"{ns} spheres, {nt} triangles: {lds} B per wave ({LDS_CU // lds} waves per CU), a lens launch "
              f"{lds + 32} B ({LDS_CU // (lds + 32)})")
        for lens_, exp in ((None, exp_pin), (lens, exp_lens), (lens, exp_lens), (None, exp_pin)):
            out = frame(torch, cam)
            hs.render_device(cam, opts, out.data_ptr(), lens=lens_)
            same_frame(torch, out, exp, f"lens={lens_ is not None}")
        hs.set_pipeline(3)
        outs = [frame(torch, cam) for _ in range(4)]
        for k, o in enumerate(outs):
            hs.render_device(cam, opts, o.data_ptr(), lens=lens if k % 2 else None)
        for k, o in enumerate(outs):
            same_frame(torch, o, exp_lens if k % 2 else exp_pin, f"stream frame {k}")
        hs.check()


# ---- every entry point and schedule on one scene with everything -----------------------------------------------------------------
W, H, SPP, SEED = 44, 30, 5, 6


@pytest.fixture(scope="module")
def full(oracle):
    cam, lens = F.all_features_camera(oracle, W, H)
    sc = F.all_features_scene(oracle)
    opts = F.all_features_opts(SPP, SEED)
    exp, exp8, _ = oracle.render(cam, sc, opts, lens=lens)
    assert (exp > 1.0).any()
    return cam, lens, sc, opts, exp, exp8


def test_every_entry_point_on_the_full_scene(hip, full):
    import torch
    cam, lens, sc, opts, exp, exp8 = full
    got, got8 = hip.render_scene(cam, SPP, sc, seed=SEED, lens=lens, **opts_kw(opts))
    assert_same_image(got, exp, "render_shaded")
    assert np.array_equal(got8, exp8)
    with hip.HipScene(sc) as hs:
        out, out8 = frame(torch, cam), torch.zeros((H, W, 3), dtype=torch.uint8, device="cuda")
        hs.render_device(cam, opts, out.data_ptr(), out8.data_ptr(), lens=lens)
        same_frame(torch, out, exp, "render_device")
        assert np.array_equal(out8.cpu().numpy(), exp8)
        for cuts in ((0, 1, 4, 5), (0, 3, 5), (0, 2, 3, 5)):
            acc, out = frame(torch, cam), frame(torch, cam)
            for b, e in zip(cuts[:-1], cuts[1:]):
                hs.render_pass(cam, opts, b, e, acc.data_ptr(), out.data_ptr() if e == SPP else None, lens=lens)
            same_frame(torch, out, exp, f"render_pass {cuts}")
        world = 3
        slot = hip.packed_pixels(W, H, 0, world)
        slots = torch.full((world * slot * 3,), float("nan"), dtype=torch.float32, device="cuda")
        for r in range(world):
            hs.render_device(cam, copy_opts(opts, tile_rank=r, tile_world=world), slots[r * slot * 3:].data_ptr(), lens=lens)
        merged = frame(torch, cam)
        hip.unpack_tiles(0, slots.data_ptr(), W, H, world, merged.data_ptr(), None, None, rank_stride_pixels=slot)
        same_frame(torch, merged, exp, "tile_world 3 + unpack_tiles")
        out = frame(torch, cam)
        hs.render_device(cam, copy_opts(opts, flags=opts.flags | abi.FLAG_COLLECT_STATS), out.data_ptr(), lens=lens)
        same_frame(torch, out, exp, "COLLECT_STATS")
        assert hs.stats()["samples"] == W * H * SPP
        hs.set_pipeline(4)
        outs = [frame(torch, cam) for _ in range(9)]
        for k in range(4):  # a stream of frames
            hs.render_device(cam, opts, outs[k].data_ptr(), lens=lens)
        torch.cuda.synchronize()
        for k in (4, 5):  # blocking frames
            hs.render_device(cam, opts, outs[k].data_ptr(), lens=lens)
            torch.cuda.synchronize()
        for k in range(6, 9):  # and a stream again
            hs.render_device(cam, opts, outs[k].data_ptr(), lens=lens)
        for k, o in enumerate(outs):
            same_frame(torch, o, exp, f"pipeline 4, frame {k}")
        hs.check()


def test_sample_batches_under_a_small_workspace(hip, oracle, full, monkeypatch):
    import torch
    _, _, sc, opts, _, _ = full
    cam, lens = F.all_features_camera(oracle, 320, 240)  # 320 x 240 x 12 B per sample: one sample per batch in 1 MiB
    o = F.all_features_opts(3, SEED)
    exp, _, _ = oracle.render(cam, sc, o, lens=lens, want_rgb8=False, col_stride=5)
    monkeypatch.setenv("RBRT_HIP_WORKSPACE_MB", "1")
    out = frame(torch, cam)
    with hip.HipScene(sc) as hs:
        hs.render_device(cam, o, out.data_ptr(), lens=lens)
        torch.cuda.synchronize()
        assert hs.last_batches()[1] >= 2, hs.last_batches()
        hs.check()
    assert_same_image(np.ascontiguousarray(out.cpu().numpy()[:, ::5]), np.ascontiguousarray(exp[:, ::5]), "batches")


ENVS = [
    ("helpers_2", {"RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": "1", "RBRT_HELPER_MIN_LAUNCH_MI": "0", "RBRT_HELPER_MIN_FREE": "1"}),
    ("share_idle_0", {"RBRT_SHARE_IDLE": "0"}),
    ("share_idle_1", {"RBRT_SHARE_IDLE": "1"}),
    ("share_idle_48", {"RBRT_SHARE_IDLE": "48"}),
    ("share_idle_1_lds_stack_1", {"RBRT_SHARE_IDLE": "1", "RBRT_LDS_STACK": "1"}),
    ("tile_pass_off", {"RBRT_PRIMARY_CULL": "0"}),
    ("refined_after_device", {"RBRT_BVH_DEVICE_MIN": "0"}),
]


@pytest.mark.parametrize("rid,env", ENVS, ids=[e[0] for e in ENVS])
def test_schedules_on_the_full_scene(hip, full, monkeypatch, rid, env):
    import torch
    cam, lens, sc, opts, exp, _ = full
    K._set_env(monkeypatch, env)
    monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    monkeypatch.delenv("RBRT_BVH_REFINE", raising=False)
    with hip.HipScene(sc) as hs:
        if rid == "refined_after_device":
            assert hs.create_times()["meshes_device_built"] == len(sc.meshes)
            out = frame(torch, cam)
            hs.render_device(cam, opts, out.data_ptr(), lens=lens)
            same_frame(torch, out, exp, "device builder's trees")
            assert hs.refine_wait(120.0)[0] == 1
        out = frame(torch, cam)
        hs.render_device(cam, opts, out.data_ptr(), lens=lens)
        same_frame(torch, out, exp, f"{rid}: blocking frame")
        hs.set_pipeline(3)
        hs.set_timing(True)
        outs = [frame(torch, cam) for _ in range(4)]
        for o in outs:
            hs.render_device(cam, opts, o.data_ptr(), lens=lens)
        for k, o in enumerate(outs):
            same_frame(torch, o, exp, f"{rid}: stream frame {k}")
        hs.render_device(cam, copy_opts(opts, flags=opts.flags | abi.FLAG_COLLECT_STATS), out.data_ptr(), lens=lens)
        same_frame(torch, out, exp, f"{rid}: counting frame")
        if rid.startswith("share_idle") and env["RBRT_SHARE_IDLE"] == "0":
            assert hs.debug_counters()["shared_entries_given"] == 0
        hs.check()


@pytest.fixture(scope="module")
def knob_refs(oracle, full):
    cam, lens, sc, opts, _, _ = full
    return {seed: oracle.render(cam, sc, copy_opts(opts, seed=seed), lens=lens)[0] for seed in (K.SEED,) + K.STREAM_SEEDS}


@pytest.mark.parametrize("rid,env,effect", K.MATRIX, ids=[r[0] for r in K.MATRIX])
def test_knob_rows_on_the_full_scene(hip, full, knob_refs, monkeypatch, rid, env, effect):
    """test_lab_knobs.MATRIX's rows on the scene with every feature: a blocking frame, a stream of four, a counting frame;
    the rows' several-batches and rank-of-three cases too."""
    import torch
    cam, lens, sc, opts, _, _ = full
    flags = K.FLAGS.get(rid, set())
    K._set_env(monkeypatch, env)
    with hip.HipScene(sc) as hs:
        hs.refine_wait(60.0)
        out = frame(torch, cam)
        hs.render_device(cam, copy_opts(opts, seed=K.SEED), out.data_ptr(), lens=lens)
        same_frame(torch, out, knob_refs[K.SEED], f"{rid}: blocking frame")
        if "own_pipeline" not in flags:
            hs.set_pipeline(3)
        outs = [frame(torch, cam) for _ in K.STREAM_SEEDS]
        for o, seed in zip(outs, K.STREAM_SEEDS):
            hs.render_device(cam, copy_opts(opts, seed=seed), o.data_ptr(), lens=lens)
        for o, seed in zip(outs, K.STREAM_SEEDS):
            same_frame(torch, o, knob_refs[seed], f"{rid}: stream frame of seed {seed}")
        hs.render_device(cam, copy_opts(opts, seed=K.SEED, flags=opts.flags | abi.FLAG_COLLECT_STATS), out.data_ptr(), lens=lens)
        same_frame(torch, out, knob_refs[K.SEED], f"{rid}: counting frame")
        if "rank" in flags:  # tiles of rank 1 of 3 (the one-shot call)
            part, _ = hip.render_scene(cam, opts.spp, sc, seed=K.SEED, lens=lens, tile_rank=1, tile_world=3, **opts_kw(opts))
            ty, tx = np.meshgrid(np.arange(H) // 8, np.arange(W) // 8, indexing="ij")
            mine = (tiles.tile_number(ty, tx, (W + 7) // 8) % 3) == 1
            assert_same_image(part[mine][None], knob_refs[K.SEED][mine][None], f"{rid}: rank 1 of 3")
        hs.check()


# ---- the shipped feature scenes through the product's host path -----------------------------------------------------------------
KINDS = {"lambertian": abi.MAT_LAMBERTIAN, "metal": abi.MAT_METAL, "dielectric": abi.MAT_DIELECTRIC, "emissive": abi.MAT_EMISSIVE}
N_TRIS = 2000


def _v(d):
    return (float(d["x"]), float(d["y"]), float(d["z"]))


def _mat(b):
    k = next(v for name, v in KINDS.items() if name in b["material_type"])
    return abi.material(k, _v(b["albedo"]) if "albedo" in b else (0.0, 0.0, 0.0), float(b.get("material_param", 0.0)))


def oracle_scene(oracle, cfg, w, h):
    """The scene of a shipped YAML prepared by the oracle and the numpy restatements: (camera, lens or None, SceneData).
    The mesh is the stand-in of N_TRIS triangles; `shading: smooth` gives it the host's area-weighted normals
    (np_smooth.area_weighted)."""
    y = yaml.safe_load(cfg.read_text())
    c = y["camera_blueprint"]
    look = _v(c["camera_look_at"])
    cam = scenes.camera(oracle, w, h, position=_v(c["camera_position"]), look_at=look, up=_v(c["camera_up"]),
                        focal_mm=float(c["camera_focal_length_mm"]))
    lens = None
    if float(c.get("camera_aperture_mm", 0.0)) > 0.0:
        lens = np_lens.lens_for(cam, look, float(c["camera_focal_length_mm"]), float(c["camera_aperture_mm"]),
                                float(c["camera_focus_distance"]))
    spheres = [(_v(s["center"]), float(s["radius"]), _mat(s)) for s in y.get("sphere_blueprints") or []]
    meshes = []
    for m in y.get("mesh_blueprints") or []:
        assert _v(m["rotation_rad"]) == (0.0, 0.0, 0.0)
        if m.get("shading") == "smooth":
            meshes.append(np_smooth.standin_smooth(oracle, N_TRIS, float(m["scale"]), _v(m["translation"]), _mat(m), "computed"))
        else:
            meshes.append(scenes.standin_mesh(oracle, N_TRIS, float(m["scale"]), _v(m["translation"]), (0.0, 0.0, 0.0), _mat(m)))
    return cam, lens, abi.SceneData(spheres=spheres, meshes=meshes)


def host_scene(tmp_path, which, w, h):
    v, f = standin.make_mesh(N_TRIS)
    standin.write_obj(tmp_path / "bunny.obj", v, f)
    (tmp_path / "scene.yaml").write_text((ROOT / "scenes" / which).read_text().replace("bunny.obj", str(tmp_path / "bunny.obj")))
    return abi.HostScene(tmp_path / "scene.yaml", h, w)


FEATURE_SCENES = {"emissive_spheres.yaml": dict(flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0)),
                  "defocus_spheres.yaml": {}, "smooth_mesh.yaml": {}}


@pytest.mark.parametrize("which", list(FEATURE_SCENES))
def test_shipped_feature_scenes_through_the_host(hip, oracle, tmp_path, which):
    w, h, spp, seed = 150, 92, 4, 12
    kw = FEATURE_SCENES[which]
    hs = host_scene(tmp_path, which, w, h)
    got, got8 = hip.render_scene(hs.camera, spp, hs, seed=seed, lens=hs.lens, **kw)
    cam, lens, sc = oracle_scene(oracle, ROOT / "scenes" / which, w, h)
    assert (hs.lens is None) == (lens is None)
    assert (hs.shading is None) == all(m.normals is None for m in sc.meshes)
    exp, exp8, _ = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=seed, **kw), lens=lens)
    assert_same_image(got, exp, which)
    assert np.array_equal(got8, exp8)
    # the host's scene through the oracle is the same image (the host prepared what the oracle prepared)
    assert_same_image(oracle.render(hs.camera, hs, abi.default_opts(spp=spp, seed=seed, **kw), lens=hs.lens)[0], exp, f"{which} host")


def test_smooth_mesh_scene_at_full_size(hip, oracle, tmp_path):
    """smooth_mesh.yaml at 1024 x 768 through the host, every 64th column against the oracle."""
    w, h, spp, seed, stride = 1024, 768, 3, 2, 64
    hs = host_scene(tmp_path, "smooth_mesh.yaml", w, h)
    got, _ = hip.render_scene(hs.camera, spp, hs, seed=seed)
    cam, lens, sc = oracle_scene(oracle, ROOT / "scenes" / "smooth_mesh.yaml", w, h)
    exp, _, _ = oracle.render(cam, sc, abi.default_opts(spp=spp, seed=seed), want_rgb8=False, col_stride=stride)
    assert_same_image(np.ascontiguousarray(got[:, ::stride]), np.ascontiguousarray(exp[:, ::stride]), "smooth_mesh.yaml 1024x768")
