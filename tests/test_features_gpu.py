"""The feature buffers on the GPU (rbrt_hip_render_features) against the numpy restatement (np_features.py, pinned by
test_np_features.py), bit for bit: every output, every size at which the kernel's tiling changes, pinhole and lens, spheres,
BasicTriangles in a mixed element order, flat and smooth meshes. Then the identity that ties the buffers to the renderer (a
scene of emitters renders to its albedo buffer), which outputs are written, what the result may depend on, that the handle is
left as it was, the refusals, and the CLI's four files."""
from __future__ import annotations

import itertools
import json
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import full_scenes
import np_features as F
import np_lens
import np_smooth
import scenes
from rbrt_amd import abi, standin

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
EXE = ROOT / "rbrt_amd" / "bin" / "rbrt"
f32 = np.float32
NAMES = ("albedo", "normal", "depth", "coverage", "object")
CHANNELS = dict(albedo=3, normal=3, depth=1, coverage=1, object=1)
POISON = 0x7FC0BEEF  # as a float: a NaN no kernel writes
GUARD = 64           # poisoned words behind every buffer
SIZES = [(1, 1), (8, 8), (37, 21), (64, 48)]  # one lane; one whole tile; ragged both ways; 48 waves
NS = (1, 2, 5)
SEED = 7


# ---- the scenes and their restated buffers, made once ---------------------------------------------------------------------------
def make_scene(oracle, which):
    if which == "spheres":  # all four materials
        return abi.SceneData(spheres=list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(abi.MAT_EMISSIVE, (3.0, 2.5, 1.5)))])
    if which == "triangles":  # BasicTriangles interleaved with the spheres, and a flat mesh of 203 entries
        return scenes.triangle_scene(oracle, 203)
    # a flat and a smooth stand-in, N % 8 = 3 both: the truncated tail is in play, and the device builder takes them
    flat = scenes.standin_mesh(oracle, 1203, **scenes.EXAMPLE_MESH)
    smooth = np_smooth.standin_smooth(oracle, 2003, 30.0, (-1.0, -1.3, -6.5), abi.material(abi.MAT_METAL, (0.8, 0.8, 0.75), 0.05), "computed")
    return abi.SceneData(spheres=scenes.EXAMPLE_SPHERES[:1], meshes=[flat, smooth])


def lens_of(cam):
    return np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 20.0, 9.0)


class Refs:
    """The rays of max(NS) samples per (size, camera) and their hits per scene, shared by every test and never changed."""

    def __init__(self, oracle):
        self.oracle, self.scenes, self.rays, self.hits = oracle, {}, {}, {}

    def scene(self, which):
        if which not in self.scenes:
            self.scenes[which] = make_scene(self.oracle, which) if which != "emitters" else F.emitter_scene(self.oracle)
        return self.scenes[which]

    def case(self, which, w, h, lensed, seed=SEED):
        cam = scenes.camera(self.oracle, w, h)
        lens = lens_of(cam) if lensed else None
        sc = self.scene(which)
        opts = abi.default_opts(spp=3, seed=seed)
        rk = (w, h, lensed, seed)
        if rk not in self.rays:
            self.rays[rk] = F.primary_rays(cam, seed, max(NS), lens)
            self.rays[rk].flags.writeable = False
        hk = (which,) + rk
        if hk not in self.hits:
            self.hits[hk] = F.hits(self.oracle, sc, self.rays[rk], opts.min_dist, opts.max_dist)
        return SimpleNamespace(cam=cam, lens=lens, sc=sc, opts=opts, w=w, h=h, hits=self.hits[hk])

    def expected(self, c, n):
        return F.scatter_pixels(F.from_hits(c.sc, *c.hits, n), F.all_pixels(c.cam), c.h, c.w)


@pytest.fixture(scope="module")
def refs(oracle):
    return Refs(oracle)


# ---- one call, with poisoned buffers and guard words ------------------------------------------------------------------------------
def call(hs, torch, cam, opts, n, lens=None, want=NAMES, expect=None, **kw):
    """rbrt_hip_render_features into poisoned buffers: {name: array} of the outputs asked for. Buffers not asked for and the
    guard words behind every buffer must keep their poison. expect: the error code the call must fail with (every buffer
    then keeps its poison)."""
    w, h = cam.img_width_pix, cam.img_height_pix
    bufs = {k: torch.full((w * h * CHANNELS[k] + GUARD,), POISON, dtype=torch.int32, device="cuda") for k in NAMES}
    ptrs = {f"d_{k}": bufs[k].data_ptr() for k in want}
    if expect is None:
        hs.render_features(cam, opts, n, lens=lens, **ptrs, **kw)
    else:
        with pytest.raises(abi.RbrtError) as e:
            hs.render_features(cam, opts, n, lens=lens, **ptrs, **kw)
        assert e.value.code == expect, (e.value, expect)
        want = ()
    torch.cuda.synchronize()
    out = {}
    for k in NAMES:
        a = bufs[k].cpu().numpy()
        size = w * h * CHANNELS[k]
        assert (a[size:] == POISON).all(), f"guard words behind {k}"
        if k not in want:
            assert (a[:size] == POISON).all(), f"{k} was not asked for"
        elif k == "object":
            out[k] = a[:size].reshape(h, w).copy()
        else:
            out[k] = a[:size].view(f32).reshape((h, w, 3) if CHANNELS[k] == 3 else (h, w)).copy()
    return out


def assert_same(got, exp, what):
    for k in got:
        e = getattr(exp, k) if not isinstance(exp, dict) else exp[k]
        if k == "object":
            assert np.array_equal(got[k], e), (what, k)
        else:
            assert full_scenes.same_bits(got[k], e), (what, k, int((got[k].view(np.uint32) != np.asarray(e, f32).view(np.uint32)).sum()))


# ---- 1. every output against the restatement ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
@pytest.mark.parametrize("which", ["spheres", "triangles", "meshes"])
def test_all_five_outputs_are_the_restatement(hip, refs, which, w, h, lensed):
    import torch
    c = refs.case(which, w, h, lensed)
    with hip.HipScene(c.sc) as hs:
        for n in NS:
            got = call(hs, torch, c.cam, c.opts, n, c.lens)
            assert set(got) == set(NAMES)
            assert_same(got, refs.expected(c, n), f"{which} {w}x{h} n={n} lens={lensed}")
        hs.check()
    if (w, h) == (64, 48):  # the scene is in view: every kind of object, the sky, and pixels on an edge
        exp = refs.expected(c, 5)
        n_obj = len(c.sc.spheres) + len(c.sc.triangles) + len(c.sc.meshes)
        seen = set(np.unique(exp.object).tolist())
        assert -1 in seen and len(seen) >= min(n_obj, 4) + 1 and max(seen) == n_obj - 1, seen
        assert ((exp.coverage > 0) & (exp.coverage < 1)).any()


# ---- 2. the identity that ties the buffers to the renderer ---------------------------------------------------------------------------
@pytest.mark.parametrize("lensed", [False, True], ids=["pinhole", "lens"])
def test_an_emitters_only_scene_renders_to_its_albedo_buffer(hip, refs, lensed):
    import torch
    c = refs.case("emitters", 37, 21, lensed, seed=3)
    with hip.HipScene(c.sc) as hs:
        for n in NS:
            opts = F.emitter_opts(n, seed=3)
            rad = torch.full((21, 37, 3), float("nan"), dtype=torch.float32, device="cuda")
            hs.render_device(c.cam, opts, rad.data_ptr(), lens=c.lens)
            got = call(hs, torch, c.cam, opts, n, c.lens)
            assert full_scenes.same_bits(rad.cpu().numpy(), got["albedo"]), (n, lensed)
            assert_same(got, refs.expected(c, n), f"emitters n={n}")
        assert got["albedo"].max() > 4.0 and (got["coverage"] == 0).any()
        hs.check()


# ---- 3. which outputs are written ------------------------------------------------------------------------------------------------------
def test_each_output_alone_and_every_pair(hip, refs):
    import torch
    c = refs.case("triangles", 37, 21, False)
    with hip.HipScene(c.sc) as hs:
        full = call(hs, torch, c.cam, c.opts, 2)
        for want in list(itertools.combinations(NAMES, 1)) + list(itertools.combinations(NAMES, 2)):
            got = call(hs, torch, c.cam, c.opts, 2, want=want)
            assert set(got) == set(want)
            assert_same(got, full, want)
        assert call(hs, torch, c.cam, c.opts, 2, want=()) == {}  # every output NULL: RBRT_OK, nothing written
        hs.check()


# ---- 4. what the result may depend on ---------------------------------------------------------------------------------------------------
def test_what_the_result_depends_on(hip, refs):
    import torch
    c = refs.case("triangles", 37, 21, True)
    with hip.HipScene(c.sc) as hs:
        base = call(hs, torch, c.cam, c.opts, 5, c.lens)
        assert_same(base, refs.expected(c, 5), "base")
        others = dict(spp=abi.default_opts(spp=64, seed=SEED), depth=abi.default_opts(spp=3, seed=SEED, max_depth=0),
                      bg=abi.default_opts(spp=3, seed=SEED, bg=(9.0, 0.0, 2.0)),
                      constant=abi.default_opts(spp=3, seed=SEED, flags=abi.FLAG_CONSTANT_BACKGROUND, bg=(0.0, 0.0, 0.0)))
        for what, o in others.items():
            assert_same(call(hs, torch, c.cam, o, 5, c.lens), base, what)
        hs.set_environment(np.full((3, 3, 3), 0.5, f32))
        assert_same(call(hs, torch, c.cam, c.opts, 5, c.lens), base, "environment")
        hs.set_environment(None)
        one = call(hs, torch, c.cam, c.opts, 1, c.lens)
        assert np.array_equal(one["object"], base["object"])  # sample 0's, whatever n
        other = call(hs, torch, c.cam, abi.default_opts(spp=3, seed=SEED + 1), 5, c.lens)
        edge = (base["coverage"] > 0) & (base["coverage"] < 1)  # pixels on a silhouette: their samples disagree
        assert edge.any() and (other["albedo"][edge] != base["albedo"][edge]).any()
        hs.check()


# ---- 5. the handle is left as it was ------------------------------------------------------------------------------------------------------
def test_renders_around_a_features_call_are_identical(hip, refs):
    import torch
    c = refs.case("meshes", 64, 48, False)
    opts = abi.default_opts(spp=4, seed=SEED, max_depth=8)
    with hip.HipScene(c.sc) as hs:
        frames = [torch.full((48, 64, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(3)]
        hs.render_device(c.cam, opts, frames[0].data_ptr())
        call(hs, torch, c.cam, c.opts, 2)
        hs.render_device(c.cam, opts, frames[1].data_ptr())
        hs.render_features(c.cam, c.opts, 2)  # (nothing asked for)
        hs.render_device(c.cam, opts, frames[2].data_ptr())
        torch.cuda.synchronize()
        a = frames[0].cpu().numpy()
        assert not np.isnan(a).any()
        assert full_scenes.same_bits(a, frames[1].cpu().numpy()) and full_scenes.same_bits(a, frames[2].cpu().numpy())
        # the adaptive sums the denoiser reads
        hs.render_adaptive(c.cam, opts, 0.05, 2, 2)
        den = [torch.full((48, 64, 3), float("nan"), dtype=torch.float32, device="cuda") for _ in range(2)]
        hs.denoise(den[0].data_ptr(), window_radius=2, patch_radius=1)
        assert_same(call(hs, torch, c.cam, c.opts, 5), refs.expected(c, 5), "after an adaptive render")
        hs.denoise(den[1].data_ptr(), window_radius=2, patch_radius=1)
        torch.cuda.synchronize()
        assert not np.isnan(den[0].cpu().numpy()).any() and full_scenes.same_bits(den[0].cpu().numpy(), den[1].cpu().numpy())
        hs.check()


def test_the_result_does_not_depend_on_the_tree(hip, refs, monkeypatch):
    import torch
    monkeypatch.setenv("RBRT_BVH_DEVICE_MIN", "0")  # every mesh starts with the device builder's tree
    monkeypatch.delenv("RBRT_BVH_BUILDER", raising=False)
    monkeypatch.delenv("RBRT_BVH_REFINE", raising=False)
    c = refs.case("meshes", 64, 48, True)
    with hip.HipScene(c.sc) as hs:
        assert hs.create_times()["meshes_device_built"] == len(c.sc.meshes)
        before = call(hs, torch, c.cam, c.opts, 5, c.lens)
        assert hs.refine_wait(120.0)[0] == 1  # the host builder's trees are in use now
        after = call(hs, torch, c.cam, c.opts, 5, c.lens)
        assert_same(after, before, "after refine_wait")
        assert_same(before, refs.expected(c, 5), "device builder's trees")
        hs.check()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(hip, refs):
    import torch
    c = refs.case("spheres", 8, 8, False)
    O = abi.default_opts
    nan = float("nan")
    with hip.HipScene(c.sc) as hs:
        call(hs, torch, c.cam, O(seed=SEED, tile_rank=1, tile_world=2), 2, expect=abi.RBRT_ERR_UNSUPPORTED)
        call(hs, torch, c.cam, O(seed=SEED, tile_rank=0, tile_world=2), 2, expect=abi.RBRT_ERR_UNSUPPORTED)
        rows = {
            "samples 0": dict(n=0), "samples 65537": dict(n=65537),
            "reserved[0]": dict(reserved=(1, 0, 0)), "reserved[1]": dict(reserved=(0, 1, 0)), "reserved[2]": dict(reserved=(0, 0, 1)),
            "collect stats": dict(opts=O(seed=SEED, flags=abi.FLAG_COLLECT_STATS)),
            "tile_rank": dict(opts=O(seed=SEED, tile_rank=3, tile_world=2)),
            "lens_u nan": dict(lens=((nan, 0.0, 0.0), (0.0, 0.1, 0.0), 300.0)),
            "focus_scale 0": dict(lens=((0.1, 0.0, 0.0), (0.0, 0.1, 0.0), 0.0)),
            "focus_scale inf": dict(lens=((0.1, 0.0, 0.0), (0.0, 0.1, 0.0), float("inf"))),
        }
        for what, r in rows.items():
            kw = dict(reserved=r["reserved"]) if "reserved" in r else {}
            call(hs, torch, c.cam, r.get("opts", c.opts), r.get("n", 2), r.get("lens"), expect=abi.RBRT_ERR_INVALID_ARG, **kw)
        zero = abi.Camera()
        zero.img_width_pix, zero.img_height_pix = 0, 8
        with pytest.raises(abi.RbrtError) as e:
            hs.render_features(zero, c.opts, 2)
        assert e.value.code == abi.RBRT_ERR_INVALID_ARG
        assert_same(call(hs, torch, c.cam, c.opts, 2), refs.expected(c, 2), "after the refusals")  # the handle still works
        hs.check()


def test_a_nan_discriminant_is_reported_by_scene_check(hip, oracle):
    import torch
    cam = scenes.camera(oracle, 8, 8)
    bad = list(scenes.EXAMPLE_SPHERES)
    c, r, m = bad[1]
    bad[1] = ((float("nan"), c[1], c[2]), r, m)  # every ray sees a NaN discriminant on this sphere
    sc = scenes.spheres_scene(bad)
    with hip.HipScene(sc) as hs:
        got = call(hs, torch, cam, abi.default_opts(seed=1), 2)
        assert not (got["object"] == 1).any() and (got["coverage"] > 0).any()  # those rays miss that sphere, and only that one
        with pytest.raises(abi.RbrtError) as e:
            hs.check()
        assert e.value.code == abi.RBRT_ERR_NAN
        hs.check()  # (reported once)


# ---- 7. the CLI -----------------------------------------------------------------------------------------------------------------------------
def read_pfm(path):
    """A colour PFM in numpy: float32 (H, W, 3), top row first."""
    raw = Path(path).read_bytes()
    magic, size, scale, body = raw.split(b"\n", 3)
    assert magic == b"PF" and float(scale) < 0  # colour, little-endian
    w, h = (int(x) for x in size.split())
    assert len(body) == w * h * 12
    return np.frombuffer(body, "<f4").reshape(h, w, 3)[::-1].copy()


def test_cli_writes_the_four_files(hip, tmp_path):
    import torch
    w, h, spp, seed = 53, 29, 2, 3
    v, f = standin.make_mesh(203)
    standin.write_obj(tmp_path / "bunny.obj", v, f)
    cfg = tmp_path / "scene.yaml"
    cfg.write_text((ROOT / "scenes" / "smooth_mesh.yaml").read_text().replace("bunny.obj", str(tmp_path / "bunny.obj")))
    prefix, rep = tmp_path / "feat", tmp_path / "report.json"
    argv = [str(EXE), "-c", str(cfg), "-t", str(tmp_path / "out.png"), "--height", str(h), "-w", str(w), "-s", str(spp), "--seed", str(seed),
            "--features", str(prefix), "--feature-samples", "3", "--report", str(rep)]
    r = subprocess.run(argv, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    js = json.loads(rep.read_text())
    assert js["features"]["samples"] == 3 and js["features"]["ms"] > 0
    files = {k: read_pfm(f"{prefix}.{k}.pfm") for k in NAMES[:4]}
    host = abi.HostScene(cfg, h, w)
    with hip.HipScene(host) as hs:
        got = call(hs, torch, host.camera, abi.default_opts(spp=spp, seed=seed), 3, host.lens)
    for k in ("albedo", "normal"):
        assert full_scenes.same_bits(files[k], got[k]), k
    for k in ("depth", "coverage"):
        for ch in range(3):
            assert full_scenes.same_bits(files[k][..., ch], got[k]), (k, ch)
    assert (got["coverage"] > 0).any() and (got["coverage"] == 0).any() and (got["object"].max() >= 1)
    # without the flags: no files, no report entry; the default is min(--samples, 8)
    r = subprocess.run([str(EXE), "-c", str(cfg), "-t", str(tmp_path / "b.png"), "--height", "16", "-w", "16", "-s", "12", "--report", str(rep),
                        "--features", str(tmp_path / "g")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(rep.read_text())["features"]["samples"] == 8
    r = subprocess.run([str(EXE), "-c", str(cfg), "-t", str(tmp_path / "c.png"), "--height", "16", "-w", "16", "-s", "1", "--report", str(rep)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "features" not in json.loads(rep.read_text())
