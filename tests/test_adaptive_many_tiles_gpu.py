"""Adaptive sampling beyond one tile per lane, and an adaptive state that grows and shrinks on one handle.

adaptive_lists_kernel is one wave: lane t owns the run [t * per, (t + 1) * per) of the rank's tiles, per = ceil(n / 64).
test_adaptive_gpu.py's mixed cases have 15 tiles (per = 1, no run mixes classes, 49 lanes empty). The cases here have 64,
65, 153 and 357 tiles (119 a rank of three): runs of 2, 3 and 6 tiles that hold active, inactive and background-only tiles
side by side, lanes behind the last run, and later rounds whose grids -- sized by the count of active tiles the host read
back -- are far smaller than the image. np_lists.py restates the runs and the classes; the conditions the cases have to
meet are asserted from the restatement and the culling table alone (test_the_inputs_meet_their_conditions).

Every case: N = 12, the first round 4, every later round 4: three rounds. Per-sample radiance, thresholds and expected
results are made as in test_adaptive_gpu.py, once per module. Everything is compared bit for bit."""
from __future__ import annotations

import os
import subprocess
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import np_adaptive as A
import np_denoise as D
import np_lists as L
import scenes
import test_adaptive_gpu as T
from rbrt_amd import tiles
from test_adaptive_gpu import bits, run_adaptive
from test_denoise_gpu import run_denoise

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
N, MIN, STEP = 12, 4, 4
# t153_ragged: the example camera turned up and rolled, so that the horizon crosses the tile rows at a slant: tile rows
# that hold background-only tiles and others side by side
RAGGED_VIEW = dict(look_at=(-2.0, 2.5, -10.0), up=(1.0, 1.0, -0.4))

#        id             scene      W    H
CASES = [("t64", "spheres", 64, 64),           # 64 tiles: every lane exactly one
         ("t65", "spheres", 104, 40),          # 13 x 5 = 65: per = 2, the last run has one tile, 31 lanes own nothing
         ("t153_ragged", "spheres", 131, 67),  # 17 x 9 = 153: per = 3, ragged both ways, both lists populated
         ("t153_full", "full", 131, 67),       # every feature, thin lens
         ("t357", "spheres", 168, 136)]        # 21 x 17 = 357: per = 6; a rank of three has 119: per = 2
# ... and the two 15-tile cases of test_adaptive_gpu.py the handle of section 2 starts with and shrinks to
SMALL = [("spheres_40x24", "spheres", 40, 24), ("spheres_37x21", "spheres", 37, 21)]
IDS = [c[0] for c in CASES]
KINDS = ("zero", "median", "half_median")
# the cases whose half images and denoised images are needed: those a handle denoises (sections 1 and 2)
DENOISED = ("spheres_40x24", "t153_ragged", "spheres_37x21", "t357", "t65")
OTHER_PARAMS = dict(window_radius=2, patch_radius=1, strength=1.0)


def build_case(oracle, cid, scene, w, h):
    """test_adaptive_gpu.build, with t153_ragged's own camera."""
    cam, lens, sc, opts_of = T.build(oracle, scene, w, h)
    if cid == "t153_ragged":
        cam = scenes.camera(oracle, w, h, **RAGGED_VIEW)
    return SimpleNamespace(cid=cid, scene=scene, w=w, h=h, n=N, mn=MIN, step=STEP, cam=cam, lens=lens, sc=sc, opts_of=opts_of)


def denoise_reference(samples, r, **params):
    """The restated half images of an adaptive result and their denoised image."""
    S, S_even = D.halves_from_samples(samples, r.counts)
    a, b, wa = D.halves(S, S_even, r.counts)
    img, rgb8 = D.denoise(a, b, wa, **params)
    return SimpleNamespace(a=a, b=b, wa=wa, image=img, rgb8=rgb8)


@pytest.fixture(scope="module")
def data(hip, oracle):
    """Per case: scene, per-sample radiance, the culling table, the restatement's results for the thresholds and, where a
    handle is denoised, the restated half images and denoised images. Made once, never changed."""
    import torch
    t0 = time.perf_counter()
    d = {}
    for cid, scene, w, h in CASES + SMALL:
        c = build_case(oracle, cid, scene, w, h)
        with hip.HipScene(c.sc) as hs:
            samples = T.extract_samples(hs, torch, c.cam, c.lens, c.opts_of, N)
            c.cull = hs.primary_cull(c.cam, c.opts_of(N), c.lens)  # uint32 [tiles_y, tiles_x]
            hs.check()
        r0 = A.adaptive(samples, 0.0, MIN, STEP)
        med = f32(np.median(r0.round_errors[0]))
        c.thr = dict(zero=0.0, huge=T.HUGE, median=float(med), half_median=float(f32(0.5) * med))
        c.rest = {k: r0 if k == "zero" else A.adaptive(samples, t, MIN, STEP) for k, t in c.thr.items()}
        c.den, c.den_other = {}, {}
        if cid in DENOISED:
            c.den = {k: denoise_reference(samples, c.rest[k]) for k in ("zero", "median")}
        if cid in ("t153_ragged", "t357"):
            c.den_other = {"median": denoise_reference(samples, c.rest["median"], **OTHER_PARAMS)}
        samples.flags.writeable = False
        c.samples = samples
        d[cid] = c
    print(f"fixture: samples, restatements and denoised references of {len(d)} cases in {time.perf_counter() - t0:.2f} s")
    return d


def local(c, tile_array, rank=0, world=1):
    return A.per_rank(tile_array, rank, world)


def expected_rounds(counts_local):
    """Tiles active at the start of each round, from the final counts: the rounds end with the first that has none."""
    per_round = [int((counts_local >= n_k).sum()) for n_k in L.schedule(N, MIN, STEP)]
    return [a for a in per_round if a > 0]


def round_classes(c, kind, rank=0, world=1, cull=True):
    """Per round of the case at the threshold: the class of every local tile (np_lists), from the restatement's final counts
    and the culling table."""
    counts = local(c, c.rest[kind].counts, rank, world)
    words = local(c, c.cull, rank, world) if cull else None
    return [L.classes(counts, words, n_k) for n_k in L.schedule(N, MIN, STEP)]


# ---- 0. the cases are what they are meant to be -------------------------------------------------------------------------------
def test_the_inputs_meet_their_conditions(data):
    """Computed from the restatement and the culling table, never from the adaptive call under test."""
    sched = L.schedule(N, MIN, STEP)
    assert sched == [4, 8, 12]
    for cid, n_tiles in (("t64", 64), ("t65", 65), ("t153_ragged", 153), ("t153_full", 153), ("t357", 357)):
        assert tiles.n_tiles(data[cid].w, data[cid].h) == n_tiles
    assert [tiles.local_tiles(168, 136, r, 3) for r in range(3)] == [119, 119, 119]
    assert [tiles.local_tiles(104, 40, r, 2) for r in range(2)] == [33, 32]
    small_round = False
    for c in data.values():
        for kind in KINDS:
            r = c.rest[kind]
            # a tile is on round k's lists if and only if its final count is at least n_k
            assert set(np.unique(r.counts).tolist()) <= set(sched) and r.rounds == len(r.round_active) <= len(sched)
            assert r.round_active == expected_rounds(local(c, r.counts)), (c.cid, kind)
            for k, n_k in enumerate(sched):
                cls = L.classes(local(c, r.counts), local(c, c.cull), n_k)
                work, sky = L.lists(cls)
                assert len(work) + len(sky) == (r.round_active[k] if k < r.rounds else 0), (c.cid, kind, k)
                # bit 31 of a tile's culling word selects the background list
                words = local(c, c.cull)
                assert (words[sky] >> 31 == 1).all() and (words[work] >> 31 == 0).all()
                if k >= 1 and c.cid in IDS and 0 < len(work) + len(sky) < len(cls) / 2:
                    small_round = True
        assert (c.rest["zero"].counts == N).all() and c.thr["median"] > 0.0 and np.isfinite(c.thr["median"])
        assert len(np.unique(c.rest["median"].counts)) >= 2, (c.cid, c.rest["median"].counts)
    assert small_round  # some later round's grids are sized well under the image
    assert len(np.unique(data["t357"].rest["median"].counts)) >= 3

    def mixed_runs(c, **kw):
        """(runs that hold an active and an inactive tile, runs that hold all three classes), over the rounds after the first."""
        both = three = 0
        for cls in round_classes(c, "median", **kw)[1:]:
            for s in L.run_class_sets(cls):
                both += L.INACTIVE in s and len(s) >= 2
                three += s == {L.WORK, L.SKY, L.INACTIVE}
        return both, three

    ragged, big = data["t153_ragged"], data["t357"]
    work, sky = L.lists(round_classes(ragged, "median")[1])
    assert len(work) > 0 and len(sky) > 0, (len(work), len(sky))  # both lists in round 2
    assert mixed_runs(ragged)[0] >= 1 and mixed_runs(ragged)[1] >= 1, mixed_runs(ragged)
    assert mixed_runs(big)[0] >= 1 and all(mixed_runs(big, rank=r, world=3)[0] >= 1 for r in range(3))
    assert mixed_runs(data["t65"])[0] >= 1
    # t64: one tile a lane, no empty lane; t65: 31 lanes behind the last run
    assert all(hi - lo == 1 for lo, hi in L.runs(64)) and sum(lo == hi == 65 for lo, hi in L.runs(65)) == 31
    for c in data.values():
        print(c.cid, "median", c.thr["median"], "counts", dict(zip(*(x.tolist() for x in np.unique(c.rest["median"].counts, return_counts=True)))),
              "active per round", c.rest["median"].round_active, "| half_median", c.rest["half_median"].round_active)


# ---- 1. adaptive rounds with many tiles ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cid", IDS)
def test_against_the_restatement(hip, data, cid, kind):
    import torch
    c = data[cid]
    r = c.rest[kind]
    with hip.HipScene(c.sc) as hs:
        g = run_adaptive(hs, torch, c, c.thr[kind])
        hs.check()
    what = f"{cid} {kind} threshold {c.thr[kind]!r}"
    assert np.array_equal(g.counts, local(c, r.counts)), (what, g.counts, local(c, r.counts))
    assert np.array_equal(bits(g.errors), bits(local(c, r.errors))), (what, g.errors, local(c, r.errors))
    assert g.res["rounds"] == r.rounds and g.rounds_active == r.round_active, (what, g.res, g.rounds_active, r.round_active)
    assert np.array_equal(bits(g.rad), bits(r.image)), (what, int((bits(g.rad) != bits(r.image)).any(axis=-1).sum()))
    assert np.array_equal(g.rgb, r.rgb8), what
    assert g.res["samples"] == r.samples and g.res["samples_fixed"] == r.samples_fixed == c.w * c.h * N, (what, g.res)


@pytest.mark.parametrize("cid", ["t65", "t153_full"])
def test_every_tile_is_the_fixed_render_at_its_count(hip, oracle, data, cid):
    T.test_every_tile_is_the_fixed_render_at_its_count(hip, oracle, data, cid)


@pytest.mark.parametrize("cid,world", [("t357", 3), ("t65", 2)], ids=["t357_of_3", "t65_of_2"])
def test_the_ranks_of_a_mixed_render_are_the_whole_render(hip, data, cid, world):
    """Every rank's tiles have the whole render's counts, errors and pixels. t357: 119 tiles a rank, runs of two; t65: 33 and
    32 tiles, one a lane, just below the boundary."""
    import torch
    c = data[cid]
    r = c.rest["median"]
    with hip.HipScene(c.sc) as hs:
        for rank in range(world):
            p = run_adaptive(hs, torch, c, c.thr["median"], rank=rank, world=world)
            assert len(p.counts) == tiles.local_tiles(c.w, c.h, rank, world)
            assert np.array_equal(p.counts, local(c, r.counts, rank, world)), (cid, rank)
            assert np.array_equal(bits(p.errors), bits(local(c, r.errors, rank, world))), (cid, rank)
            assert np.array_equal(bits(p.rad), bits(tiles.pack(r.image, rank, world))), (cid, rank)
            assert np.array_equal(p.rgb, tiles.pack(r.rgb8, rank, world)), (cid, rank)
            assert p.rounds_active == expected_rounds(local(c, r.counts, rank, world)) and p.res["rounds"] == len(p.rounds_active), (cid, rank)
        hs.check()


CHILD = """import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import numpy as np, torch
import rbrt_amd
from oracle import pyoracle
import test_adaptive_many_tiles_gpu as M
out = {{}}
for (cid, scene, w, h), thr in {cases!r}:
    c = M.build_case(pyoracle, cid, scene, w, h)
    with rbrt_amd.HipScene(c.sc) as hs:
        g = M.run_adaptive(hs, torch, c, thr)
        out[cid + "_batches"] = np.array(hs.last_batches())
        hs.check()
    out[cid + "_rad"], out[cid + "_counts"], out[cid + "_rounds"] = g.rad, g.counts, np.array(g.rounds_active)
np.savez({out!r}, **out)
"""

ENV_ROWS = [("tile_pass_off", {"RBRT_PRIMARY_CULL": "0"}),       # no culling words: every active tile on the work list
            ("small_workspace", {"RBRT_HIP_WORKSPACE_MB": "1"})]  # 357 tiles: three samples a batch, a round of four is 3 + 1


@pytest.mark.parametrize("rid,env", ENV_ROWS, ids=[r[0] for r in ENV_ROWS])
def test_mixed_rounds_under_other_schedules(data, tmp_path, rid, env):
    """Each row in a fresh child process (the knobs are read when the library first needs them), at the parent's median
    thresholds: the child's counts and radiance are the parent's restatement's."""
    chosen = [c for c in CASES if c[0] in ("t153_ragged", "t357")]
    cases = [(c, float(repr(data[c[0]].thr["median"]))) for c in chosen]
    assert all(thr == data[c[0]].thr["median"] for c, thr in cases)  # (repr of the float: nothing is lost on the way)
    script, out = tmp_path / "child.py", tmp_path / "child.npz"
    script.write_text(CHILD.format(root=str(ROOT), tests=str(ROOT / "tests"), cases=cases, out=str(out)))
    r = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300, env=dict(os.environ, RBRT_HIP_LAB="1", **env))
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    for (cid, scene, w, h), thr in cases:
        rest = data[cid].rest["median"]
        assert np.array_equal(z[cid + "_counts"], A.per_rank(rest.counts)), (rid, cid)
        assert np.array_equal(bits(z[cid + "_rad"]), bits(rest.image)), (rid, cid)
        assert z[cid + "_rounds"].tolist() == rest.round_active, (rid, cid)
    if rid == "small_workspace":
        assert z["t357_batches"][1] >= 2 and z["t357_batches"][0] < MIN, z["t357_batches"]  # a round split into batches


@pytest.mark.parametrize("cid", ["t153_ragged", "t357"])
def test_a_handle_denoises_a_mixed_render(hip, data, cid):
    """The half images are the restatement's -- a stopped tile's sums were not written again --, the image is the restated
    filter's at the defaults and at other parameters."""
    import torch
    c = data[cid]
    r, den, other = c.rest["median"], c.den["median"], c.den_other["median"]
    with hip.HipScene(c.sc) as hs:
        g = run_adaptive(hs, torch, c, c.thr["median"])
        assert np.array_equal(g.counts, local(c, r.counts)) and np.array_equal(bits(g.rad), bits(r.image))
        d1 = run_denoise(hs, torch, c)
        assert np.array_equal(bits(d1.a), bits(den.a)) and np.array_equal(bits(d1.b), bits(den.b)), cid
        assert np.array_equal(bits(d1.rad), bits(den.image)), (cid, int((bits(d1.rad) != bits(den.image)).sum()))
        assert np.array_equal(d1.rgb, den.rgb8)
        d2 = run_denoise(hs, torch, c, **OTHER_PARAMS)
        assert np.array_equal(bits(d2.a), bits(den.a)) and np.array_equal(bits(d2.b), bits(den.b)), cid
        assert np.array_equal(bits(d2.rad), bits(other.image)) and np.array_equal(d2.rgb, other.rgb8), cid
        hs.check()


# ---- 2. the state grows and shrinks -------------------------------------------------------------------------------------------
#        case             rank world
STEPS = [("spheres_40x24", 0, 1),  # 15 tiles
         ("t153_ragged", 0, 1),    # every buffer grows
         ("spheres_37x21", 0, 1),  # a shrink: the one piece was carved for 153 tiles, the second list sits at 15
         ("t357", 1, 3),           # 119 local tiles of 357: below 153, only the culling words grow
         ("t357", 0, 1),           # everything grows again
         ("t65", 0, 1)]


def test_the_adaptive_state_grows_and_shrinks_on_one_handle(hip, data):
    """One handle, six calls of different sizes and cameras: every call's counts, errors and pixels are a fresh handle's (the
    restatement's), the denoised image of every whole-image call too (the half buffers grow with W x H), and a plain render
    before and after each step is the same."""
    import torch

    def plain(hs, c):
        t = torch.full((c.h, c.w, 3), float("nan"), dtype=torch.float32, device="cuda")
        hs.render_device(c.cam, c.opts_of(N), t.data_ptr(), lens=c.lens)
        torch.cuda.synchronize()
        return t.cpu().numpy()

    assert all(data[cid].scene == "spheres" for cid, _, _ in STEPS)
    with hip.HipScene(data["t65"].sc) as hs:
        for step, (cid, rank, world) in enumerate(STEPS):
            c = data[cid]
            before = plain(hs, c)
            assert np.array_equal(bits(before), bits(c.rest["zero"].image)), (step, cid)
            for kind in ("median", "zero"):
                r = c.rest[kind]
                what = (step, cid, rank, world, kind)
                g = run_adaptive(hs, torch, c, c.thr[kind], rank=rank, world=world)
                assert np.array_equal(g.counts, local(c, r.counts, rank, world)), what
                assert np.array_equal(bits(g.errors), bits(local(c, r.errors, rank, world))), what
                assert g.rounds_active == expected_rounds(local(c, r.counts, rank, world)), what
                if world == 1:
                    assert np.array_equal(bits(g.rad), bits(r.image)) and np.array_equal(g.rgb, r.rgb8), what
                    d = run_denoise(hs, torch, c)
                    assert np.array_equal(bits(d.a), bits(c.den[kind].a)) and np.array_equal(bits(d.b), bits(c.den[kind].b)), what
                    assert np.array_equal(bits(d.rad), bits(c.den[kind].image)) and np.array_equal(d.rgb, c.den[kind].rgb8), what
                else:
                    assert np.array_equal(bits(g.rad), bits(tiles.pack(r.image, rank, world))), what
                    assert np.array_equal(g.rgb, tiles.pack(r.rgb8, rank, world)), what
            assert np.array_equal(bits(plain(hs, c)), bits(before)), (step, cid)
        hs.check()


def test_the_state_grows_with_nothing_allocated_in_between(hip, data):
    """Adaptive calls and nothing else on a fresh handle -- no plain render, no denoiser, so no other device memory is
    asked for between one size and the next: 15 tiles, 153, 357, and 65 again. Every call's results are a fresh handle's."""
    import torch
    with hip.HipScene(data["t65"].sc) as hs:
        for cid in ("spheres_40x24", "t153_ragged", "t357", "t65"):
            c = data[cid]
            for kind in ("median", "zero"):
                r = c.rest[kind]
                g = run_adaptive(hs, torch, c, c.thr[kind])
                assert np.array_equal(g.counts, local(c, r.counts)), (cid, kind)
                assert np.array_equal(bits(g.errors), bits(local(c, r.errors))), (cid, kind)
                assert g.rounds_active == r.round_active, (cid, kind)
                assert np.array_equal(bits(g.rad), bits(r.image)) and np.array_equal(g.rgb, r.rgb8), (cid, kind)
        hs.check()
