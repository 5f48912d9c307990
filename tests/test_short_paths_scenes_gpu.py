"""The short-path stage (short_paths.inl) on the inputs test_short_paths_gpu.py never gave it: more elements than the culling
word has element bits, element orders in which position and sphere index disagree around 24, two, seven and eight meshes, a
lens together with a mesh, the cameras of the culling fuzz, batches longer than one 64-bit mask over tiles the stage gives
up or does not own, images smaller than a tile, and the calls that must not get the stage after one that did.

Every render case compares, as the older file does, the float32 radiance with the stage in front of every launch (mode 2)
bit for bit with the CPU oracle AND with the same handle's render without it (mode 0), sample buffers poisoned in both, and
ends with the handle's check(). The scenes and the host-side walk of the stage's rule are in short_cases.py; the conditions on
the inputs that need no GPU are asserted in test_short_paths_conditions.py, those that need the device's culling table here."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import pytest

import np_adaptive as A
import np_lens
import scenes
import short_cases as S
import test_adaptive_gpu as TA
import test_primary_cull as PC
from rbrt_amd import abi
from test_short_paths_gpu import assert_masks, assert_same, on_and_off, poisoned, popcount, render, side_mesh_scene  # noqa: F401

pytestmark = pytest.mark.gpu

ONES = (1 << 64) - 1


def both_references(on, off, exp, what):
    assert_same(on, exp, f"{what} against the oracle")
    assert_same(on, off, f"{what} against the stage off")


def sample0_hits(oracle, cam, sc):
    """[H, W] of the object the camera ray of sample 0 hits with its jitter in the middle of the pixel, by the oracle's hit
    routine (-1: nothing; number of elements + k: mesh k)."""
    H, W = cam.img_height_pix, cam.img_width_pix
    half = np.full((H, W), np.float32(0.5))
    return oracle.trace_rays(sc, PC.camera_rays(cam, half, half))[1].reshape(H, W)


def owned_tiles(cull, n_meshes):
    """Tiles of the stage: on the work list, every mesh bit set."""
    mesh_bits = np.uint32((1 << n_meshes) - 1)
    return ((cull >> 31) == 0) & (((cull >> 24) & mesh_bits) == mesh_bits)


# ---- 1. elements beyond the culling word --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.ELEMENT_SCENES))
def test_more_elements_than_element_bits(hip, oracle, name):
    """24, 25 and 32 spheres of all four materials, and 30 elements in an order in which position and sphere index disagree
    around 24: no mesh, so every tile on the work list is the stage's and the restated rule gives its masks exactly."""
    sc, cam, opts = S.ELEMENT_SCENES[name](), S.element_camera(oracle), abi.default_opts(**S.ELEMENT_OPTS)
    n_elem = len(sc.spheres) + len(sc.triangles)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    own = owned_tiles(cull, 0)
    low = cull & np.uint32((1 << min(n_elem, 24)) - 1)
    assert (own & (low != 0) & (low != (1 << min(n_elem, 24)) - 1)).any(), f"{name}: no tile of the stage has element bits both set and clear"
    assert not (cull & np.uint32(0x7F000000)).any(), cull  # (no mesh: no bit at 24 or above but the background-only one)
    if n_elem > 24:
        assert own.all()  # (a scene the word cannot describe whole has no background-only tiles)
    S.assert_masks(masks, cam, sc, opts, cull, name, walked=S.element_walk(oracle, name))
    assert 0 < popcount(masks).sum() < 64 * len(masks)
    both_references(on, off, oracle.render(cam, sc, opts)[0], name)


def test_more_elements_than_element_bits_beside_a_mesh(hip, oracle):
    """32 spheres and a mesh at the right edge: in a tile of the stage bit 24 is SET (the mesh's box is out of reach) while
    the sphere at position 24 is in reach -- a sphere skip that read the word at position 24 and above would take the mesh's
    bit for the sphere's and lose the hit."""
    sc, cam, opts = S.grid_and_mesh_scene(oracle), S.element_camera(oracle), abi.default_opts(**S.ELEMENT_OPTS)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    own = owned_tiles(cull, 1)
    assert own.any() and not own.all(), cull
    hit = sample0_hits(oracle, cam, sc)
    seen = PC.tiles_of((hit >= 24) & (hit < 32), cam.img_width_pix, cam.img_height_pix)
    assert (own & seen).any(), "no tile of the stage sees a sphere at position 24 or above"
    n = popcount(masks)
    assert 0 < np.count_nonzero(n) <= opts.spp * np.count_nonzero(own) and np.count_nonzero(n == 0) >= opts.spp * np.count_nonzero(~own)
    both_references(on, off, oracle.render(cam, sc, opts)[0], "32 spheres and a mesh")


# ---- 2. two, seven and eight meshes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_meshes", [2, 7])
def test_several_meshes(hip, oracle, n_meshes):
    """Every mesh bit decides somewhere: for each mesh a tile whose only clear mesh bit is that mesh's and that sees the mesh."""
    sc, cam, opts = S.mesh_scene(oracle, n_meshes), S.mesh_camera(oracle), abi.default_opts(**S.MESH_OPTS)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    every = (1 << n_meshes) - 1
    mesh_word, sky = (cull >> 24) & np.uint32(every), (cull >> 31) != 0
    own = owned_tiles(cull, n_meshes)
    assert own.any(), "no tile has all mesh bits set and is not background-only"
    assert ((mesh_word != 0) & (mesh_word != every)).any(), "no tile has some mesh bits set but not all"
    hit = sample0_hits(oracle, cam, sc)
    for m in range(n_meshes):
        only = ~sky & (mesh_word == (every & ~(1 << m)))
        sees = PC.tiles_of(hit == len(sc.spheres) + m, cam.img_width_pix, cam.img_height_pix)
        assert (only & sees).any(), f"mesh {m}: no tile with bit {24 + m} as its only clear mesh bit has a camera ray that hits it"
    for m, tile in S.NEIGHBOUR_TILES[n_meshes].items():
        assert own[tile], f"tile {tile} beside mesh {m} is not the stage's"  # (test_short_paths_conditions: its second rays reach the mesh)
    n = popcount(masks)
    assert 0 < np.count_nonzero(n) <= opts.spp * np.count_nonzero(own)
    assert np.count_nonzero(n == 0) >= opts.spp * np.count_nonzero(~own & ~sky)
    both_references(on, off, oracle.render(cam, sc, opts)[0], f"{n_meshes} meshes")


def test_eight_meshes_have_no_stage(hip, oracle):
    """The culling word has seven mesh bits: a scene of eight meshes gets no stage even when asked for."""
    cam, opts = S.mesh_camera(oracle), abi.default_opts(**S.MESH_OPTS)
    sc = S.mesh_scene(oracle, 8)
    with hip.HipScene(sc) as hs:
        hs.set_short_paths(2)
        on = render(hs, cam, opts)
        assert len(hs.short_masks()) == 0
        hs.set_short_paths(0)
        off = render(hs, cam, opts)
        hs.check()
    both_references(on, off, oracle.render(cam, sc, opts)[0], "8 meshes")
    with hip.HipScene(S.mesh_scene(oracle, 7)) as hs:
        hs.set_short_paths(2)
        render(hs, cam, opts)
        assert popcount(hs.short_masks()).sum() > 0
        hs.check()


# ---- 3. a lens and a mesh -----------------------------------------------------------------------------------------------------
def test_a_lens_widens_the_mesh_bits(hip, oracle):
    """A lens 0.6 units across: the mesh's box comes into reach of tiles whose pinhole rays miss it, and those tiles
    are no longer the stage's."""
    sc, cam = side_mesh_scene(oracle), scenes.camera(oracle, 96, 64)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], S.WIDE_APERTURE_MM, 10.0)
    opts = abi.default_opts(spp=3, seed=29)
    with hip.HipScene(sc) as hs:
        pinhole, table = hs.primary_cull(cam), hs.primary_cull(cam, lens=lens)
        on, masks, off = on_and_off(hs, cam, opts, lens)
    kept, before = np.count_nonzero((table >> 24) & 1), np.count_nonzero((pinhole >> 24) & 1)
    assert 0 < kept < before, (kept, before)
    own = owned_tiles(table, 1)
    n = popcount(masks)
    assert 0 < np.count_nonzero(n) <= opts.spp * np.count_nonzero(own)
    assert np.count_nonzero(n == 0) >= opts.spp * np.count_nonzero(~own & ((table >> 31) == 0)) > 0
    assert (n < 64).any() and n.sum() > 0  # (both sides: samples finished, samples left)
    both_references(on, off, oracle.render(cam, sc, opts, lens=lens)[0], "a lens and a mesh")


# ---- 4. the cull fuzz through the stage ---------------------------------------------------------------------------------------
def fuzz_results(hip, oracle):
    out = []
    for k in range(S.N_FUZZ):
        c = S.fuzz_case(oracle, k)
        exp = oracle.render(c.cam, c.sc, c.opts, lens=c.lens)[0]
        with hip.HipScene(c.sc) as hs:
            on, masks, off = on_and_off(hs, c.cam, c.opts, c.lens)
        both_references(on, off, exp, f"fuzz case {k} (seed {S.FUZZ_BASE + k}, {c.w}x{c.h}x{c.opts.spp}, camera mode {c.mode})")
        # a set bit in a slot that lies inside the image in EVERY tile is a real sample the stage finished
        inside = sum(1 << p for p in range(64) if p // 8 < (c.h % 8 or 8) and p % 8 < (c.w % 8 or 8))
        out.append(SimpleNamespace(k=k, mode=c.mode, on_sphere=c.on_sphere, n_meshes=len(c.sc.meshes), chunks=len(masks),
                                   finished=int(sum(1 for m in masks if int(m) & inside))))
    return out


def test_the_cull_fuzz_through_the_stage(hip, oracle):
    """The scenes and cameras of test_primary_cull's fuzz (seeds FUZZ_BASE + k of this file's own), 9 to 48 pixels each way, 1
    to 4 samples, max_depth 12, a lens on every third case, the stage in front of every launch: against the oracle and
    against the stage off. No case is skipped; over the set, at least half the cases have a tile of the stage with a finished
    sample, and at least three of those have the camera inside or on a sphere (fuzz_camera's modes 1 to 3).

    Seed base 96000, 24 cases, on an MI355X: 18 cases with a finished sample, 7 of them with the camera inside or on a sphere
    (cases 2, 7, 9, 11, 14, 17, 18); case 21 has no work for the trace kernel and so no stage."""
    res = fuzz_results(hip, oracle)
    assert len(res) == S.N_FUZZ == 24
    finished = [r for r in res if r.finished > 0]
    hard = [r for r in finished if r.on_sphere]
    print(f"fuzz base {S.FUZZ_BASE}: {len(finished)} of {len(res)} cases with a finished sample, {len(hard)} of them with the camera inside or "
          f"on a sphere; {sum(r.chunks == 0 for r in res)} cases without a stage (more than 7 meshes or no work); per case "
          f"{[(r.k, r.mode, r.n_meshes, r.chunks, r.finished) for r in res]}")
    assert 2 * len(finished) >= len(res), [r.k for r in finished]
    assert len(hard) >= 3, [r.k for r in hard]


# ---- 5. masks nobody rewrote --------------------------------------------------------------------------------------------------
LONG = 70  # samples of a batch: more than the 64 the zeroing loops take in one stride


def ceiling_camera(oracle, size):
    return scenes.camera(oracle, *size, **S.CEILING_LOOK)


@pytest.mark.parametrize("scene", list(S.COVERED))
def test_a_given_up_tile_with_a_long_batch(hip, oracle, scene):
    """One lane, one buffer. A first launch (max_depth 1: every sample ends with its second ray) leaves 70 masks of all ones
    per tile; in the second launch over the same camera the stage gives tiles up after two samples and has to zero the other
    68 masks, more than one 64-lane stride of its loop: a stale one would tell the trace kernel that 64 samples are done which
    nobody computed, and the poisoned buffer would show it."""
    sc, cam = S.COVERED[scene](), ceiling_camera(oracle, (16, 16))
    first, opts = abi.default_opts(spp=LONG, seed=5, max_depth=1), abi.default_opts(spp=LONG, seed=5, max_depth=50)
    with hip.HipScene(sc) as hs:
        hs.set_pipeline(1)
        hs.set_short_paths(2)
        cull = hs.primary_cull(cam)
        render(hs, cam, first)
        before = hs.short_masks()
        assert hs.last_batches() == (LONG, 1) and len(before) == LONG * cull.size and (before == np.uint64(ONES)).all()
        on, masks, off = on_and_off(hs, cam, opts)
        assert hs.last_batches() == (LONG, 1)
    assert not (cull >> 31).any()
    assert len(masks) == LONG * cull.size
    assert np.count_nonzero(masks == 0) >= LONG - 2, "no tile was given up"  # (test_short_paths_conditions: the rule gives one up)
    assert_masks(masks, cam, sc, opts, cull, f"{scene}: a given-up tile, 70 samples")
    both_references(on, off, oracle.render(cam, sc, opts)[0], f"{scene}: a given-up tile, 70 samples")


def test_a_foreign_tile_with_a_long_batch(hip, oracle):
    """One handle, the ground and a mesh, two cameras. From the first the mesh is out of view and below the horizon of the
    ground it sees: all 70 masks of every tile end as all ones. From the second the mesh's box is in reach of every tile: none
    is the stage's, and it has to zero all 70 masks of each."""
    sc = S.two_camera_scene(oracle)
    cam_a, cam_b = S.camera_away(oracle), S.camera_at_the_mesh(oracle)
    first, opts = abi.default_opts(spp=LONG, seed=6, max_depth=1), abi.default_opts(spp=LONG, seed=6)
    with hip.HipScene(sc) as hs:
        hs.set_pipeline(1)
        hs.set_short_paths(2)
        cull_a, cull_b = hs.primary_cull(cam_a), hs.primary_cull(cam_b)
        render(hs, cam_a, first)
        before = hs.short_masks()
        assert hs.last_batches() == (LONG, 1) and len(before) == LONG * cull_a.size and (before == np.uint64(ONES)).all()
        on, masks, off = on_and_off(hs, cam_b, opts)
        assert hs.last_batches() == (LONG, 1)
    assert ((cull_a >> 24) == 1).all(), cull_a  # (the stage's: the mesh bit set, not background-only)
    assert not ((cull_b >> 24) & 1).any() and not (cull_b >> 31).any(), cull_b
    assert len(masks) == LONG * cull_b.size == len(before) and not masks.any(), masks
    both_references(on, off, oracle.render(cam_b, sc, opts)[0], "a foreign tile, 70 samples")


@pytest.mark.parametrize("scene", list(S.COVERED))
@pytest.mark.parametrize("spp", [1, 2, 3])
def test_sample_counts_around_the_probe(hip, oracle, spp, scene):
    """Fewer samples than the probe, as many, one more (the first launch at which a tile can be given up). Under the ceiling
    no sample finishes anyway; under the overhang a given-up tile's third mask is zero where the rule alone makes it so."""
    sc, cam, opts = S.COVERED[scene](), ceiling_camera(oracle, (16, 16)), abi.default_opts(spp=spp, seed=5)
    with hip.HipScene(sc) as hs:
        hs.set_pipeline(1)
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    assert len(masks) == spp * cull.size
    assert_masks(masks, cam, sc, opts, cull, f"{scene}, {spp} samples")
    if spp == 3:
        assert np.count_nonzero(masks == 0) >= 1
    both_references(on, off, oracle.render(cam, sc, opts)[0], f"{scene}, {spp} samples")


# ---- 6. smaller than a tile ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["ceiling", "spheres"])
@pytest.mark.parametrize("size", S.SMALL_SIZES, ids=[f"{w}x{h}" for w, h in S.SMALL_SIZES])
def test_images_smaller_than_a_tile(hip, oracle, size, scene):
    """One ragged tile (1x1, 5x3), one whole tile, one whole and one a column wide: the probe counts the slots beyond the
    edge as finished."""
    sc, cam = S.small_case(oracle, scene, size)
    opts = abi.default_opts(**S.SMALL_OPTS)
    with hip.HipScene(sc) as hs:
        cull = hs.primary_cull(cam)
        on, masks, off = on_and_off(hs, cam, opts)
    assert len(masks) == opts.spp * np.count_nonzero((cull >> 31) == 0) > 0
    assert_masks(masks, cam, sc, opts, cull, f"{scene} {size}")
    both_references(on, off, oracle.render(cam, sc, opts)[0], f"{scene} {size}")


# ---- 7. calls that must not have the stage ------------------------------------------------------------------------------------
def test_a_counting_render_after_the_stage(hip, oracle):
    """The stage keeps no counters: a render with FLAG_COLLECT_STATS gets none, whatever masks the lane's buffer holds."""
    sc, cam = side_mesh_scene(oracle), scenes.camera(oracle, 40, 24)
    opts, counting = abi.default_opts(spp=4, seed=31), abi.default_opts(spp=4, seed=31, flags=abi.FLAG_COLLECT_STATS)
    exp, _, rays = oracle.render(cam, sc, opts)
    with hip.HipScene(sc) as hs:
        hs.set_pipeline(1)
        hs.set_short_paths(2)
        assert_same(render(hs, cam, opts), exp, "the render before")
        before = hs.short_masks()
        assert popcount(before).sum() > 0
        got = render(hs, cam, counting)
        st = hs.stats()
        after = hs.short_masks()
        assert_same(render(hs, cam, opts), exp, "the render after")
        hs.check()
    assert_same(got, exp, "the counting render")
    assert st["samples"] == 40 * 24 * 4 and st["rays"] == rays, (st, rays)
    assert np.array_equal(before, after)


@pytest.fixture(scope="module")
def adaptive_case(hip, oracle):
    """test_adaptive_gpu's case spheres_37x21 with its restatement at threshold 0 and at the median of the first round's errors."""
    import torch
    cid, scene, w, h, n, mn, step = TA.CASES[1]
    cam, lens, sc, opts_of = TA.build(oracle, scene, w, h)
    with hip.HipScene(sc) as hs:
        samples = TA.extract_samples(hs, torch, cam, lens, opts_of, n)
        hs.check()
    zero = A.adaptive(samples, 0.0, mn, step)
    median = float(np.float32(np.median(zero.round_errors[0])))
    return SimpleNamespace(cid=cid, w=w, h=h, n=n, mn=mn, step=step, cam=cam, lens=lens, sc=sc, opts_of=opts_of,
                           thr=dict(zero=0.0, median=median), rest=dict(zero=zero, median=A.adaptive(samples, median, mn, step)))


@pytest.mark.parametrize("kind", ["zero", "median"])
def test_an_adaptive_render_after_the_stage(hip, adaptive_case, kind):
    """The rounds of render_adaptive get no stage. On a handle in mode 2 whose last render_device left masks with finished
    samples in the lane's buffer, the call gives what it gives on a fresh handle in mode 0, and what np_adaptive gives."""
    import torch
    c = adaptive_case
    r = c.rest[kind]
    assert len(np.unique(c.rest["median"].counts)) >= 2  # (the median threshold stops some tiles early)
    with hip.HipScene(c.sc) as hs:
        hs.set_pipeline(1)
        hs.set_short_paths(2)
        render(hs, c.cam, c.opts_of(c.n))
        before = hs.short_masks()
        assert popcount(before).sum() > 0
        g = TA.run_adaptive(hs, torch, c, c.thr[kind])
        assert np.array_equal(hs.short_masks(), before)
        hs.check()
    with hip.HipScene(c.sc) as hs:
        hs.set_short_paths(0)
        f = TA.run_adaptive(hs, torch, c, c.thr[kind])
        hs.check()
    assert np.array_equal(g.counts, f.counts) and g.res == f.res and g.rounds_active == f.rounds_active, (g.counts, f.counts, g.res, f.res)
    assert_same(g.rad, f.rad, f"adaptive {kind} against a fresh handle in mode 0")
    assert np.array_equal(g.rgb, f.rgb)
    assert np.array_equal(g.counts, A.per_rank(r.counts)) and g.res["rounds"] == r.rounds and g.res["samples"] == r.samples
    assert_same(g.rad, r.image, f"adaptive {kind} against the restatement")
