"""Conditions on the inputs of test_short_paths_scenes_gpu.py that need no GPU: that the scenes built to reach a line of the
short-path stage (short_paths.inl) do reach it, by the host-side walk of short_cases.py over np_reference. A scene that
stopped meeting its condition would leave the GPU test green and blind."""
from __future__ import annotations

import numpy as np
import pytest

import scenes
import short_cases as S
from rbrt_amd import abi


def whole(cam):
    """The culling table of an image none of whose tiles is background-only (the GPU tests assert that of the device's)."""
    return np.zeros(((cam.img_height_pix + 7) // 8, (cam.img_width_pix + 7) // 8), np.uint32)


@pytest.mark.parametrize("name", list(S.ELEMENT_SCENES))
def test_rays_reach_elements_beyond_the_culling_word(oracle, name):
    """Camera rays AND scattered second rays whose closest hit is at position 24 or above, where the sphere skip's guard
    `e < 24u` is all that keeps the mesh bits out of it; all four materials; tiles the rule keeps and tiles it gives up."""
    sc = S.ELEMENT_SCENES[name]()
    n_elem = len(sc.spheres) + len(sc.triangles)
    assert n_elem == {"grid24": 24, "grid25": 25, "grid32": 32, "mixed30": 30}[name]
    assert {m.kind for _, _, m in sc.spheres} == {S.L, S.M, S.D, S.EM}
    walked = S.element_walk(oracle, name)
    first = np.concatenate([v[0].ravel() for v in walked.values()])
    second = np.concatenate([v[1].ravel() for v in walked.values()])
    assert first.max() < n_elem and second.max() < n_elem
    if n_elem > 24:
        assert (first >= 24).any(), f"{name}: no camera ray's closest hit is at position 24 or above"
        assert (second >= 24).any(), f"{name}: no second ray's closest hit is at position 24 or above"
    else:
        assert (first == 23).any() and (second == 23).any()  # (the last position that has a bit)
    gave_up = [S.tile_masks(v[2])[1] for v in walked.values()]
    assert any(gave_up) or name == "grid24"
    assert not all(gave_up)


def test_the_mixed_order_disagrees_with_the_sphere_indices_around_24(oracle):
    S.check_mixed_order()
    sc = S.mixed_scene()
    walked = S.element_walk(oracle, "mixed30")
    first = np.concatenate([v[0].ravel() for v in walked.values()])
    order = S.MIXED_ORDER
    for what, positions in (("a sphere with index >= 24 at a position < 24", [p for p, e in enumerate(order) if not e >> 31 and e >= 24 and p < 24]),
                            ("a sphere with index < 24 at a position >= 24", [p for p, e in enumerate(order) if not e >> 31 and e < 24 and p >= 24]),
                            ("a triangle at a position < 24", [p for p, e in enumerate(order) if e >> 31 and p < 24])):
        assert np.isin(first, positions).any(), f"no camera ray's closest hit is {what}"
    assert len(sc.triangles) == 4


@pytest.mark.parametrize("n_meshes", [2, 7])
def test_second_rays_reach_the_first_and_the_last_mesh(oracle, n_meshes):
    """From the tiles of NEIGHBOUR_TILES (the stage's: the GPU test asserts it from the device's table) second rays' closest
    hits are mesh 0 and the last mesh: next_gated_mesh has to walk from mesh 0 to the last for the stage to decline them."""
    sc, cam, opts = S.mesh_scene(oracle, n_meshes), S.mesh_camera(oracle), abi.default_opts(**S.MESH_OPTS)
    tiles = S.NEIGHBOUR_TILES[n_meshes]
    assert set(tiles) == {0, n_meshes - 1}
    walked = S.walk(cam, sc, opts, list(tiles.values()))
    for m, tile in tiles.items():
        first, second, _ = walked[tile]
        assert (first < len(sc.spheres)).all(), f"a camera ray of tile {tile} hits a mesh"
        assert (second == len(sc.spheres) + m).any(), f"no second ray from tile {tile} has mesh {m} as its closest hit"


@pytest.mark.parametrize("scene", list(S.COVERED))
def test_the_rule_gives_tiles_up_under_cover(oracle, scene):
    """The 16 x 16 image of the long-batch test: the probe (the launch's first two samples, the same for 3 samples and for 70)
    gives at least one tile up. Under the overhang a given-up tile's probe finished some samples and its third sample would
    have (the zero mask is the rule's doing, not the scene's), and another tile is kept."""
    sc, cam = S.COVERED[scene](), scenes.camera(oracle, 16, 16, **S.CEILING_LOOK)
    walked = S.walk(cam, sc, abi.default_opts(spp=3, seed=5), S.work_tiles(whole(cam)))
    rows = [(S.tile_masks(fin)[1], int(fin[:2].sum()), int(fin[2].sum())) for _, _, fin in walked.values()]
    assert any(g for g, _, _ in rows), rows
    if scene == "overhang":
        assert any(g and probe > 0 and third > 0 for g, probe, third in rows), rows
        assert any(not g for g, _, _ in rows), rows


def test_the_5x3_image_is_kept_for_its_ragged_slots_only(oracle):
    """15 real pixels in a tile of 64 slots, under the ceiling: fewer than three quarters of the real pixels' probe samples
    finish, and the tile is kept all the same because the 49 slots beyond the edges count as finished."""
    sc, cam = S.small_case(oracle, "ceiling", (5, 3))
    first, _, fin = S.walk(cam, sc, abi.default_opts(**S.SMALL_OPTS), [(0, 0)])[(0, 0)]
    real = first[:S.PROBE] != S.RAGGED
    assert real.sum() == S.PROBE * 15
    real_finished = int((fin[:S.PROBE] & real).sum())
    assert real_finished * S.KEEP_DEN < real.sum() * S.KEEP_NUM                        # on its real pixels the tile would be given up
    assert real_finished * S.KEEP_DEN < S.PROBE * 64 * S.KEEP_NUM                       # ... also against the rule's fixed 128
    assert not S.tile_masks(fin)[1]                                                    # and it is kept
    assert (real_finished + int((~real).sum())) * S.KEEP_DEN >= S.PROBE * 64 * S.KEEP_NUM


def test_the_fuzz_cases_are_what_the_issue_asks_for(oracle):
    cases = [S.fuzz_case(oracle, k) for k in range(S.N_FUZZ)]
    assert len(cases) == 24
    assert all(9 <= c.w <= 48 and 9 <= c.h <= 48 and 1 <= c.opts.spp <= 4 and c.opts.max_depth == 12 for c in cases)
    assert [c.lens is not None for c in cases] == [k % 3 == 2 for k in range(24)]
    assert sum(c.on_sphere for c in cases) >= 3
    for c in cases:  # `mode` is fuzz_camera's own: in modes 1 to 3 the camera is within a thousandth of a radius of a sphere, or inside
        if c.on_sphere:
            pos = np.array(list(c.cam.position), np.float64)
            assert any(np.linalg.norm(pos - np.array(ctr, np.float64)) <= r * 1.0011 for ctr, r, _ in c.sc.spheres), c.mode


def test_the_camera_far_from_the_mesh_sees_ground_whose_horizon_hides_it(oracle):
    """The first camera of the foreign-tile case: every camera ray hits the ground, and the mesh's box lies below the tangent
    plane of every ground point in view by more than 100 units -- a ray scattered off the ground goes up from that plane, so
    none can pass the box, and with max_depth 1 every sample is the stage's to finish."""
    import test_primary_cull as PC
    sc, cam = S.two_camera_scene(oracle), S.camera_away(oracle)
    rng = np.random.default_rng(3)
    centre, radius = np.array(S.GROUND[0], np.float64), S.GROUND[1]
    lo, hi = sc.meshes[0].bbox_lo.astype(np.float64), sc.meshes[0].bbox_hi.astype(np.float64)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    for u0, u1 in PC.jitters(rng, 16, 16):
        rays = PC.camera_rays(cam, u0, u1)
        t, obj, _, _ = oracle.trace_rays(sc, rays)
        assert (obj == 0).all()
        points = rays[:, :3].astype(np.float64) + t[:, None].astype(np.float64) * rays[:, 3:].astype(np.float64)
        normals = (points - centre) / radius
        height = ((corners[None, :, :] - points[:, None, :]) * normals[:, None, :]).sum(-1)  # of the box's corners over each tangent plane
        assert height.max() < -100.0, height.max()
