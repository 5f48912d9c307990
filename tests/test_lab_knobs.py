"""Lab knobs (include/rbrt_hip_debug.h): every one of them is validated by rbrt_hip_scene_create, and none of them changes
the image.

The scheduling knobs steer branches inside the one product megakernel (refill water marks, leaf rounds, register-resident
shading, striped work hand-out, grids, the light-tile tail); the tuning tools time the kernel under non-default values,
which is only meaningful if the image stays the oracle's. MATRIX below renders three small scenes under every row, through
the paths that select different code: a blocking frame (full grid, list mode 4), a stream of four queued frames (overlap
grid, list mode 0), the counting build, and on some rows several sample batches per frame or tiles of one rank of three.
Where a debug counter or the RBRT_TRACE_LAUNCHES line shows that the knob took effect, the row asserts it.

VALID lists each knob's range; the validation tests check both ends, the values just outside them and malformed strings.
test_every_header_knob_has_rows (CPU) fails when a knob is added to the header without rows here."""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import scenes
import test_emissive as E
from rbrt_amd import abi, tiles
from test_gpu_parity import assert_same_image

ROOT = Path(__file__).resolve().parent.parent
STATS, CONST_BG = abi.FLAG_COLLECT_STATS, abi.FLAG_CONSTANT_BACKGROUND

# ---- the knobs' ranges --------------------------------------------------------------------------------------------------
# kind: "int" (lo..hi), "pow2" (0 or a power of two in lo..hi), "float" ([lo, hi]), "float_open" ((lo, hi]), "enum" (lo|hi)
VALID = {
    "RBRT_LDS_STACK": ("int", 1, 64), "RBRT_Y_LOW": ("int", 1, 64), "RBRT_Y_HIGH": ("int", 1, 64),
    "RBRT_Y_HIGH_PARKED": ("int", 1, 256), "RBRT_LEAF_ROUND": ("int", 1, 64), "RBRT_LEAF_LEAVES": ("int", 1, 128),
    "RBRT_SHARE_IDLE": ("int", 0, 64), "RBRT_WORK_STRIPES": ("pow2", 0, 65536), "RBRT_WORK_STRIPES_OVERLAP": ("pow2", 0, 65536),
    "RBRT_SHADE_ROUNDS": ("int", 1, 64), "RBRT_SHADE_CONT_MIN": ("int", 1, 64), "RBRT_WAVES_PER_CU": ("int", 1, 32),
    "RBRT_PIPELINE": ("int", 0, 8), "RBRT_BVH_CT": ("float_open", 0.0, 1000.0), "RBRT_PLOC_RADIUS": ("int", 1, 256),
    "RBRT_BVH_DEVICE_MIN": ("int", 0, 1 << 30), "RBRT_BVH_DEVICE_ALGO": ("enum", "ploc", "lbvh"),
    "RBRT_POISON_SAMPLES": ("int", 0, 1), "RBRT_PRIMARY_CULL": ("int", 0, 1), "RBRT_TILE_TAIL_DIV": ("int", 1, 1024),
    "RBRT_OVERLAP_WAVES_PER_CU": ("int", 0, 16), "RBRT_TRACE_LAUNCHES": ("int", 0, 1), "RBRT_HELPERS": ("int", 0, 2),
    "RBRT_HELPER_MIN_ITEMS": ("int", 1, 1 << 24), "RBRT_HELPER_ROUNDS": ("int", 1, 16), "RBRT_HELPER_MIN_LAUNCH_MI": ("int", 0, 4096),
    "RBRT_HELPER_MIN_FREE": ("int", 1, 16), "RBRT_BVH_SPATIAL": ("float", 0.0, 0.6), "RBRT_TRACE_CREATE": ("int", 0, 1),
}
BVH_KNOBS = ("RBRT_BVH_CT", "RBRT_BVH_SPATIAL", "RBRT_PLOC_RADIUS", "RBRT_BVH_DEVICE_ALGO")  # also parsed by the debug builders


def accepted_values(name):
    kind, lo, hi = VALID[name]
    if kind == "float_open":
        return ["1e-06", repr(hi)]
    if kind == "float":
        return [repr(lo), repr(hi)]
    return [str(lo), str(hi)]


def refused_values(name):
    kind, lo, hi = VALID[name]
    bad = ["12x", "", "-1"]
    if kind == "enum":
        return bad + ["PLOC", "lbvh ", "radix"]
    if kind in ("float", "float_open"):
        return bad + [repr(lo - 1), repr(hi + 1), "nan", "inf", "-inf", repr(hi * 1.01)] + (["0", "0.0"] if kind == "float_open" else [])
    bad += [str(lo - 1), str(hi + 1), "1.5", "0x10"]
    if kind == "pow2":
        bad += ["3", "12", "65535"]
    return bad


# ---- the matrix ---------------------------------------------------------------------------------------------------------
# Each row: (id, env, what shows the knob took effect). Scheduling counters depend on timing: a row compares them only where
# the margin is large, and a knob with no counter of its own says so. Flags: "batches" = RBRT_HIP_WORKSPACE_MB=1 and a
# frame that takes several sample batches; "rank" = tiles of rank 1 of 3; "own_pipeline" = the stream is issued at the
# depth the knob sets (no set_pipeline(3)).
MATRIX = [
    ("default", {}, "the baseline of the counter comparisons"),
    ("y_low_1", {"RBRT_Y_LOW": "1"}, "no counter of its own (refill_rounds moves with timing)"),
    ("y_low_64", {"RBRT_Y_LOW": "64"}, "no counter of its own"),
    ("y_high_1", {"RBRT_Y_HIGH": "1"}, "no counter of its own (below RBRT_Y_LOW: the kernel uses Y_LOW)"),
    ("y_high_64", {"RBRT_Y_HIGH": "64", "RBRT_Y_HIGH_PARKED": "1"}, "no counter of its own"),
    ("y_parked_1", {"RBRT_Y_HIGH_PARKED": "1", "RBRT_Y_LOW": "1", "RBRT_Y_HIGH": "64"}, "no counter of its own"),
    ("y_parked_64", {"RBRT_Y_HIGH_PARKED": "64", "RBRT_Y_HIGH": "37"}, "no counter of its own"),
    ("y_parked_256", {"RBRT_Y_HIGH_PARKED": "256", "RBRT_Y_LOW": "64"}, "no counter of its own"),
    ("leaf_round_1", {"RBRT_LEAF_ROUND": "1"}, "no counter asserted"),
    ("leaf_round_64", {"RBRT_LEAF_ROUND": "64", "RBRT_LEAF_LEAVES": "37"}, "no counter asserted"),
    ("leaf_leaves_1", {"RBRT_LEAF_LEAVES": "1"}, "leaf_lanes / leaf_rounds well below the other end's (26 against 68)"),
    ("leaf_leaves_128", {"RBRT_LEAF_LEAVES": "128", "RBRT_LEAF_ROUND": "64"}, "no counter asserted"),
    ("shade_2_cont_1", {"RBRT_SHADE_ROUNDS": "2", "RBRT_SHADE_CONT_MIN": "1"}, "no counter asserted"),
    ("shade_2_cont_64", {"RBRT_SHADE_ROUNDS": "2", "RBRT_SHADE_CONT_MIN": "64"}, "no counter asserted"),
    ("shade_64_cont_64", {"RBRT_SHADE_ROUNDS": "64", "RBRT_SHADE_CONT_MIN": "64"}, "no counter asserted"),
    ("shade_64_cont_1", {"RBRT_SHADE_ROUNDS": "64", "RBRT_SHADE_CONT_MIN": "1", "RBRT_WAVES_PER_CU": "1"},
     "shade_extra_rounds well above the same grid's at the default shading (5900 against 3400)"),
    # one wave per CU: the waves of the 200x150x5 counting frame take ~9 chunks each (at the full grid, one), so the
    # branches taken while work items are left run under these rows
    ("y_low_1_1wave", {"RBRT_Y_LOW": "1", "RBRT_WAVES_PER_CU": "1"}, "no counter of its own"),
    ("y_parked_256_1wave", {"RBRT_Y_HIGH_PARKED": "256", "RBRT_Y_LOW": "64", "RBRT_WAVES_PER_CU": "1"}, "no counter of its own"),
    ("y_high_64_1wave", {"RBRT_Y_HIGH": "64", "RBRT_Y_HIGH_PARKED": "1", "RBRT_Y_LOW": "5", "RBRT_WAVES_PER_CU": "1"},
     "no counter of its own"),
    ("leaf_1_1wave", {"RBRT_LEAF_ROUND": "1", "RBRT_LEAF_LEAVES": "1", "RBRT_WAVES_PER_CU": "1"}, "no counter asserted"),
    ("shade_2_cont_64_1wave", {"RBRT_SHADE_ROUNDS": "2", "RBRT_SHADE_CONT_MIN": "64", "RBRT_WAVES_PER_CU": "1"}, "no counter asserted"),
    ("stripes_1_1wave", {"RBRT_WORK_STRIPES": "1", "RBRT_WORK_STRIPES_OVERLAP": "1", "RBRT_WAVES_PER_CU": "1"}, "the image only"),
    ("stripes_65536_1wave", {"RBRT_WORK_STRIPES": "65536", "RBRT_WORK_STRIPES_OVERLAP": "65536", "RBRT_WAVES_PER_CU": "1"},
     "the image only"),
    ("stripes_0", {"RBRT_WORK_STRIPES": "0", "RBRT_WORK_STRIPES_OVERLAP": "0"}, "no counter: the image only"),
    ("stripes_1", {"RBRT_WORK_STRIPES": "1", "RBRT_WORK_STRIPES_OVERLAP": "1"}, "no counter: the image only"),
    ("stripes_2", {"RBRT_WORK_STRIPES": "2", "RBRT_WORK_STRIPES_OVERLAP": "2"}, "no counter: the image only"),
    ("stripes_65536", {"RBRT_WORK_STRIPES": "65536", "RBRT_WORK_STRIPES_OVERLAP": "65536"}, "no counter: the image only"),
    ("stripes_mixed", {"RBRT_WORK_STRIPES": "2", "RBRT_WORK_STRIPES_OVERLAP": "65536", "RBRT_HIP_WORKSPACE_MB": "1"},
     "several batches per frame"),
    ("waves_1", {"RBRT_WAVES_PER_CU": "1"}, "every trace launch has 1 wave per CU (trace line, scene info)"),
    ("waves_3", {"RBRT_WAVES_PER_CU": "3"}, "every trace launch has 3 waves per CU"),
    ("waves_32", {"RBRT_WAVES_PER_CU": "32"}, "every trace launch has 32 waves per CU (more than can be resident)"),
    ("overlap_waves_0", {"RBRT_OVERLAP_WAVES_PER_CU": "0"}, "the default: no grid asserted"),
    ("overlap_waves_1", {"RBRT_OVERLAP_WAVES_PER_CU": "1"}, "the stream's overlapped launches have 1 wave per CU"),
    ("overlap_waves_16", {"RBRT_OVERLAP_WAVES_PER_CU": "16"}, "the stream's overlapped launches have 16 waves per CU"),
    ("pipeline_0", {"RBRT_PIPELINE": "0"}, "no counter (own_pipeline)"),
    ("pipeline_1", {"RBRT_PIPELINE": "1"}, "no stream launch overlaps another (own_pipeline)"),
    ("pipeline_8", {"RBRT_PIPELINE": "8"}, "no counter (own_pipeline)"),
    ("tail_1_cull_0", {"RBRT_TILE_TAIL_DIV": "1", "RBRT_PRIMARY_CULL": "0"}, "no tile pass"),
    ("tail_1_cull_1", {"RBRT_TILE_TAIL_DIV": "1", "RBRT_PRIMARY_CULL": "1"}, "list mode 4 for the blocking frame"),
    ("tail_1024_cull_0", {"RBRT_TILE_TAIL_DIV": "1024", "RBRT_PRIMARY_CULL": "0"}, "no tile pass"),
    ("tail_1024_cull_1", {"RBRT_TILE_TAIL_DIV": "1024", "RBRT_PRIMARY_CULL": "1"}, "list mode 4 for the blocking frame"),
    ("share_idle_64", {"RBRT_SHARE_IDLE": "64"}, "share_rounds == 0 (a wave with 64 idle lanes has nothing to share)"),
    ("lds_stack_1", {"RBRT_LDS_STACK": "1"}, "stack_pushes_beyond_lds > 1000 (11 at the default)"),
    ("lds_stack_64", {"RBRT_LDS_STACK": "64"}, "stack_pushes_beyond_lds == 0"),
    ("poison_0", {"RBRT_POISON_SAMPLES": "0"}, "no counter (the other rows poison)"),
    ("helpers_lo", {"RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": "1", "RBRT_HELPER_ROUNDS": "1",
                    "RBRT_HELPER_MIN_LAUNCH_MI": "0", "RBRT_HELPER_MIN_FREE": "1"}, "no counter asserted"),
    ("helpers_hi", {"RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": str(1 << 24), "RBRT_HELPER_ROUNDS": "16",
                    "RBRT_HELPER_MIN_LAUNCH_MI": "4096", "RBRT_HELPER_MIN_FREE": "16"}, "no counter asserted"),
    ("helpers_mid", {"RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": "777", "RBRT_HELPER_ROUNDS": "3",
                     "RBRT_HELPER_MIN_LAUNCH_MI": "5", "RBRT_HELPER_MIN_FREE": "7", "RBRT_HIP_WORKSPACE_MB": "1"},
     "several batches per frame"),
    ("helpers_watcher", {"RBRT_HELPERS": "1", "RBRT_HELPER_MIN_LAUNCH_MI": "0", "RBRT_HELPER_MIN_FREE": "16",
                         "RBRT_HELPER_MIN_ITEMS": "1"}, "no counter asserted"),
    ("extremes_lo", {"RBRT_Y_LOW": "1", "RBRT_Y_HIGH": "1", "RBRT_Y_HIGH_PARKED": "1", "RBRT_LEAF_ROUND": "1", "RBRT_LEAF_LEAVES": "1",
                     "RBRT_SHADE_ROUNDS": "64", "RBRT_SHADE_CONT_MIN": "1", "RBRT_WORK_STRIPES": "1", "RBRT_WORK_STRIPES_OVERLAP": "1",
                     "RBRT_WAVES_PER_CU": "1", "RBRT_PIPELINE": "8", "RBRT_TILE_TAIL_DIV": "1", "RBRT_LDS_STACK": "1",
                     "RBRT_SHARE_IDLE": "1", "RBRT_HELPERS": "2", "RBRT_HELPER_MIN_ITEMS": "1", "RBRT_HELPER_ROUNDS": "16",
                     "RBRT_TRACE_CREATE": "1", "RBRT_HIP_WORKSPACE_MB": "1"}, "rank 1 of 3; several batches"),
    ("extremes_hi", {"RBRT_Y_LOW": "64", "RBRT_Y_HIGH": "64", "RBRT_Y_HIGH_PARKED": "256", "RBRT_LEAF_ROUND": "64",
                     "RBRT_LEAF_LEAVES": "128", "RBRT_SHADE_ROUNDS": "64", "RBRT_SHADE_CONT_MIN": "64",
                     "RBRT_WORK_STRIPES": "65536", "RBRT_WORK_STRIPES_OVERLAP": "65536", "RBRT_WAVES_PER_CU": "32",
                     "RBRT_OVERLAP_WAVES_PER_CU": "16", "RBRT_PIPELINE": "1", "RBRT_TILE_TAIL_DIV": "1024", "RBRT_LDS_STACK": "64",
                     "RBRT_SHARE_IDLE": "64", "RBRT_PRIMARY_CULL": "0"}, "rank 1 of 3"),
    ("extremes_mixed", {"RBRT_Y_LOW": "64", "RBRT_Y_HIGH": "1", "RBRT_Y_HIGH_PARKED": "256", "RBRT_LEAF_ROUND": "1",
                        "RBRT_LEAF_LEAVES": "128", "RBRT_SHADE_ROUNDS": "2", "RBRT_SHADE_CONT_MIN": "1",
                        "RBRT_WORK_STRIPES": "0", "RBRT_WORK_STRIPES_OVERLAP": "2", "RBRT_OVERLAP_WAVES_PER_CU": "1",
                        "RBRT_TILE_TAIL_DIV": "3", "RBRT_LDS_STACK": "2", "RBRT_HELPERS": "2", "RBRT_WAVES_PER_CU": "3"},
     "no counter asserted"),
]
FLAGS = {"stripes_mixed": {"batches"}, "helpers_mid": {"batches"}, "extremes_lo": {"batches", "rank"},
         "extremes_hi": {"rank", "own_pipeline"}, "pipeline_0": {"own_pipeline"}, "pipeline_1": {"own_pipeline"},
         "pipeline_8": {"own_pipeline"}}
# knobs the matrix covers elsewhere: the BVH knobs in test_bvh_knobs_keep_the_brute_force_answer (below)
ELSEWHERE = {"RBRT_BVH_CT", "RBRT_BVH_SPATIAL", "RBRT_PLOC_RADIUS", "RBRT_BVH_DEVICE_MIN", "RBRT_BVH_DEVICE_ALGO"}
# set on every matrix row (the grid of every trace launch is read from its stderr line)
ALWAYS = {"RBRT_HIP_LAB": "1", "RBRT_POISON_SAMPLES": "1", "RBRT_TRACE_LAUNCHES": "1"}


def header_knobs():
    """Every RBRT_* name in the lab-knob comment of include/rbrt_hip_debug.h, but the two its first sentence names."""
    text = (ROOT / "include" / "rbrt_hip_debug.h").read_text()
    block = text[text.index("Lab knobs"):text.index("*/")]
    return sorted(set(re.findall(r"RBRT_[A-Z_]+[A-Z]", block)) - {"RBRT_HIP_LAB", "RBRT_ERR_INVALID_ARG"})


def test_every_header_knob_has_rows():
    """CPU: a knob listed in the header has a validation row and a matrix row here (or is covered by the BVH test)."""
    listed = header_knobs()
    assert len(listed) >= 29, listed
    in_matrix = {k for _, env, _ in MATRIX for k in env} | set(ALWAYS) | ELSEWHERE
    assert [k for k in listed if k not in VALID] == []
    assert [k for k in listed if k not in in_matrix] == []
    assert sorted(VALID) == listed  # (and nothing here that the header does not list)
    for name in VALID:  # the values the rows use are inside the stated ranges
        assert set(accepted_values(name)).isdisjoint(refused_values(name))
    for rid, env, _ in MATRIX:
        for k, v in env.items():
            if k in VALID:
                kind, lo, hi = VALID[k]
                assert lo <= int(v) <= hi and (kind != "pow2" or int(v) & (int(v) - 1) == 0), (rid, k, v)


# ---- validation ---------------------------------------------------------------------------------------------------------
def _create(sc):
    lib = abi.load_hip()
    h = C.c_void_p()
    rc = lib.rbrt_hip_scene_create(sc.ptr(), 0, C.byref(h))
    if rc == abi.RBRT_OK:
        lib.rbrt_hip_scene_destroy(h)
    return rc, lib.rbrt_hip_last_error().decode(errors="replace")


def _clear_knobs(monkeypatch):
    for k in VALID:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("RBRT_HIP_LAB", "1")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(VALID))
def test_scene_create_validates_the_knob(hip, oracle, monkeypatch, name):
    _clear_knobs(monkeypatch)
    sc = scenes.example_scene(oracle, 61)
    for v in accepted_values(name):
        monkeypatch.setenv(name, v)
        rc, msg = _create(sc)
        assert rc == abi.RBRT_OK, (name, v, msg)
    for v in refused_values(name):
        monkeypatch.setenv(name, v)
        rc, msg = _create(sc)
        assert rc == abi.RBRT_ERR_INVALID_ARG, (name, v, rc)
        assert name in msg, (name, v, msg)
    monkeypatch.delenv("RBRT_HIP_LAB")  # outside lab mode the same strings are not read at all
    for v in refused_values(name):
        monkeypatch.setenv(name, v)
        rc, msg = _create(sc)
        assert rc == abi.RBRT_OK, (name, v, msg)


def _build_host(md):
    lib = abi.load_hip()
    nodes, tris = C.c_void_p(), C.c_void_p()
    nn, nt, depth, me = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_float()
    rc = lib.rbrt_hip_bvh_build_host(C.byref(md.struct), C.byref(nodes), C.byref(nn), C.byref(tris), C.byref(nt),
                                     C.byref(depth), C.byref(me))
    if rc == abi.RBRT_OK:
        lib.rbrt_hip_free_host(nodes)
        lib.rbrt_hip_free_host(tris)
    return rc


def _build_records(recs):
    lib = abi.load_hip()
    nodes, tris = C.c_void_p(), C.c_void_p()
    nn, nt, depth, me = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_float()
    rc = lib.rbrt_hip_bvh_build_host_records(recs.ctypes.data_as(C.c_void_p), len(recs), C.byref(nodes), C.byref(nn),
                                             C.byref(tris), C.byref(nt), C.byref(depth), C.byref(me))
    if rc == abi.RBRT_OK:
        lib.rbrt_hip_free_host(nodes)
        lib.rbrt_hip_free_host(tris)
    return rc


def _build_device_refused(md):
    """rbrt_hip_bvh_build_device's return code for a knob value it must refuse (before it touches the device)."""
    lib = abi.load_hip()
    nodes, tris = C.c_void_p(), C.c_void_p()
    nn, nt, depth, me, built = C.c_size_t(), C.c_size_t(), C.c_uint32(), C.c_float(), C.c_int()
    return lib.rbrt_hip_bvh_build_device(C.byref(md.struct), C.byref(nodes), C.byref(nn), C.byref(tris), C.byref(nt),
                                         C.byref(depth), C.byref(me), C.byref(built))


@pytest.mark.parametrize("name", BVH_KNOBS)
def test_debug_builders_validate_the_bvh_knobs(oracle, monkeypatch, name):
    """CPU: the BVH debug entry points parse the BVH knobs on every call, with scene_create's rules."""
    _clear_knobs(monkeypatch)
    md = scenes.standin_mesh(oracle, 61, **scenes.EXAMPLE_MESH)
    recs = np.zeros((8, 12), np.float32)
    recs[:, 3] = recs[:, 7] = 1.0  # eight unit right triangles at the origin
    recs[:, 9] = np.arange(8, dtype=np.uint32).view(np.float32)
    lib = abi.load_hip()
    for v in accepted_values(name):
        monkeypatch.setenv(name, v)
        assert _build_host(md) == abi.RBRT_OK, (name, v)
        assert _build_records(recs) == abi.RBRT_OK, (name, v)
    for v in refused_values(name):
        monkeypatch.setenv(name, v)
        assert _build_host(md) == abi.RBRT_ERR_INVALID_ARG, (name, v)
        assert name.encode() in lib.rbrt_hip_last_error(), (name, v)
        assert _build_records(recs) == abi.RBRT_ERR_INVALID_ARG, (name, v)
        assert _build_device_refused(md) == abi.RBRT_ERR_INVALID_ARG, (name, v)
        assert name.encode() in lib.rbrt_hip_last_error(), (name, v)
    monkeypatch.delenv("RBRT_HIP_LAB")
    for v in refused_values(name):
        monkeypatch.setenv(name, v)
        assert _build_host(md) == abi.RBRT_OK, (name, v)


# ---- the matrix on the GPU ----------------------------------------------------------------------------------------------
SEED, STREAM_SEEDS = 7, (11, 12, 13, 14)


class Case:
    """One scene of the matrix: its camera, options and reference images (computed once per module)."""

    def __init__(self, name, sc, cam, spp, refs_of, **opt_kw):
        self.name, self.sc, self.cam, self.spp, self.opt_kw = name, sc, cam, spp, opt_kw
        self.refs = {seed: refs_of(cam, sc, self.opts(seed)) for seed in (SEED,) + STREAM_SEEDS}

    def opts(self, seed, flags=0):
        kw = dict(self.opt_kw)
        kw["flags"] = kw.get("flags", 0) | flags
        return abi.default_opts(spp=self.spp, seed=seed, **kw)


def _dielectric_spheres():
    """Spheres only, most of them glass (one inside another, a lens in front of a mirror): paths of many bounces and a
    long drain at max_depth 50."""
    L, M, D = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC
    return abi.SceneData(spheres=[
        ((0.0, -1000.0, -5.0), 1000.0, abi.material(L, (0.5, 0.5, 0.5))),
        ((0.0, 1.5, -9.0), 1.5, abi.material(D, (0, 0, 0), 1.5)),
        ((0.0, 1.5, -9.0), 1.2, abi.material(D, (0, 0, 0), 1.0 / 1.5)),
        ((-3.0, 1.2, -8.0), 1.2, abi.material(D, (0, 0, 0), 2.4)),
        ((3.0, 1.0, -7.0), 1.0, abi.material(D, (0, 0, 0), 1.33)),
        ((0.0, 4.0, -16.0), 4.0, abi.material(M, (0.95, 0.95, 0.95), 0.0)),
        ((-1.5, 0.6, -5.5), 0.6, abi.material(D, (0, 0, 0), 1.8)),
    ])


@pytest.fixture(scope="module")
def cases(oracle):
    orc = lambda cam, sc, o: oracle.render(cam, sc, o)[0]  # noqa: E731
    example = scenes.example_scene(oracle, 3001)
    lit = E.lit_scene(oracle)
    out = {
        "example": Case("example", example, scenes.camera(oracle, 100, 61), 4, orc),
        "glass": Case("glass", _dielectric_spheres(), scenes.camera(oracle, 72, 45), 3, orc, max_depth=50),
        "lit": Case("lit", lit, scenes.camera(oracle, 40, 27), 2, lambda cam, sc, o: E.restated_image(cam, sc, o)[0],
                    flags=CONST_BG, bg=(0.0, 0.0, 0.0)),
    }
    # the counting frame and the batched frame: the example scene at 200 x 150 x 5 (152,000 work items, more than the
    # lanes of a grid of one wave per CU hold, so that the shading rounds while work is left do run)
    big_cam = scenes.camera(oracle, 200, 150)
    big_opts = abi.default_opts(spp=5, seed=SEED)
    out["big"] = (big_cam, big_opts, oracle.render(big_cam, example, big_opts)[0])
    return out


def _launch_lines(err):
    """(grid, CUs, full-grid waves per CU) of every trace launch in the RBRT_TRACE_LAUNCHES lines."""
    return [tuple(int(x) for x in m) for m in re.findall(r"trace launch: grid (\d+) waves on (\d+) CUs \((\d+) waves per CU\)", err)]


def _frame(torch, case_cam):
    return torch.full((case_cam.img_height_pix, case_cam.img_width_pix, 3), float("nan"), dtype=torch.float32, device="cuda")


def _render_case(hip, torch, capfd, case, flags, what):
    """Blocking frame, stream of four, counting frame of one case. Returns the counters of the counting frame, the helper
    launches of the stream, and the trace-launch lines of the blocking frame and of the stream."""
    cam = case.cam
    with hip.HipScene(case.sc) as hs:
        hs.refine_wait(60.0)
        capfd.readouterr()
        out = _frame(torch, cam)
        hs.render_device(cam, case.opts(SEED), out.data_ptr())
        torch.cuda.synchronize()
        blocking_err = capfd.readouterr().err
        assert_same_image(out.cpu().numpy(), case.refs[SEED], f"{what} {case.name}: blocking frame")
        if "own_pipeline" not in flags:
            hs.set_pipeline(3)
        hs.set_timing(True)
        outs = [_frame(torch, cam) for _ in STREAM_SEEDS]
        for o, seed in zip(outs, STREAM_SEEDS):
            hs.render_device(cam, case.opts(seed), o.data_ptr())
        torch.cuda.synchronize()
        stream_err = capfd.readouterr().err
        n_helpers = hs.helper_launches()
        for o, seed in zip(outs, STREAM_SEEDS):
            assert_same_image(o.cpu().numpy(), case.refs[seed], f"{what} {case.name}: stream frame of seed {seed}")
        hs.render_device(cam, case.opts(SEED, STATS), out.data_ptr())
        torch.cuda.synchronize()
        assert_same_image(out.cpu().numpy(), case.refs[SEED], f"{what} {case.name}: counting frame")
        hs.check()
    return n_helpers, blocking_err, stream_err


def _count_big(hip, torch, cases, what):
    """The counting build on the big frame of the example scene: its image, and its counters."""
    cam, opts, ref = cases["big"]
    out = _frame(torch, cam)
    with hip.HipScene(cases["example"].sc) as hs:
        hs.refine_wait(60.0)
        o = abi.default_opts(spp=opts.spp, seed=opts.seed, flags=STATS)
        hs.render_device(cam, o, out.data_ptr())
        torch.cuda.synchronize()
        assert_same_image(out.cpu().numpy(), ref, f"{what}: counting frame 200x150x5")
        d = hs.debug_counters()
        hs.check()
    return d


def _set_env(monkeypatch, env):
    _clear_knobs(monkeypatch)
    monkeypatch.delenv("RBRT_HIP_WORKSPACE_MB", raising=False)
    for k, v in {**ALWAYS, **env}.items():
        monkeypatch.setenv(k, v)


COUNTER_KEYS = ("shade_extra_rounds", "leaf_rounds", "leaf_lanes", "stack_pushes_beyond_lds", "refill_rounds", "share_rounds",
                "trav_wave_steps")


@pytest.mark.gpu
@pytest.mark.parametrize("rid,env,effect", MATRIX, ids=[r[0] for r in MATRIX])
def test_knob_matrix_leaves_the_image_bit_identical(hip, cases, monkeypatch, capfd, record_property, rid, env, effect):
    import torch
    flags = FLAGS.get(rid, set())
    _set_env(monkeypatch, env)
    info = {}
    for name in ("example", "glass", "lit"):
        n_helpers, blocking_err, stream_err = _render_case(hip, torch, capfd, cases[name], flags, rid)
        info[name] = (n_helpers, _launch_lines(blocking_err), _launch_lines(stream_err), blocking_err)
        record_property(f"{name}_helpers", n_helpers)
        record_property(f"{name}_stream_grids", sorted({g for g, _, _ in info[name][2]}))
    counters = _count_big(hip, torch, cases, rid)
    for k in COUNTER_KEYS:
        record_property(k, counters[k])

    if "batches" in flags:  # several sample batches per frame (RBRT_HIP_WORKSPACE_MB=1)
        cam, opts, ref = cases["big"]
        out = _frame(torch, cam)
        with hip.HipScene(cases["example"].sc) as hs:
            hs.render_device(cam, opts, out.data_ptr())
            torch.cuda.synchronize()
            assert hs.last_batches()[1] >= 2, hs.last_batches()
            hs.check()
        assert_same_image(out.cpu().numpy(), ref, f"{rid}: batched frame")
    if "rank" in flags:  # tiles of rank 1 of 3 (the one-shot call)
        c = cases["example"]
        part, _ = hip.render_scene(c.cam, c.spp, c.sc, seed=SEED, tile_rank=1, tile_world=3)
        h, w = part.shape[:2]
        ty, tx = np.meshgrid(np.arange(h) // 8, np.arange(w) // 8, indexing="ij")
        mine = (tiles.tile_number(ty, tx, (w + 7) // 8) % 3) == 1
        assert_same_image(part[mine][None], c.refs[SEED][mine][None], f"{rid}: rank 1 of 3")

    # the knob took effect
    overlap_grid_seen = False
    for name, (_, blocking, stream, blocking_err) in info.items():
        assert blocking and stream, (rid, name)  # (every frame printed its trace launches)
        n_waves = blocking[0][1] * blocking[0][2]
        assert all(g == n_waves for g, _, _ in blocking), (rid, name, blocking)  # a blocking frame: the full grid
        if env.get("RBRT_PRIMARY_CULL") != "0":
            assert "full grid list_mode 4" in blocking_err, (rid, name)
        else:
            assert "tile pass" not in blocking_err and "list_mode" not in blocking_err, (rid, name)
        if "RBRT_WAVES_PER_CU" in env:
            k = int(env["RBRT_WAVES_PER_CU"])
            assert {(g, per) for g, cus, per in blocking + stream} == {(blocking[0][1] * k, k)}, (rid, name)
        elif env.get("RBRT_OVERLAP_WAVES_PER_CU", "0") != "0" and env.get("RBRT_PIPELINE") != "1":
            # a launch of the stream has the full grid when it finds the GPU idle, the knob's grid when it overlaps
            k = int(env["RBRT_OVERLAP_WAVES_PER_CU"])
            grids = {g for g, _, _ in stream}
            assert grids <= {min(blocking[0][1] * k, n_waves), n_waves}, (rid, name, grids)
            overlap_grid_seen |= min(blocking[0][1] * k, n_waves) in grids
        if env.get("RBRT_PIPELINE") == "1":
            assert all(g == n_waves for g, _, _ in stream), (rid, name, stream)  # one lane: nothing runs side by side
    if env.get("RBRT_OVERLAP_WAVES_PER_CU", "0") != "0" and "RBRT_WAVES_PER_CU" not in env and env.get("RBRT_PIPELINE") != "1":
        assert overlap_grid_seen, (rid, {n: i[2] for n, i in info.items()})  # (in one scene's stream at least)
    if env.get("RBRT_HELPERS") == "2":  # a helper launch with every overlapped launch of the streams
        assert sum(i[0] for i in info.values()) > 0, rid
    if rid in ("lds_stack_1", "extremes_lo"):
        assert counters["stack_pushes_beyond_lds"] > 1000
    if rid in ("lds_stack_64", "extremes_hi"):
        assert counters["stack_pushes_beyond_lds"] == 0
    if env.get("RBRT_SHARE_IDLE") == "64":
        assert counters["share_rounds"] == 0
    if rid == "leaf_leaves_1":  # against the other end of the range (the default's 35 is too close to compare with)
        _set_env(monkeypatch, {"RBRT_LEAF_LEAVES": "128", "RBRT_LEAF_ROUND": "64"})
        base = _count_big(hip, torch, cases, "leaf_leaves_128")
        ratio, base_ratio = (c["leaf_lanes"] / max(1, c["leaf_rounds"]) for c in (counters, base))
        record_property("leaf_lanes_per_round", (ratio, base_ratio))
        assert ratio < 0.6 * base_ratio, (ratio, base_ratio)
    if rid == "shade_64_cont_1":
        _set_env(monkeypatch, {"RBRT_WAVES_PER_CU": "1"})
        base = _count_big(hip, torch, cases, "shade_base_1wave")
        record_property("shade_extra_rounds_base", base["shade_extra_rounds"])
        assert counters["shade_extra_rounds"] > 1.4 * base["shade_extra_rounds"], (counters["shade_extra_rounds"], base["shade_extra_rounds"])


# ---- the BVH knobs: trees of another shape, the same answers ------------------------------------------------------------
BVH_ROWS = [
    ("ct_0.01", {"RBRT_BVH_CT": "0.01", "RBRT_BVH_BUILDER": "host"}, "host"),
    ("ct_1000", {"RBRT_BVH_CT": "1000", "RBRT_BVH_BUILDER": "host"}, "host"),
    ("spatial_0", {"RBRT_BVH_SPATIAL": "0", "RBRT_BVH_BUILDER": "host"}, "host"),
    ("spatial_0.6", {"RBRT_BVH_SPATIAL": "0.6", "RBRT_BVH_BUILDER": "host"}, "host"),
    ("ploc_1", {"RBRT_PLOC_RADIUS": "1", "RBRT_BVH_DEVICE_ALGO": "ploc", "RBRT_BVH_BUILDER": "device"}, "device"),
    ("ploc_256", {"RBRT_PLOC_RADIUS": "256", "RBRT_BVH_DEVICE_ALGO": "ploc", "RBRT_BVH_BUILDER": "device"}, "device"),
    ("lbvh_1", {"RBRT_PLOC_RADIUS": "1", "RBRT_BVH_DEVICE_ALGO": "lbvh", "RBRT_BVH_BUILDER": "device"}, "device"),
    ("lbvh_256", {"RBRT_PLOC_RADIUS": "256", "RBRT_BVH_DEVICE_ALGO": "lbvh", "RBRT_BVH_BUILDER": "device"}, "device"),
    # the device builder first, then the background build with the knobs scene_create parsed (refine_wait adopts it)
    ("device_min_0_refined", {"RBRT_BVH_DEVICE_MIN": "0", "RBRT_BVH_CT": "1000", "RBRT_BVH_SPATIAL": "0.6"}, "refined"),
    ("device_min_0", {"RBRT_BVH_DEVICE_MIN": "0", "RBRT_BVH_REFINE": "0", "RBRT_PLOC_RADIUS": "3"}, "device"),
    ("device_min_above_all", {"RBRT_BVH_DEVICE_MIN": str(1 << 30)}, "host"),
]


@pytest.fixture(scope="module")
def bvh_case(oracle):
    sc = scenes.example_scene(oracle, 3001, kind="rough")
    cam = scenes.camera(oracle, 100, 61)
    opts = abi.default_opts(spp=3, seed=SEED)
    md = sc.meshes[0]
    rng = np.random.default_rng(17)
    c, R = (md.bbox_lo + md.bbox_hi) / 2, float(np.linalg.norm(md.bbox_hi - md.bbox_lo) / 2)
    o = c + rng.normal(size=(20000, 3)) * R * 2.0
    d = (c + rng.uniform(-1, 1, (20000, 3)) * R) - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(0.2, 3.0, (20000, 1))
    rays = np.concatenate([o, d], 1).astype(np.float32)
    return sc, cam, opts, oracle.render(cam, sc, opts)[0], rays, oracle.trace_rays(sc, rays)


@pytest.mark.gpu
@pytest.mark.parametrize("rid,env,builder", BVH_ROWS, ids=[r[0] for r in BVH_ROWS])
def test_bvh_knobs_keep_the_brute_force_answer(hip, bvh_case, monkeypatch, rid, env, builder):
    import torch
    sc, cam, opts, ref, rays, (et, eo, ei, _) = bvh_case
    _set_env(monkeypatch, env)
    for k in ("RBRT_BVH_BUILDER", "RBRT_BVH_REFINE"):
        if k not in env:
            monkeypatch.delenv(k, raising=False)
    out = _frame(torch, cam)
    with hip.HipScene(sc) as hs:
        state, _ = hs.refine_wait(120.0)
        assert state == (1 if builder == "refined" else 0), state
        assert hs.create_times()["meshes_device_built"] == (0 if builder == "host" else 1)
        hs.render_device(cam, opts, out.data_ptr())
        torch.cuda.synchronize()
        gt, go, gi, _ = hs.trace_rays(rays)
        hs.check()
    assert_same_image(out.cpu().numpy(), ref, rid)
    assert np.array_equal(eo, go) and np.array_equal(ei, gi) and np.array_equal(et.view(np.uint32), gt.view(np.uint32)), rid
    assert (go == len(sc.spheres)).sum() > 1000  # (the mesh is hit)


@pytest.mark.gpu
def test_device_min_puts_a_small_mesh_on_the_device_builder(hip, oracle, monkeypatch):
    """RBRT_BVH_DEVICE_MIN=9, above the 8-entry floor below which the device builder declines: a mesh of a few more entries
    goes to the device builder and renders the oracle's image; one above its entry count sends it to the host builder."""
    import torch
    sc = scenes.example_scene(oracle, 12)
    n_total = sc.meshes[0].n_total
    assert 9 <= n_total < 32
    cam = scenes.camera(oracle, 64, 40)
    opts = abi.default_opts(spp=3, seed=SEED)
    ref = oracle.render(cam, sc, opts)[0]
    for device_min, n_device in (("9", 1), (str(n_total + 1), 0), (str(n_total), 1), ("0", 1)):
        _set_env(monkeypatch, {"RBRT_BVH_DEVICE_MIN": device_min, "RBRT_BVH_REFINE": "0"})
        out = _frame(torch, cam)
        with hip.HipScene(sc) as hs:
            assert hs.create_times()["meshes_device_built"] == n_device, device_min
            hs.render_device(cam, opts, out.data_ptr())
            torch.cuda.synchronize()
            hs.check()
        assert_same_image(out.cpu().numpy(), ref, f"RBRT_BVH_DEVICE_MIN={device_min}")
