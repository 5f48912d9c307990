"""Scenes that use every per-sample feature at once, for tests/test_np_whole.py (CPU) and tests/test_whole_gpu.py: the fuzzed
scene kinds of full_scenes.fuzz_case (emitters, backgrounds, the lens, smooth and flat meshes, shuffled BasicTriangles, distance
windows, depth 0 / 1 / 3, ragged sizes) with solid patterns, a shutter, moving spheres, a phase and an environment on top; and
one hand-built scene with everything.

The generator is seeded and deterministic: what a case holds is in case["has"], a set of the names in FEATURES, so that the
coverage of the feature pairs can be established from the descriptors alone."""
from __future__ import annotations

import os
from types import SimpleNamespace

import numpy as np

import full_scenes as F
import np_env
import np_lens
import scenes
from rbrt_amd import abi

f32 = np.float32
L_, M_, D_, EM = abi.MAT_LAMBERTIAN, abi.MAT_METAL, abi.MAT_DIELECTRIC, abi.MAT_EMISSIVE
T = scenes.T
N_FUZZ = int(os.environ.get("RBRT_FUZZ_WHOLE_SCENES", "24"))
PHASES = (0.0, 0.5, -3.0, 7.0, 4096.25)  # (the last one: phase + t loses the low 13 bits of t)
FEATURES = ("lens", "shutter", "motion", "phase", "environment", "pattern_on_a_moving_sphere", "pattern_on_a_mesh", "smooth_mesh",
            "basic_triangle", "emitter", "constant_background")
STREAM = 173000       # the generator's own random stream is default_rng(STREAM + seed)
EQUAL_COLOURS_SEED = 4 # the case whose patterns all have albedo2 == albedo
ZERO_MOTION_SEED = 9    # the case whose motion is all zero (and still draws)


def element_order(sc):
    return sc.element_order if sc.element_order is not None else list(range(len(sc.spheres))) + [T | i for i in range(len(sc.triangles))]


def object_materials(sc):
    """[object id] -> material: the elements in their order, the meshes behind them."""
    return [sc.triangles[e & 0x7FFFFFFF][1] if e >> 31 else sc.spheres[e][2] for e in element_order(sc)] + [md.struct.mat for md in sc.meshes]


def with_patterns(sc, patterns):
    return abi.SceneData(spheres=sc.spheres, meshes=sc.meshes, triangles=sc.triangles, element_order=sc.element_order, patterns=patterns)


def unit(rng):
    v = rng.normal(size=3)
    return v / np.linalg.norm(v)


def log_uniform(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def fuzz_case(oracle, seed):
    """full_scenes.fuzz_case(oracle, seed, tiny=True) -- at most 12 x 9 pixels, 2 spp, depth 0 / 1 / 3 -- and on top of it:
    checkers on most of the lambertian objects (spheres, BasicTriangles, flat and smooth meshes), cells from 2e-3 units (far
    below a pixel's footprint) to 80 (larger than everything but the ground), origins anywhere; a shutter that is absent, zero,
    small or comparable to the scene; a motion (absent in one case of seven) whose travels are zero, small or, for one sphere,
    long enough to carry it out of the frame within the exposure; a phase of PHASES; in half of the cases a noise environment
    of N = 1, 2 or 8, under which a non-black bg and, where the base case has it, the constant flag stay set.

    One object is added to three cases of four: a lambertian sphere on the view axis. The base draws a material's kind from
    four, a third of its tiny cases have depth 0 and most of its objects cover a pixel or two, so without it only one patterned
    case in ten ever scatters from a patterned object twice (tests/test_np_whole.py asks for both colours in a third of them).
    STREAM is the first of 170000, 171000, ... whose 24 cases have every pair of FEATURES and that third.
    -> a namespace: cam, lens, sc, opts, builder, shutter, travels, phase, nodes, has, patterns, what."""
    base = F.fuzz_case(oracle, seed, tiny=True)
    rng = np.random.default_rng(STREAM + seed)
    sc0, cam, lens, opts0 = base["sc"], base["cam"], base["lens"], base["opts"]
    if rng.random() < 0.75:  # a lambertian sphere of the generator's own on the view axis (see the docstring)
        pos = np.array(list(cam.position), np.float64)
        axis = np.array(list(cam.img_center_point), np.float64) - pos
        centre = pos + rng.uniform(6.0, 11.0) * axis / np.linalg.norm(axis) + rng.uniform(-0.7, 0.7, 3)
        own = (tuple(float(x) for x in centre), float(rng.uniform(1.0, 2.5)), F.mat(rng, (L_,)))
        order0 = None if sc0.element_order is None else list(sc0.element_order)
        if order0 is not None:
            order0.insert(int(rng.integers(len(order0) + 1)), len(sc0.spheres))
        sc0 = abi.SceneData(spheres=sc0.spheres + [own], meshes=sc0.meshes, triangles=sc0.triangles, element_order=order0)
    order, mats = element_order(sc0), object_materials(sc0)
    n_elem = len(order)
    # patterns
    patterns = {}
    for k, m in enumerate(mats):
        if int(m.kind) == L_ and rng.random() < 0.85:
            a2 = tuple(m.albedo) if seed == EQUAL_COLOURS_SEED else tuple(float(x) for x in rng.uniform(0.0, 1.0, 3))
            size = log_uniform(rng, *((2e-3, 2e-2), (0.05, 2.0), (0.05, 2.0), (20.0, 80.0))[int(rng.integers(4))])
            patterns[k] = abi.checker(a2, size, tuple(float(x) for x in rng.uniform(-3.0, 3.0, 3)))
    sc = with_patterns(sc0, patterns) if patterns else sc0
    # the shutter
    kind = int(rng.integers(4))
    shutter = (None, (0.0, 0.0, 0.0), tuple(float(f32(v)) for v in log_uniform(rng, 1e-3, 0.3) * unit(rng)),
               tuple(float(f32(v)) for v in log_uniform(rng, 2.0, 12.0) * unit(rng)))[kind]
    # the motion
    travels = None
    if rng.random() < 0.85 or seed == ZERO_MOTION_SEED:
        travels = np.zeros((len(sc.spheres), 3), f32)
        if seed != ZERO_MOTION_SEED:
            far = int(rng.integers(len(sc.spheres))) if sc.spheres and rng.random() < 0.4 else -1
            for i in range(len(sc.spheres)):
                patterned = order.index(i) in patterns
                if i == far and sc.spheres[i][1] < 100.0:  # (not the ground: a sphere that leaves the frame within the exposure)
                    travels[i] = log_uniform(rng, 30.0, 80.0) * unit(rng)
                elif rng.random() < (0.9 if patterned else 0.6):
                    travels[i] = log_uniform(rng, 1e-3, 1.5) * unit(rng)
    phase = float(PHASES[int(rng.integers(len(PHASES)))])
    # the environment; bg and the flag stay set under it
    nodes = None
    kw = dict(max_depth=opts0.max_depth, min_dist=opts0.min_dist, max_dist=opts0.max_dist, bg=tuple(opts0.bg), flags=opts0.flags)
    if rng.random() < 0.5:
        nodes = np_env.noise_map(int(rng.choice([1, 2, 8])), 500 + seed)
        if not any(kw["bg"]):
            kw["bg"] = tuple(float(x) for x in rng.uniform(0.2, 2.0, 3))
    opts = abi.default_opts(spp=opts0.spp, seed=opts0.seed, **kw)
    moving = set() if travels is None else {i for i in range(len(sc.spheres)) if travels[i].any()}
    has = set()
    for name, there in (("lens", lens is not None), ("shutter", shutter is not None), ("motion", travels is not None),
                        ("phase", phase != 0.0), ("environment", nodes is not None),
                        ("pattern_on_a_moving_sphere", any(not order[k] >> 31 and order[k] in moving for k in patterns if k < n_elem)),
                        ("pattern_on_a_mesh", any(k >= n_elem for k in patterns)), ("smooth_mesh", any(md.normals is not None for md in sc.meshes)),
                        ("basic_triangle", bool(sc.triangles)), ("emitter", any(int(m.kind) == EM for m in mats)),
                        ("constant_background", bool(opts.flags & abi.FLAG_CONSTANT_BACKGROUND))):
        if there:
            has.add(name)
    what = (f"{base['what']}; patterns on {sorted(patterns)}, shutter {shutter}, motion "
            f"{'none' if travels is None else [round(float(np.linalg.norm(t)), 3) for t in travels]}, phase {phase}, "
            f"environment {None if nodes is None else nodes.shape[0] - 1}")
    return SimpleNamespace(cam=cam, lens=lens, sc=sc, opts=opts, builder=base["builder"], shutter=shutter, travels=travels, phase=phase,
                           nodes=nodes, has=has, patterns=patterns, what=what)


def restate(NW, case, **kw):
    """np_whole.restated_image of a case (NW: the module), with what the caller adds (pixels=, traces=, scatters=)."""
    return NW.restated_image(case.cam, case.sc, case.opts, lens=case.lens, shutter=case.shutter, travels=case.travels, phase=case.phase,
                             nodes=case.nodes, **kw)


def configure(hs, case):
    """Puts a handle of case.sc into the case's state."""
    if case.nodes is not None:
        hs.set_environment(case.nodes)
    hs.set_shutter(case.shutter)
    hs.set_motion(case.travels)
    hs.set_motion_phase(case.phase)
    return hs


# ---- one scene with everything ---------------------------------------------------------------------------------------------------
HAND_TRAVELS = np.array([(0.0, 0.0, 0.0), (0.9, 0.0, 0.0), (-0.4, 0.3, 0.5), (0.0, 0.6, -0.7), (-1.1, -0.2, 0.0)], f32)
HAND_SHUTTER = (0.3, -0.2, 0.1)
HAND_PHASE = 0.5
HAND_MOVING = 1  # the object id of the patterned sphere that moves (sphere 1, the blue lambertian)


def hand_scene(oracle, mesh=False):
    """The example spheres and an emitter; the ground and the moving lambertian sphere patterned (cells of 1.5 and 0.4 units,
    so that the first hits of one sphere see both colours); a metal BasicTriangle between them in the element order; mesh: a
    13-entry stand-in in front of them."""
    sph = list(scenes.EXAMPLE_SPHERES) + [((3.5, 1.0, -7.0), 1.0, abi.material(EM, (3.0, 2.5, 1.5)))]
    tris = [(((-4.0, 0.3, -6.0), (-1.5, 0.4, -6.5), (-2.7, 2.6, -7.0)), abi.material(M_, (0.9, 0.6, 0.3), 0.05))]
    meshes = [scenes.standin_mesh(oracle, 13, 25.0, (0.5, -0.6, -4.5), (0.0, 0.4, 0.0), abi.material(M_, (0.8, 0.7, 0.6), 0.05))] if mesh else []
    patterns = {0: abi.checker((0.8, 0.8, 0.7), 1.5, (0.13, -0.21, 0.37)), HAND_MOVING: abi.checker((0.9, 0.2, 0.1), 0.4, (-0.31, 0.17, 0.05))}
    return abi.SceneData(spheres=sph, meshes=meshes, triangles=tris, element_order=[0, 1, T | 0, 2, 3, 4], patterns=patterns)


def hand_case(oracle, w, h, spp, seed=7, depth=8, mesh=False, **state):
    """hand_scene under the example camera with a lens, HAND_SHUTTER, HAND_TRAVELS at HAND_PHASE and a noise environment of
    N = 8; `state` replaces any of lens, shutter, travels, phase, nodes, cam."""
    cam = state.pop("cam", None) or scenes.camera(oracle, w, h)
    lens = np_lens.lens_for(cam, scenes.CAMERA["look_at"], scenes.CAMERA["focal_mm"], 40.0, 9.0)
    c = SimpleNamespace(cam=cam, lens=lens, sc=hand_scene(oracle, mesh), opts=abi.default_opts(spp=spp, seed=seed, max_depth=depth, bg=(0.4, 0.3, 0.2)),
                        builder=None, shutter=HAND_SHUTTER, travels=HAND_TRAVELS, phase=HAND_PHASE, nodes=np_env.noise_map(8, 3))
    for k, v in state.items():
        setattr(c, k, v)
    return c


# ---- one handle through its states -------------------------------------------------------------------------------------------------
WALK_W, WALK_H, WALK_SPP, WALK_STEPS = 20, 12, 2, 16
KINDS = ("shutter", "motion", "phase", "environment", "camera", "lens")
SHUTTERS = (HAND_SHUTTER, (0.0, 0.0, 0.0), (-0.5, 0.1, 0.2))
MOTIONS = (HAND_TRAVELS, (HAND_TRAVELS * f32(-0.5)).astype(f32), np.zeros_like(HAND_TRAVELS))
WALK_PHASES = (0.0, 0.5, -3.0, 7.0)
CAMERAS = ({}, dict(position=(0.6, 4.6, 4.4)))


def walk():
    """The seeded sequence of single changes: a list of (what changed, state after it), state = dict(shutter, motion, phase,
    environment, camera, lens) of indices into the tables above (None: not set). It starts from a handle with nothing set, the
    first camera and no lens; a change always changes the state."""
    rng = np.random.default_rng(16)
    state = dict(shutter=None, motion=None, phase=0, environment=None, camera=0, lens=0)
    n_of = dict(shutter=len(SHUTTERS), motion=len(MOTIONS), environment=2)
    out = []
    for _ in range(WALK_STEPS):
        kind = KINDS[int(rng.integers(len(KINDS)))]
        if kind in n_of:
            if state[kind] is None:
                state[kind], what = int(rng.integers(n_of[kind])), f"set {kind}"
            elif rng.random() < 0.4:
                state[kind], what = None, f"clear {kind}"
            else:
                state[kind], what = (state[kind] + 1 + int(rng.integers(n_of[kind] - 1))) % n_of[kind], f"replace {kind}"
        elif kind == "phase":
            state[kind], what = (state[kind] + 1 + int(rng.integers(len(WALK_PHASES) - 1))) % len(WALK_PHASES), "change phase"
        else:
            state[kind], what = 1 - state[kind], f"swap {kind}"
        out.append((what, dict(state)))
    return out


def walk_case(oracle, state):
    """hand_case in a state of walk()."""
    cam = scenes.camera(oracle, WALK_W, WALK_H, **CAMERAS[state["camera"]])
    case = hand_case(oracle, WALK_W, WALK_H, WALK_SPP, seed=11, depth=6, cam=cam,
                     shutter=None if state["shutter"] is None else SHUTTERS[state["shutter"]],
                     travels=None if state["motion"] is None else MOTIONS[state["motion"]], phase=WALK_PHASES[state["phase"]],
                     nodes=None if state["environment"] is None else np_env.noise_map((8, 2)[state["environment"]], 3 + state["environment"]))
    if not state["lens"]:
        case.lens = None
    return case
