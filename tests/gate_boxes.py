"""Boxes and rays for the mesh gate (aabbox.rs:28-58; kernels.hip bbox_gate / bbox_gate_fast): shared by the condition on
the inputs in test_np_reference.py (numpy alone) and the device test in test_gpu_parity.py."""
import numpy as np

GATE_SPECIALS = np.float32([0.0, -0.0, 1e-38, -1e-38, 1e-31, 1e31, np.inf, -np.inf, np.nan, 1.0, -1.0])
# name -> (lo, hi, direction scales). The quotients the gate forms are (bound - o) / d with d = (target - o) * scale, about
# 1 / scale whatever the box: the scales of the last two boxes put them from 1e28 to 1e32 and from 1e-32 to 1e-28, either
# side of the gate's own cut-offs m < 1e30 and m > 1e-30, with direction components (1e-22, 1e22) well inside its others.
GATE_SCALES = np.float32([1e-20, 1e-3, 0.3, 1.0, 1.0, 7.0, 1e4, 1e20])
GATE_BOXES = {
    "config2": ([0.7825403, 0.57846975, -15.222859], [7.573573, 7.4303217, -9.879498], None),  # (None: the rays this test always had)
    "config2_long_and_short": ([0.7825403, 0.57846975, -15.222859], [7.573573, 7.4303217, -9.879498], GATE_SCALES),
    "around_the_origin": ([-1.5, -0.25, -3.0], [2.0, 0.75, 1.0], GATE_SCALES),
    "flat": ([-2.0, 1.25, -7.0], [3.0, 1.25, -4.0], GATE_SCALES),
    "point": ([0.3, -1.7, 2.9], [0.3, -1.7, 2.9], GATE_SCALES),
    "far+1e5": ([1e5, 1e5, -1e5], [1e5 + 1, 1e5 + 1, -1e5 + 1], GATE_SCALES),
    "far-3e4": ([-3e4, 1e4, -2e4], [-3e4 + 1, 1e4 + 1, -2e4 + 1], GATE_SCALES),
    "1e-4_across": ([0.5, -0.25, 0.125], [0.5001, -0.2499, 0.1251], GATE_SCALES),
    "1e6_across": ([-3e5, -6e5, -1e6], [7e5, 4e5, 0.0], GATE_SCALES),
    "empty_mesh": (None, None, GATE_SCALES),  # (what mesh_prep gives a mesh without triangles)
    "quotients_near_1e30": ([1e8, -3e8, 2e8], [2e8, -2e8, 3e8], np.float32([1e-28, 1e-29, 3e-30, 1e-30, 3e-31, 1e-31, 1e-32])),
    "quotients_near_1e-30": ([1e-8, -3e-8, 2e-8], [2e-8, -2e-8, 3e-8], np.float32([1e28, 1e29, 3e29, 1e30, 3e30, 1e31, 1e32])),
}


def gate_rays(name, lo, hi, scales):
    """Rays for one box: origins around it (inside it, near it, far from it, and around the world's origin), aimed at points
    ON its surface -- a face point, snapped to edges and corners for a third of the rays --, scaled, nudged by -3..+3 ulp
    per component; then the table of special components from origins on, inside and outside the box. Returns (rays, number
    of the special ones at the end, the generator where the drawing left it)."""
    import zlib
    n = 400_000
    if scales is None:  # config 2's box, as this test always drew them
        rng = np.random.default_rng(11)
        o = (rng.normal(size=(n, 3)) * 12).astype(np.float32)
        t = rng.uniform(lo, hi, (n, 3)).astype(np.float32)
        for k in range(3):
            snap = rng.random(n) < 0.55
            t[snap, k] = np.where(rng.random(snap.sum()) < 0.5, lo[k], hi[k])
        d = (t - o).astype(np.float32)
        d *= rng.choice(np.float32([1e-3, 0.3, 1.0, 1.0, 7.0, 1e4]), (n, 1))
        inside = [4, 4, -12]
    else:
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        if np.abs(lo).max() > 1e37:  # the inverted box of an empty mesh: no surface to aim at
            c, half, t = np.zeros(3), 1.0, (rng.normal(size=(n, 3)) * 10).astype(np.float32)
        else:
            c = (lo.astype(np.float64) + hi) / 2
            half = float(np.linalg.norm(hi.astype(np.float64) - lo) / 2) or 1.0
            t = (lo + rng.random((n, 3)) * (hi.astype(np.float64) - lo)).astype(np.float32)
            for k in range(3):
                snap = rng.random(n) < 0.55
                t[snap, k] = np.where(rng.random(snap.sum()) < 0.5, lo[k], hi[k])
        spread = rng.choice([0.5, 2.0, 20.0, 0.0], (n, 1))
        o = np.where(spread > 0, c + rng.normal(size=(n, 3)) * spread * half, rng.normal(size=(n, 3)) * 12).astype(np.float32)
        with np.errstate(over="ignore"):
            d = (t - o).astype(np.float32) * rng.choice(scales, (n, 1))
        inside = c.astype(np.float32)
    ulps = rng.integers(-3, 4, (n, 3))
    d = (d.view(np.int32) + ulps.astype(np.int32)).view(np.float32)  # nudge by a few ulp either way
    rays = np.concatenate([o, d], 1)
    # axis-parallel and degenerate directions, origins on / inside / outside the box
    extra = []
    for a in GATE_SPECIALS:
        for b in GATE_SPECIALS:
            for org in ([0, 0, 0], inside, lo, hi, [lo[0], inside[1], inside[2]], [inside[0], hi[1], 30], [np.nan, 0, 0], [np.inf, 0, 0]):
                extra.append([*org, a, b, -1.0])
                extra.append([*org, -0.5, a, b])
                extra.append([*org, b, 0.25, a])
    return np.concatenate([rays, np.float32(extra)]).astype(np.float32), len(extra), rng


def gate_box(oracle, name):
    lo, hi, scales = GATE_BOXES[name]
    if lo is None:
        md = oracle.mesh_prep(np.zeros((0, 3, 3), np.float32))
        lo, hi = md.bbox_lo, md.bbox_hi
    return np.float32(lo), np.float32(hi), scales
