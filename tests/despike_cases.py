"""Inputs for the spike removal's tests (test_np_despike.py without a GPU, test_despike_gpu.py with one): two half images, made
once per size and never changed.

The base is smooth, with mild independent noise in each half, an all-zero region and one pixel with a negative channel. On it
spikes are planted, where the image is large enough to hold them: in A only, in B only, in both halves at one pixel (equal, and
unequal); clusters of 1 to 5 adjacent pixels; in the four corners and on the borders; in the columns TW - 1 and TW and the rows
TH - 1 and TH either side of the kernel's tile edge, and R and R + 1 pixels away from it for both radii, where a neighbour is the
last one inside a workgroup's halo or the first one outside; and a sprinkling at random. With nonfinite=True there are NaN,
+inf and -inf too: as centres, in one channel and in all, in one half and in both, and next to spikes as their neighbours.
No spike lies in or next to the all-zero region, so that a huge threshold leaves the clean case untouched."""
from __future__ import annotations

import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

f32 = np.float32
_debug = (Path(__file__).resolve().parent.parent / "include" / "rbrt_hip_debug.h").read_text()
TW, TH = (int(re.search(rf"#define RBRT_DESPIKE_TILE_{k} (\d+)u", _debug).group(1)) for k in "WH")
SPIKE = np.array([3000.0, 2700.0, 2100.0], f32)

#         W   H
SIZES = [(1, 1), (2, 2), (5, 3), (67, 1), (1, 23), (TW - 1, TH - 1), (TW, TH), (TW + 1, TH + 1), (2 * TW, 2 * TH), (3 * TW + 1, 3 * TH + 2)]
MAIN = (3 * TW + 1, 3 * TH + 2)  # an interior workgroup with halos on all four sides

CLUSTERS = {1: [(0, 0)], 2: [(0, 0), (0, 1)], 3: [(0, 0), (0, 1), (1, 0)], 4: [(0, 0), (0, 1), (1, 0), (1, 1)],
            5: [(0, 0), (0, 1), (1, 0), (1, 1), (0, 2)]}


def zero_region(W, H):
    """(y0, y1, x0, x1) of the all-zero block, or None where the image is too small for one."""
    if W < 24 or H < 12:
        return None
    return H - 5, H - 2, 12, 17


def _near_zero_region(W, H, y, x, margin=3):
    z = zero_region(W, H)
    return z is not None and z[0] - margin <= y < z[1] + margin and z[2] - margin <= x < z[3] + margin


@functools.lru_cache(maxsize=None)
def case(W, H, nonfinite=False):
    """-> namespace(W, H, a, b float32 [H, W, 3]; spikes_a, spikes_b bool [H, W]: where a spike was planted; bad bool [H, W]: where
    something is not finite)."""
    rng = np.random.default_rng(7000 + 100 * W + H)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    tone = 0.35 + 0.2 * np.sin(xs / 7.0) + 0.1 * np.cos(ys / 5.0)
    base = np.stack([tone * 0.9, tone * 1.0, tone * 0.6], -1)
    a = (base * (1.0 + rng.normal(0.0, 0.05, base.shape))).astype(f32)
    b = (base * (1.0 + rng.normal(0.0, 0.05, base.shape))).astype(f32)
    z = zero_region(W, H)
    if z:
        a[z[0]:z[1], z[2]:z[3]] = 0
        b[z[0]:z[1], z[2]:z[3]] = 0
    planted = {"a": np.zeros((H, W), bool), "b": np.zeros((H, W), bool)}
    halves = {"a": a, "b": b}

    def put(which, y, x, scale=1.0, shape=1):
        for dy, dx in CLUSTERS[shape]:
            yy, xx = y + dy, x + dx
            if 0 <= yy < H and 0 <= xx < W and not _near_zero_region(W, H, yy, xx):
                for h in which:
                    halves[h][yy, xx] = SPIKE * f32(scale)
                    planted[h][yy, xx] = True

    # corners and borders
    put("a", 0, 0), put("b", 0, W - 1), put("ab", H - 1, 0), put("a", H - 2, W - 2, shape=4)
    put("a", 0, W // 2), put("b", H // 2, 0), put("b", H - 1, W // 3, shape=2), put("a", H // 3, W - 1)
    # either side of a tile edge: single pixels and clusters that straddle it
    put("a", 3, TW - 1), put("b", 5, TW), put("b", TH - 1, 5), put("a", TH, 9)
    put("a", 1, TW - 1, shape=2), put("b", TH - 1, 20, shape=3), put("a", TH - 1, TW - 1, shape=4), put("b", 2 * TH - 1, 2 * TW - 2, shape=5)
    # R and R + 1 away from a tile edge, for R = 1 and 2: pairs whose partner is the last pixel inside a halo or the first outside
    for R in (1, 2):
        row = TH + 2 * R
        put("a", row, TW - R), put("a", row, TW), put("b", row, TW - R - 1), put("b", row, TW)           # left of the edge
        put("a", row + 1, TW + R - 1, 0.5), put("a", row + 1, TW - 1, 0.5), put("b", row + 1, TW + R, 0.5), put("b", row + 1, TW - 1, 0.5)
        col = 3 + 7 * R
        put("a", TH - R, col), put("a", TH, col), put("b", TH - R - 1, col + 3), put("b", TH, col + 3)   # above the edge
        put("a", 2 * TH + R - 1, col), put("a", 2 * TH - 1, col), put("b", 2 * TH + R, col + 3), put("b", 2 * TH - 1, col + 3)
    # clusters of 1 to 5 in each half, inside the interior workgroup where there is one
    for n in range(1, 6):
        put("a", TH + 1 + (n % 2) * 3, TW + 2 + 5 * n, 0.3 * n, shape=n)
        put("b", 2 * TH + 2, TW + 1 + 5 * n, 0.2 * n, shape=n)
    # both halves at one pixel: equal (never limited), and unequal
    put("ab", H // 2, W // 2)
    if H > 4 and W > 8:
        put("a", H // 2 + 2, W // 2 + 3), put("b", H // 2 + 2, W // 2 + 3, 0.01)
    # a sprinkling at random: one pixel in 60 of each half
    for which in ("a", "b"):
        for _ in range(W * H // 60):
            put(which, int(rng.integers(H)), int(rng.integers(W)), float(rng.uniform(0.01, 1.0)))
    # a negative channel
    if H > 2 and W > 3 and not _near_zero_region(W, H, 2, 3):
        a[2, 3, 2] = f32(-0.05)
        b[2, 3, 0] = f32(-2.0)  # (its luminance is negative)
    bad = np.zeros((H, W), bool)
    if nonfinite:
        nan, inf = f32(np.nan), f32(np.inf)

        def poison(img, y, x, value, channel=None):
            if 0 <= y < H and 0 <= x < W:
                if channel is None:
                    img[y, x] = value
                else:
                    img[y, x, channel] = value
                bad[y, x] = True

        poison(a, 0, 0, nan) if W * H == 1 else None          # the one pixel there is
        poison(a, 1, 3, nan, 0), put("a", 1, 4)               # a NaN next to a spike
        poison(b, H - 2, W - 3, inf), put("b", H - 2, W - 4)
        poison(a, TH, TW - 1, -inf, 1), put("a", TH, TW)      # either side of a tile edge
        poison(b, TH - 1, TW, nan), poison(a, TH - 1, TW, inf, 2)   # both halves at one pixel
        poison(a, H - 1, W - 1, inf), poison(b, 0, W // 2 + 1, -inf)
        poison(a, 2 * TH + 1, 2 * TW + 1, nan), poison(a, 2 * TH + 1, 2 * TW + 2, inf), poison(a, 2 * TH + 2, 2 * TW + 1, -inf)  # a non-finite cluster
        if H > 6:
            a[H // 2 + 1, 0, :2] = f32(3e38)  # finite, and huge: t * base overflows next to it
    out = SimpleNamespace(W=W, H=H, a=a, b=b, spikes_a=planted["a"], spikes_b=planted["b"], bad=bad)
    for x in (a, b, planted["a"], planted["b"], bad):
        x.flags.writeable = False
    return out
