"""Inputs for the image comparison's tests (test_np_compare.py without a GPU, test_compare_gpu.py with one): an image X and a
reference R, made once per size and kind and never changed.

R is a smooth HDR image (a bright band of about 20 beside tones below 1) and X is R with independent noise of 10 %. Kinds:
  "clean"     nothing else: every pixel is usable and every sum is finite.
  "mixed"     NaN, +inf, -inf and negative channels are planted in X, in R or in both, where the image is large enough to hold
              them: in the corners, as centres inside a tile, in the rows and columns TILE - 1 and TILE either side of a tile's
              edge, and 5 and 6 pixels away from it, where a pixel is the last one inside a workgroup's halo or the first one
              outside. What is not finite is skipped by the sums, so they stay finite.
  "overflow"  "clean" with one finite channel of X at 1e25, whose squared error is infinite.
"""
from __future__ import annotations

import functools
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np

f32 = np.float32
_header = (Path(__file__).resolve().parent.parent / "include" / "rbrt_hip.h").read_text()
TW, TH = (int(re.search(rf"#define RBRT_COMPARE_TILE_{k} (\d+)u", _header).group(1)) for k in "WH")
HALO = 5

#         W   H
SIZES = [(1, 1), (3, 3), (1, 40), (40, 1), (15, 17), (16, 16), (17, 15), (33, 47), (49, 50)]
MANY_TILES = [(272, 260), (1, 8200)]  # 289 tiles: the reduce kernel's lanes wrap once; 513: twice
MAIN = (33, 47)
SMALL = [(1, 1), (3, 3), (1, 20), (19, 18)]  # what the scalar evaluation of test_np_compare.py can afford


@functools.lru_cache(maxsize=None)
def case(W, H, kind="mixed"):
    """-> namespace(W, H, x, r float32 [H, W, 3]; bad bool [H, W]: where a channel of X or R is not finite)."""
    assert kind in ("clean", "mixed", "overflow")
    rng = np.random.default_rng(9000 + 100 * W + H)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    tone = 0.4 + 0.25 * np.sin(xs / 6.0) + 0.12 * np.cos(ys / 4.0) + 20.0 * (np.abs(xs - ys - 3.0) < 2.0)
    base = np.stack([tone * 0.9, tone * 1.0, tone * 0.55], -1)
    r = base.astype(f32)
    x = (base * (1.0 + rng.normal(0.0, 0.1, base.shape))).astype(f32)
    bad = np.zeros((H, W), bool)

    def poison(img, y, x_, value, channel=None):
        if 0 <= y < H and 0 <= x_ < W:
            img[y, x_, slice(None) if channel is None else channel] = value
            if not np.isfinite(value):
                bad[y, x_] = True

    if kind == "mixed":
        nan, inf = f32(np.nan), f32(np.inf)
        if W * H == 1:
            poison(x, 0, 0, f32(-0.3), 1)  # the one pixel there is: a negative channel
        else:
            poison(x, 0, 0, nan, 0), poison(r, H - 1, W - 1, inf), poison(r, 0, W - 1, f32(-2.0)), poison(x, H - 1, 0, -inf, 2)
        if W > 4 and H > 4:
            poison(x, 2, 3, f32(-0.05), 2), poison(r, 3, 2, nan, 1), poison(x, 4, 4, inf), poison(r, 4, 4, -inf)  # (both at one pixel)
        # either side of a tile's edge, and at the reach of the window from it
        for d in (-1, 0, HALO - 1, HALO, -HALO, -HALO - 1):
            poison(x, 7, TW + d, nan), poison(r, TH + d, 9, inf, 0), poison(x, TH + d, TW + d, f32(-1.5)), poison(r, 2 * TH + d, TW + 3, nan, 2)
        poison(x, 2 * TH + 1, 2 * TW - 1, -inf, 1), poison(r, 2 * TH - 1, 2 * TW, f32(-0.5), 0)
        for _ in range(W * H // 150):
            poison(x if rng.integers(2) else r, int(rng.integers(H)), int(rng.integers(W)), (nan, inf, -inf, f32(-0.7))[int(rng.integers(4))], int(rng.integers(3)))
    if kind == "overflow":
        x[H // 2, W // 2, 1] = f32(1e25)
    out = SimpleNamespace(W=W, H=H, x=x, r=r, bad=bad)
    for a in (x, r, bad):
        a.flags.writeable = False
    return out
