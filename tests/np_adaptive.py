"""Adaptive sampling restated in numpy (include/rbrt_hip.h "Adaptive sampling"), written from the rule
and independently of the C++: per-sample radiance in, tile counts, tile errors, rounds and the image out.

Everything is float32, one operation at a time (numpy never fuses), in the rule's order. Tile arrays are indexed by image
tile (tile row, tile column); `per_rank` puts them into a rank's ascending tile-number order.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from rbrt_amd import tiles

f32 = np.float32
TILE = 8


class Result(NamedTuple):
    counts: np.ndarray      # uint32 [tiles_y, tiles_x]: n_t
    errors: np.ndarray      # float32 [tiles_y, tiles_x]: the last E computed for the tile
    rounds: int
    image: np.ndarray       # float32 [H, W, 3]
    rgb8: np.ndarray        # uint8 [H, W, 3]
    samples: int
    samples_fixed: int
    round_errors: list      # per round: float32 [tiles_y, tiles_x], NaN-free only where the tile was active (else the old value)
    round_active: list      # per round: tiles active at its start


def tile_grid(H, W):
    return (H + TILE - 1) // TILE, (W + TILE - 1) // TILE


def _to_tiles(a, fill):
    """[H, W] -> [tiles_y, tiles_x, 64] with p = (y % 8) * 8 + (x % 8); slots beyond the image hold `fill`."""
    H, W = a.shape
    ty, tx = tile_grid(H, W)
    pad = np.full((ty * TILE, tx * TILE), fill, a.dtype)
    pad[:H, :W] = a
    return pad.reshape(ty, TILE, tx, TILE).transpose(0, 2, 1, 3).reshape(ty, tx, 64)


def tile_error(S, S_even, n):
    """E of every tile after n samples: S, S_even float32 [H, W, 3] -> float32 [tiles_y, tiles_x]."""
    H, W, _ = S.shape
    h = (n + 1) // 2
    inv_n, inv_h = f32(1.0) / f32(n), f32(1.0) / f32(h)
    with np.errstate(all="ignore"):
        I, A = S * inv_n, S_even * inv_h
        d = np.abs(I - A)
        e = (d[..., 0] + d[..., 1]) + d[..., 2]
        q = e / (np.sqrt((I[..., 0] + I[..., 1]) + I[..., 2]) + f32(0.0001))
        assert q.dtype == f32
        v = _to_tiles(q, f32(0.0))
        lane = np.arange(64)
        for dd in (1, 2, 4, 8, 16, 32):
            v = v + v[..., lane ^ dd]
        assert (v.view(np.uint32) == v[..., :1].view(np.uint32)).all()  # every lane ends with the same bits
        inside = _to_tiles(np.ones((H, W), f32), f32(0.0)).sum(-1)      # (small integers: exact)
        return (v[..., 0] / inside.astype(f32)).astype(f32)


def quantise(c):
    """(sqrt(c) * 256) as u8: the cast saturates and maps NaN to 0."""
    with np.errstate(all="ignore"):
        v = np.sqrt(c.astype(f32)) * f32(256.0)
        out = np.where(v >= f32(255.0), f32(255.0), v)
        out = np.where(np.isnan(v) | (v <= 0), f32(0.0), out)
        return out.astype(np.uint8)


def adaptive(samples, threshold, min_samples, step) -> Result:
    """samples: float32 [N, H, W, 3], sample s of every pixel. N is the limit."""
    samples = np.asarray(samples, f32)
    N, H, W, _ = samples.shape
    assert N >= 1 and min_samples >= 2 and step >= 1 and threshold >= 0 and np.isfinite(threshold)
    threshold = f32(threshold)
    ty, tx = tile_grid(H, W)
    py, px = np.meshgrid(np.arange(H) // TILE, np.arange(W) // TILE, indexing="ij")  # every pixel's tile
    S, S_even = np.zeros((H, W, 3), f32), np.zeros((H, W, 3), f32)
    active = np.ones((ty, tx), bool)
    counts, errors = np.zeros((ty, tx), np.uint32), np.zeros((ty, tx), f32)
    rounds, n_prev, n_k = 0, 0, min(min_samples, N)
    round_errors, round_active = [], []
    with np.errstate(all="ignore"):
        while active.any():
            round_active.append(int(active.sum()))
            m = active[py, px]
            for s in range(n_prev, n_k):
                S[m] = S[m] + samples[s][m]
                if s % 2 == 0:
                    S_even[m] = S_even[m] + samples[s][m]
            E = tile_error(S, S_even, n_k)
            counts[active] = n_k
            errors[active] = E[active]
            round_errors.append(errors.copy())
            active = active & (n_k < N) & ~(E < threshold)
            rounds += 1
            n_prev, n_k = n_k, min(n_k + step, N)
        inv = f32(1.0) / counts.astype(f32)
        image = (S * inv[py, px][..., None]).astype(f32)
    inside = _to_tiles(np.ones((H, W), np.int64), 0).sum(-1)
    return Result(counts, errors, rounds, image, quantise(image), int((inside * counts).sum()), int(inside.sum()) * N,
                  round_errors, round_active)


def per_rank(tile_array, rank=0, world=1):
    """[tiles_y, tiles_x] -> the entries of the rank's tiles in ascending tile number (rbrt_hip_tile_xy's dealing)."""
    ty, tx = tile_array.shape
    yy, xx = np.meshgrid(np.arange(ty), np.arange(tx), indexing="ij")
    num = tiles.tile_number(yy, xx, tx)
    flat = np.empty(ty * tx, tile_array.dtype)
    flat[num.ravel()] = tile_array.ravel()
    return flat[rank::world]


def sample_map(counts, H, W, N):
    """The per-pixel count scaled to 0-255 (the CLI's --sample-map): uint8 [H, W], count * 255 // N."""
    py, px = np.meshgrid(np.arange(H) // TILE, np.arange(W) // TILE, indexing="ij")
    return (counts[py, px].astype(np.uint64) * 255 // N).astype(np.uint8)
