"""The tile lists of an adaptive round restated in numpy (rbrt_amd/csrc/kernels.hip adaptive_lists_kernel, DESIGN.md
section 9): which local tiles a lane of the one wave owns, the class of every tile in a round, and the two lists.

A rank's tiles are numbered 0 .. n - 1 in ascending tile number (np_adaptive.per_rank puts a tile array into that order).
Lane t of 64 owns the run [t * per, (t + 1) * per) cut off at n, per = ceil(n / 64): the lanes behind the last run own
nothing (lo = hi = n). A tile's class in a round: WORK (active, some ray may hit something), SKY (active, bit 31 of its
culling word: it sees only the background) or INACTIVE (it stopped in an earlier round; on neither list).
"""
from __future__ import annotations

import numpy as np

LANES = 64
WORK, SKY, INACTIVE = 0, 1, 2


def schedule(n_max, min_samples, step):
    """The counts n_k at the end of round k = 0, 1, ...: min(min_samples, N), then `step` more each round up to N."""
    out = [min(min_samples, n_max)]
    while out[-1] < n_max:
        out.append(min(out[-1] + step, n_max))
    return out


def runs(n):
    """[(lo, hi)] * 64: lane t's run of local tiles."""
    per = (n + LANES - 1) // LANES
    return [(min(t * per, n), min(min(t * per, n) + per, n)) for t in range(LANES)]


def classes(counts, cull, n_k):
    """The class of every local tile in the round that ends at n_k samples. counts: the tiles' FINAL counts, cull: their
    culling words (None: no tile pass, no background list), both in local order. A tile is active in that round if and
    only if its final count is at least n_k."""
    counts = np.asarray(counts)
    sky = np.zeros(counts.shape, bool) if cull is None else (np.asarray(cull, np.uint32) >> 31).astype(bool)
    return np.where(counts >= n_k, np.where(sky, SKY, WORK), INACTIVE).astype(np.uint8)


def lists(cls):
    """(work list, background list) of a round: the local tiles of either class, ascending."""
    cls = np.asarray(cls)
    return np.flatnonzero(cls == WORK).astype(np.uint32), np.flatnonzero(cls == SKY).astype(np.uint32)


def lists_by_lane(cls):
    """The same two lists made the way the wave makes them: every lane counts its run, an exclusive scan over the lanes
    gives each run its place in either list, every lane writes its own tiles. Returns (work, sky, n_work, n_sky), the lists
    in one array of 2 n words each with the second list at n -- the words no lane wrote are 0xFFFFFFFF."""
    cls = np.asarray(cls)
    n = len(cls)
    mine = np.array([[int((cls[lo:hi] == c).sum()) for c in (WORK, SKY)] for lo, hi in runs(n)], np.int64)
    before = np.cumsum(mine, axis=0) - mine
    words = np.full(2 * n, 0xFFFFFFFF, np.uint32)
    for t, (lo, hi) in enumerate(runs(n)):
        r = [int(before[t, 0]), int(before[t, 1])]
        for tl in range(lo, hi):
            if cls[tl] == WORK:
                words[r[0]] = tl
                r[0] += 1
            elif cls[tl] == SKY:
                words[n + r[1]] = tl
                r[1] += 1
    n_work, n_sky = int(mine[:, 0].sum()), int(mine[:, 1].sum())
    return words[:n_work], words[n:n + n_sky], n_work, n_sky


def run_class_sets(cls):
    """Per lane: the set of classes in its run (empty for a lane that owns nothing)."""
    cls = np.asarray(cls)
    return [set(int(c) for c in cls[lo:hi]) for lo, hi in runs(len(cls))]
