"""The helper that restates an adaptive round's tile lists (np_lists.py), on hand-made patterns and without a GPU."""
import numpy as np
import pytest

import np_lists as L

W, S, I = L.WORK, L.SKY, L.INACTIVE


def test_schedule():
    assert L.schedule(12, 4, 4) == [4, 8, 12]
    assert L.schedule(11, 4, 3) == [4, 7, 10, 11]
    assert L.schedule(7, 16, 16) == [7]
    assert L.schedule(5, 4, 1) == [4, 5]


@pytest.mark.parametrize("n,per,owners,last", [(1, 1, 1, (0, 1)), (15, 1, 15, (14, 15)), (64, 1, 64, (63, 64)), (65, 2, 33, (64, 65)),
                                               (119, 2, 60, (118, 119)), (128, 2, 64, (126, 128)), (129, 3, 43, (126, 129)),
                                               (153, 3, 51, (150, 153)), (357, 6, 60, (354, 357))])
def test_runs_partition_the_tiles(n, per, owners, last):
    r = L.runs(n)
    assert len(r) == 64 and r[0] == (0, min(per, n))
    own = [(lo, hi) for lo, hi in r if hi > lo]
    assert len(own) == owners and own[-1] == last
    assert all(hi - lo == per for lo, hi in own[:-1]) and 1 <= last[1] - last[0] <= per
    assert all((lo, hi) == (n, n) for lo, hi in r[owners:])  # the lanes behind the last run: clamped to n
    assert [t for lo, hi in r for t in range(lo, hi)] == list(range(n))  # every tile once, in order


def test_runs_by_hand():
    assert L.runs(65)[:2] == [(0, 2), (2, 4)] and L.runs(65)[32] == (64, 65) and L.runs(65)[33] == (65, 65)
    assert L.runs(129)[42] == (126, 129) and L.runs(129)[43] == (129, 129) and L.runs(129)[63] == (129, 129)
    assert L.runs(64)[63] == (63, 64)


def test_classes_by_hand():
    counts = np.array([4, 8, 12, 12, 4, 8])
    cull = np.array([0, 0x80000000, 0x80000001, 0x7FFFFFFF, 0x80000000, 3], np.uint32)
    assert L.classes(counts, cull, 4).tolist() == [W, S, S, W, S, W]
    assert L.classes(counts, cull, 8).tolist() == [I, S, S, W, I, W]
    assert L.classes(counts, cull, 12).tolist() == [I, I, S, W, I, I]
    assert L.classes(counts, None, 8).tolist() == [I, W, W, W, I, W]  # no tile pass: no background list


def pattern(n, kind):
    if kind == "all_work":
        return np.full(n, W, np.uint8)
    if kind == "all_inactive":
        return np.full(n, I, np.uint8)
    if kind == "cycle":   # work, background, inactive, work, ...: every run of three holds all three classes
        return (np.arange(n) % 3).astype(np.uint8)
    if kind == "last_only":
        c = np.full(n, I, np.uint8)
        c[-1] = S
        return c
    if kind == "halves":  # background first, then work: the lists are filled by different lanes
        c = np.full(n, W, np.uint8)
        c[:n // 2] = S
        return c
    return np.random.default_rng(n).integers(0, 3, n).astype(np.uint8)


@pytest.mark.parametrize("kind", ["all_work", "all_inactive", "cycle", "last_only", "halves", "random"])
@pytest.mark.parametrize("n", [1, 15, 63, 64, 65, 128, 129, 153, 357])
def test_the_lanes_make_the_ascending_lists(n, kind):
    cls = pattern(n, kind)
    work, sky = L.lists(cls)
    assert work.tolist() == [t for t in range(n) if cls[t] == W] and sky.tolist() == [t for t in range(n) if cls[t] == S]
    lw, ls, n_work, n_sky = L.lists_by_lane(cls)
    assert (n_work, n_sky) == (len(work), len(sky))
    assert np.array_equal(lw, work) and np.array_equal(ls, sky)


def test_run_class_sets_by_hand():
    n = 129  # per = 3
    sets = L.run_class_sets(pattern(n, "cycle"))
    assert all(s == {W, S, I} for s in sets[:43]) and all(s == set() for s in sets[43:])
    n = 65   # per = 2: the last run has one tile
    cls = np.array([W, I] * 32 + [S], np.uint8)
    sets = L.run_class_sets(cls)
    assert all(s == {W, I} for s in sets[:32]) and sets[32] == {S} and all(s == set() for s in sets[33:])
    assert all(len(s) == 1 for s in L.run_class_sets(pattern(64, "cycle")))  # one tile a lane: no run mixes classes
