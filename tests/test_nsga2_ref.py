"""CPU: the numpy twin of the Pareto ranking (tests/nsga2_ref.py) -- its bucket programme against the O(n^2) definition, word for word,
and the properties a non-dominated sort, a crowding distance and the tournament must have."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nsga2_ref as R  # noqa: E402

POPS = [1, 2, 3, 50, 400, 1500]
SPANS = [1, 2, 19, 65535]


def population(rng, pop, kind, span):
    """err, cx: 30 % NaN, some +-inf, some -0, cx in [0, span)"""
    if kind == "continuous":
        err = rng.exponential(1.0, pop).astype(np.float32)
    else:   # quantised: many ties
        err = (rng.integers(0, 6, pop) * 0.25).astype(np.float32)
    err[rng.random(pop) < 0.30] = np.nan
    err[rng.random(pop) < 0.03] = np.inf
    err[rng.random(pop) < 0.02] = -np.inf
    err[rng.random(pop) < 0.05] = -0.0
    cx = rng.integers(0, span, pop).astype(np.int32)
    return err, cx


def assert_same(got, want, what=""):
    for name, g, w in zip(("front", "crowding", "order"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, f"{what}: {name} {g.dtype}{g.shape} vs {w.dtype}{w.shape}"
        gv, wv = (g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else (g, w)
        bad = np.flatnonzero(gv != wv)
        assert not len(bad), f"{what}: {name} differs at {len(bad)} of {len(g)} trees, e.g. tree {bad[0]}: {g[bad[0]]} vs {w[bad[0]]}"


@pytest.mark.parametrize("pop", POPS)
@pytest.mark.parametrize("span", SPANS)
@pytest.mark.parametrize("kind", ["continuous", "quantised"])
def test_bucket_programme_equals_definition(rng, kind, span, pop):
    err, cx = population(rng, pop, kind, span)
    assert_same(R.rank(err, cx), R.rank_bruteforce(err, cx), f"{kind} pop {pop} span {span}")


def test_all_unranked_all_clones_and_the_bound(rng):
    for pop in (1, 7, 300):
        err = np.full(pop, np.nan, np.float32)
        err[::2] = np.inf
        front, crowd, order = R.rank(err, np.arange(pop, dtype=np.int32) % 5)
        assert (front == R.UNRANKED).all() and (crowd == 0).all() and order.tolist() == list(range(pop))
        assert_same((front, crowd, order), R.rank_bruteforce(err, np.arange(pop, dtype=np.int32) % 5))
        clones = (np.full(pop, 0.5, np.float32), np.full(pop, 9, np.int32))
        front, crowd, order = R.rank(*clones)
        assert (front == 0).all() and np.isinf(crowd[0]) and (crowd[1:] == 0).all() and order.tolist() == list(range(pop))
        assert_same((front, crowd, order), R.rank_bruteforce(*clones))
    # a tree outside [0, cx_bound] is unranked, whatever its error
    err = np.array([0.1, 0.2, 0.3, 0.4], np.float32)
    cx = np.array([5, -1, 11, 10], np.int32)
    for fn in (R.rank, R.rank_bruteforce):
        front, crowd, order = fn(err, cx, 10)
        assert front.tolist() == [0, R.UNRANKED, R.UNRANKED, 1] and order.tolist() == [0, 3, 1, 2]
    with pytest.raises(AssertionError):
        R.rank(err, cx, 65536)
    # -0 and +0 are one key; NaN and +-inf are unranked
    err = np.array([-0.0, 0.0, np.nan, -np.inf, np.inf, 1.0], np.float32)
    front, crowd, order = R.rank(err, np.array([3, 3, 0, 0, 0, 1], np.int32))
    assert front.tolist() == [0, 0] + [R.UNRANKED] * 3 + [0]
    assert np.isinf(crowd[0]) and crowd[1] == 0 and np.isinf(crowd[5]) and order.tolist() == [0, 5, 1, 2, 3, 4]


def test_hand_checked_example():
    #         tree  0     1     2     3     4     5     6
    err = np.array([4.0, 2.0, 1.5, 3.0, 2.0, 0.5, 2.5], np.float32)
    cx = np.array([1, 2, 4, 2, 3, 8, 3], np.int32)
    front, crowd, order = R.rank(err, cx)
    # front 0: (4,1) (2,2) (1.5,4) (.5,8); front 1: (3,2) [by tree 1], (2,3) [by 1]; front 2: (2.5,3) [by 4]
    assert front.tolist() == [0, 0, 0, 1, 1, 0, 2]
    f32 = np.float32
    d1 = (f32(4) - f32(1)) / (f32(8) - f32(1)) + (f32(4.0) - f32(1.5)) / (f32(4.0) - f32(0.5))
    d2 = (f32(8) - f32(2)) / (f32(8) - f32(1)) + (f32(2.0) - f32(0.5)) / (f32(4.0) - f32(0.5))
    assert crowd.tolist() == [np.inf, d1, d2, np.inf, np.inf, np.inf, np.inf]
    assert order.tolist() == [0, 5, 2, 1, 3, 4, 6]       # d2 > d1
    assert_same((front, crowd, order), R.rank_bruteforce(err, cx))


@pytest.mark.parametrize("pop,kind,span", [(400, "continuous", 19), (400, "quantised", 19), (1500, "quantised", 2), (1500, "continuous", 65535)])
def test_properties(rng, pop, kind, span):
    err, cx = population(rng, pop, kind, span)
    front, crowd, order = R.rank(err, cx)
    key = R.keys(err)
    ranked = R.ranked_mask(key, cx, R.CX_MAX)
    assert ((front == R.UNRANKED) == ~ranked).all()
    D = R.domination_matrix(key, cx.astype(np.int64), ranked)
    same = front[:, None] == front[None, :]
    assert not (D & same).any(), "a tree dominates another tree of its own front"
    below = front[:, None] == front[None, :] - 1                  # [q][p]: q lies one front below p
    has_parent = (D & below).any(axis=0)
    assert has_parent[ranked & (front > 0)].all(), "a tree of front f > 0 that no tree of front f - 1 dominates"
    assert not D[:, front == 0].any()
    assert sorted(order.tolist()) == list(range(pop)), "order is not a permutation"
    # exactly one clone per point carries a distance, the lowest tree index
    bits = key.view(np.uint32).astype(np.int64) << 17 | cx
    for b in np.unique(bits[ranked]):
        members = np.flatnonzero(ranked & (bits == b))
        assert crowd[members[0]] > 0 and (crowd[members[1:]] == 0).all()
    assert (crowd[~ranked] == 0).all() and not np.isnan(crowd).any()
    # the order: fronts ascend, inside a front the distances descend, ties by tree index; the unranked trees come last in index order
    f, c = front[order].astype(np.int64), crowd[order]
    assert (np.diff(f) >= 0).all()
    inside = np.diff(f) == 0
    with np.errstate(invalid="ignore"):
        assert (c[1:][inside] <= c[:-1][inside]).all()
    tie = inside & (c[1:] == c[:-1])
    assert (np.diff(order)[tie] > 0).all()


def test_many_fronts_at_scale(rng):
    """100 000 trees shaped like a fresh population (35 % NaN, geometric sizes capped at 64): thousands of fronts from 64 dependent
    steps, each front an antichain in (key, cx)"""
    pop = 100_000
    err = rng.exponential(1.0, pop).astype(np.float32)
    err[rng.random(pop) < 0.35] = np.nan
    cx = np.minimum(rng.geometric(0.08, pop), 64).astype(np.int32)
    front, crowd, order = R.rank(err, cx, 64)
    ranked = front != R.UNRANKED
    assert front[ranked].max() > 1000
    # inside every front, sorted by cx ascending, the keys of the distinct points descend strictly
    idx = np.flatnonzero(ranked)
    idx = idx[np.lexsort((R.keys(err)[idx], cx[idx], front[idx]))]
    f, c, k = front[idx], cx[idx], R.keys(err)[idx]
    same_front = f[1:] == f[:-1]
    clone = same_front & (c[1:] == c[:-1])
    assert (k[1:][clone] == k[:-1][clone]).all()
    step = same_front & ~clone
    assert (c[1:][step] > c[:-1][step]).all() and (k[1:][step] < k[:-1][step]).all()
    assert sorted(order.tolist()) == list(range(pop))


def test_select(rng):
    from evogp_amd.parallel import random_words

    order = rng.permutation(500).astype(np.int32)
    for t_size, pool, n in [(1, 1, 10), (2, 250, 500), (7, 500, 1501), (2, 500, 0), (1, 500, 64)]:
        got = R.select(order, pool, n, t_size, 99, 3)
        assert got.shape == (n,) and got.dtype == np.int32
        if n == 0:
            continue
        w = random_words(99, 3, t_size, 0, n, "cpu", first_row=2**22).numpy().astype(np.int64)
        want = [order[min(int(w[k][i]) % pool for k in range(t_size))] for i in range(n)]
        assert got.tolist() == want
        pos = np.empty(500, np.int64)
        pos[order] = np.arange(500)
        assert (pos[got] < pool).all()
    assert (R.select(order, 1, 50, 3, 1, 1) == order[0]).all()
    # larger tournaments pick earlier places of the order
    pos = np.empty(500, np.int64)
    pos[order] = np.arange(500)
    assert pos[R.select(order, 500, 4000, 7, 5, 0)].mean() < pos[R.select(order, 500, 4000, 2, 5, 0)].mean() < 250
    assert not np.array_equal(R.select(order, 500, 100, 2, 5, 0), R.select(order, 500, 100, 2, 5, 1))
