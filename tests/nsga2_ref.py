"""numpy restatement of the Pareto ranking and the NSGA-II tournament (include/evogp_hip.h evogp_hip_pareto_rank and
evogp_hip_nsga2_select, csrc/nsga2.hip, evogp_amd/algorithm/selection.py NSGA2Selection).

``rank`` computes the fronts by the dynamic programme over the complexity buckets (one dependent step per distinct cx value) and
everything else with sorts; ``rank_bruteforce`` is the definition itself: the O(n^2) domination matrix, fronts peeled one at a time,
the crowding distance point by point in explicit np.float32 scalar operations, the order by a Python sort.  Both return
``(front int32, crowding float32, order int32)``."""
import numpy as np

UNRANKED = 0x7FFFFFFF
CX_MAX = 65535
ROW_CONTENDER = 2**22          # + k: contender k of tournament i


def keys(err):
    """key(e): NaN -> +inf, -0 -> +0"""
    k = np.array(err, dtype=np.float32, copy=True).reshape(-1)
    k[np.isnan(k)] = np.inf
    k[k == 0] = 0.0
    return k


def ranked_mask(key, cx, cx_bound):
    assert 0 <= cx_bound <= CX_MAX, "cx_bound must be in [0, 65535]"
    return np.isfinite(key) & (cx >= 0) & (cx <= cx_bound)


def _inputs(err, cx, cx_bound):
    key = keys(err)
    cx = np.asarray(cx).reshape(-1).astype(np.int64)
    assert key.shape == cx.shape and len(key) > 0
    return key, cx, ranked_mask(key, cx, cx_bound)


def _order(front, crowding):
    """front ascending, crowding descending, tree index ascending"""
    idx = np.arange(len(front))
    with np.errstate(invalid="ignore"):
        return np.lexsort((idx, -crowding.astype(np.float64), front)).astype(np.int32)


# ---- the bucket programme --------------------------------------------------------------------------------------------------------
def fronts(key, cx, ranked):
    """front of every tree (int64; UNRANKED for the unranked ones)"""
    front = np.full(len(key), UNRANKED, dtype=np.int64)
    idx = np.flatnonzero(ranked)
    if not len(idx):
        return front
    idx = idx[np.lexsort((key[idx], cx[idx]))]                     # bucket by bucket, ascending key inside a bucket
    c = cx[idx]
    kpos = np.unique(key[idx], return_inverse=True)[1].reshape(-1)     # dense rank of the key
    A = np.full(int(kpos.max()) + 1, -1, dtype=np.int64)             # A[j]: largest front so far among processed trees of key rank <= j
    starts = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    ends = np.concatenate([starts[1:], [len(c)]])
    for s, e in zip(starts, ends):                                   # one dependent step per distinct cx value
        groups, inv = np.unique(kpos[s:e], return_inverse=True)       # the groups of equal key, ascending
        i = np.arange(len(groups))
        fr = i + np.maximum.accumulate(A[groups] + 1 - i)
        front[idx[s:e]] = fr[inv.reshape(-1)]
        A[groups] = np.maximum(A[groups], fr)
        A[groups[0]:] = np.maximum.accumulate(A[groups[0]:])          # restore the running maximum
    return front


def crowding_distance(key, cx, front, ranked):
    """float32: Deb's distance on the representatives of the distinct points, 0 on clones and unranked trees"""
    crowd = np.zeros(len(key), dtype=np.float32)
    idx = np.flatnonzero(ranked)
    if not len(idx):
        return crowd
    idx = idx[np.lexsort((idx, cx[idx], front[idx]))]              # by front, cx, tree: equal (front, cx) is one point
    f, c = front[idx], cx[idx]
    head = np.concatenate([[True], (f[1:] != f[:-1]) | (c[1:] != c[:-1])])
    rep = idx[head]                                                  # the points, front by front in ascending cx
    pf, pc, pk = front[rep], cx[rep].astype(np.float32), key[rep]
    n = len(rep)
    first = np.concatenate([[True], pf[1:] != pf[:-1]])
    last = np.concatenate([pf[1:] != pf[:-1], [True]])
    a = np.maximum.accumulate(np.where(first, np.arange(n), 0))                     # first point of the point's front
    b = np.minimum.accumulate(np.where(last, np.arange(n), n)[::-1])[::-1]           # last point of it
    prev, nxt = np.maximum(np.arange(n) - 1, 0), np.minimum(np.arange(n) + 1, n - 1)
    with np.errstate(all="ignore"):
        dc = (pc[nxt] - pc[prev]) / (pc[b] - pc[a])                                  # float32 arrays: one IEEE operation each
        dk = (pk[prev] - pk[nxt]) / (pk[a] - pk[b])
        d = dc + dk
    assert d.dtype == np.float32
    d[np.isnan(d)] = np.inf
    d[first | last] = np.inf
    crowd[rep] = d
    return crowd


def rank(err, cx, cx_bound=CX_MAX):
    key, cx, ranked = _inputs(err, cx, cx_bound)
    front = fronts(key, cx, ranked)
    crowd = crowding_distance(key, cx, front, ranked)
    return front.astype(np.int32), crowd, _order(front, crowd)


# ---- the definition --------------------------------------------------------------------------------------------------------------
def domination_matrix(key, cx, ranked):
    """D[q][p]: ranked q dominates ranked p"""
    le = (key[:, None] <= key[None, :]) & (cx[:, None] <= cx[None, :])
    lt = (key[:, None] < key[None, :]) | (cx[:, None] < cx[None, :])
    return le & lt & ranked[:, None] & ranked[None, :]


def rank_bruteforce(err, cx, cx_bound=CX_MAX):
    key, cx, ranked = _inputs(err, cx, cx_bound)
    n = len(key)
    D = domination_matrix(key, cx, ranked)
    front = np.full(n, UNRANKED, dtype=np.int64)
    left = D.sum(axis=0)                                             # dominators not yet peeled
    remaining = ranked.copy()
    level = 0
    while remaining.any():
        cur = remaining & (left == 0)
        assert cur.any()
        front[cur] = level
        remaining &= ~cur
        left = left - D[cur].sum(axis=0)
        level += 1
    crowd = np.zeros(n, dtype=np.float32)
    inf = np.float32(np.inf)
    for f in range(level):
        members = np.flatnonzero(front == f)
        points = {}
        for t in members:                                            # ascending tree index: the first of a point is its representative
            points.setdefault((key[t].tobytes(), int(cx[t])), int(t))
        reps = sorted(points.values(), key=lambda t: int(cx[t]))
        assert len(set(int(cx[t]) for t in reps)) == len(reps)
        first, last = reps[0], reps[-1]
        for j, t in enumerate(reps):
            if j == 0 or j == len(reps) - 1:
                crowd[t] = inf
                continue
            lo, hi = reps[j - 1], reps[j + 1]
            with np.errstate(all="ignore"):
                dc = (np.float32(cx[hi]) - np.float32(cx[lo])) / (np.float32(cx[last]) - np.float32(cx[first]))
                dk = (np.float32(key[lo]) - np.float32(key[hi])) / (np.float32(key[first]) - np.float32(key[last]))
                d = np.float32(dc + dk)
            crowd[t] = inf if np.isnan(d) else d
    order = sorted(range(n), key=lambda t: (int(front[t]), -float(crowd[t]), t))
    return front.astype(np.int32), crowd, np.array(order, dtype=np.int32)


# ---- the tournaments -------------------------------------------------------------------------------------------------------------
def select(order, pool, n, t_size, seed, generation):
    """winners[i] = order[min over k < t_size of (word(seed, generation, 2^22 + k, i) mod pool)] -- int32[n]"""
    from evogp_amd.parallel import random_words

    order = np.asarray(order)
    assert 1 <= pool <= len(order) and 1 <= t_size <= 2**20 and n >= 0
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    words = random_words(seed, generation, t_size, 0, n, "cpu", first_row=ROW_CONTENDER).numpy().astype(np.int64)     # (t_size, n)
    return order[(words % pool).min(axis=0)].astype(np.int32)
