"""TEST-ONLY: numpy restatement of the rank statistics (csrc/sr_rank.hip, include/evogp_hip.h evogp_hip_sr_rank_stats / evogp_hip_rank_rows)
on given float32 predictions.  Integers are exact, so the kernel is held to the words without a tolerance; it shares no code with it."""
import numpy as np


def keys(p):
    """the order-preserving uint32 of float32 values, -0.0 taken as +0.0"""
    u = np.ascontiguousarray(p, np.float32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def mid_ranks2(p):
    """doubled mid-ranks of a 1-d float32 vector without NaN: #less + #less-or-equal + 1"""
    k = keys(p)
    s = np.sort(k)
    return (np.searchsorted(s, k, "left") + np.searchsorted(s, k, "right") + 1).astype(np.int64)


def rank_rows(v, seg):
    """(r2 (D,) int64, consts (G, 2) int64 of the ranks, status (G,)) of a float32 vector within the segments seg (G + 1,)"""
    r2, status = np.zeros(len(v), np.int64), np.zeros(len(seg) - 1, np.int64)
    for g, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
        status[g] = np.isnan(v[a:b]).any()
        if not status[g]:
            r2[a:b] = mid_ranks2(v[a:b])
    return r2, consts(r2, seg), status


def words(P, formed, q, seg):
    """(words (pop, G, 2) int64, status (pop,)): P (pop, D) float32 predictions, formed (pop,) bool, q (D,) integer payload"""
    status = (~np.asarray(formed, bool) | np.isnan(P).any(axis=1)).astype(np.uint8)
    w, q = np.zeros((P.shape[0], len(seg) - 1, 2), np.int64), np.asarray(q, np.int64)
    for t in np.flatnonzero(status == 0):
        for g, (a, b) in enumerate(zip(seg[:-1], seg[1:])):
            r2 = mid_ranks2(P[t, a:b])
            w[t, g] = (r2 * q[a:b]).sum(), (r2 * r2).sum()
    return w, status


def consts(q, seg):
    return np.array([[q[a:b].sum(), (q[a:b] ** 2).sum()] for q in [np.asarray(q, np.int64)] for a, b in zip(seg[:-1], seg[1:])], np.int64)


def scores(w, c, seg, metric):
    """(pop, G) float64 segment scores from exact Python integers, NaN where undefined"""
    out = np.full(w.shape[:2], np.nan)
    for t in range(w.shape[0]):
        for g in range(w.shape[1]):
            n, S1, S2, Q, Q2 = int(seg[g + 1] - seg[g]), int(w[t, g, 0]), int(w[t, g, 1]), int(c[g, 0]), int(c[g, 1])
            if S2 == 0:   # the words of an unusable tree: no score
                continue
            if metric == "auc":
                if Q != 0 and Q != n:
                    out[t, g] = np.float64(S1 - Q * (Q + 1)) / np.float64(2 * Q * (n - Q))
            else:
                A, Bp, Bl = n * S1 - n * (n + 1) * Q, n * S2 - (n * (n + 1)) ** 2, n * Q2 - Q * Q
                if Bp != 0 and Bl != 0:
                    out[t, g] = np.float64(A) / np.sqrt(np.float64(Bp) * np.float64(Bl))
    return out


def fused(sc, status):
    """(pop, 3) float64: sum, sum of squares, count of the defined scores, added in ascending segment; NaN for an unusable tree"""
    out = np.zeros((sc.shape[0], 3))
    for g in range(sc.shape[1]):
        ok = ~np.isnan(sc[:, g])
        out[ok, 0] += sc[ok, g]
        out[ok, 1] += sc[ok, g] * sc[ok, g]
        out[ok, 2] += 1
    out[np.asarray(status) != 0] = np.nan
    return out

