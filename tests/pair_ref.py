"""TEST-ONLY: numpy restatement of the pairwise semantic moments (csrc/sr_pair.hip, include/evogp_hip.h evogp_hip_sr_pair_moments), of the
four mate criteria and of the arg-min rule (evogp_amd/algorithm/semantic_mate.py), over a (pop, D) float32 prediction matrix and a
well-formed mask.  Nothing here shares code with the kernels.

    r_t[d] = (double)p_t[d] - (double)y[d]                      (exactly: no rounding in the restatement)
    own[e]           = sum_d r_a^2                a = first[e]
    moments[e, m, 0] = sum_d r_b^2                b = candidates[e, m]
    moments[e, m, 1] = sum_d r_a r_b
    moments[e, m, 2] = sum_d (p_a - p_b)^2

A tree is unusable when it is malformed, when a prediction is not finite, or when its index lies outside its forest; an unusable first tree
makes own[e] and moments[e] NaN, an unusable candidate its three words.  ``exact=True`` sums in fractions.Fraction and rounds once at the
end (the planted cases, small fuzz); otherwise the sums run in np.longdouble."""
from fractions import Fraction

import numpy as np

CRITERIA = ("midpoint", "blend", "angle", "competent")


def usable(P, formed):
    """bool (pop,): well formed and finite on every row"""
    return np.asarray(formed, bool) & np.isfinite(np.asarray(P, np.float32)).all(axis=1)


def _sum(terms, exact):
    if exact:
        return float(sum(terms, Fraction(0)))
    return np.sum(terms, dtype=np.longdouble)


def _resid(p, y, exact):
    if exact:
        return [Fraction(float(a)) - Fraction(float(b)) for a, b in zip(p, y)]
    return p.astype(np.longdouble) - y.astype(np.longdouble)


def _mul(a, b, exact):
    return [x * z for x, z in zip(a, b)] if exact else a * b


def _abs(a, exact):
    return [abs(x) for x in a] if exact else np.abs(a)


def pair_moments(PA, usable_a, PB, usable_b, y, first, cand, exact=False):
    """``(own (E,), moments (E, M, 3), own_mag (E,), mag (E, M, 3))`` float64; ``mag`` holds the sum of the ABSOLUTE terms of every word
    (the scale of its rounding error; it differs from the word for Sab only).  ``y`` None: every label is 0."""
    PA, PB = np.asarray(PA, np.float32), np.asarray(PB, np.float32)
    first, cand = np.asarray(first, np.int64), np.asarray(cand, np.int64)
    E, M = cand.shape
    assert first.shape == (E,) and PA.shape[1] == PB.shape[1]
    D = PA.shape[1]
    y = np.zeros(D, np.float32) if y is None else np.asarray(y, np.float32).reshape(D)
    own, mom = np.full(E, np.nan), np.full((E, M, 3), np.nan)
    own_mag, mag = np.full(E, np.nan), np.full((E, M, 3), np.nan)
    for e in range(E):
        a = int(first[e])
        if not (0 <= a < PA.shape[0]) or not usable_a[a]:
            continue
        ra = _resid(PA[a], y, exact)
        own[e] = own_mag[e] = _sum(_mul(ra, ra, exact), exact)
        for m in range(M):
            b = int(cand[e, m])
            if not (0 <= b < PB.shape[0]) or not usable_b[b]:
                continue
            rb = _resid(PB[b], y, exact)
            dd = _resid(PA[a], PB[b], exact)
            ab = _mul(ra, rb, exact)
            mom[e, m] = (_sum(_mul(rb, rb, exact), exact), _sum(ab, exact), _sum(_mul(dd, dd, exact), exact))
            mag[e, m] = (mom[e, m, 0], _sum(_abs(ab, exact), exact), mom[e, m, 2])
    return own, mom, own_mag, mag


def bound(D, mag):
    """what a float64 evaluation may differ from the exact word by: every term carries at most three roundings (the two residuals, the
    fused multiply-add) and the sum D - 1 more, so |got - want| <= (D + 8) 2^-53 sum_d |term_d|"""
    return (D + 8) * 2.0 ** -53 * np.asarray(mag, np.float64)


# ---- the criteria and the arg-min rule ---------------------------------------------------------------------------------------------------
def scores(criterion, own, mom):
    """float64 (E, M): lower is better; an unusable pair (NaN) scores +inf"""
    saa = np.asarray(own, np.float64)[:, None]
    sbb, sab, sdd = (np.asarray(mom, np.float64)[..., k] for k in range(3))
    with np.errstate(all="ignore"):
        if criterion == "midpoint":
            s = (saa + 2.0 * sab + sbb) / 4.0
        elif criterion == "blend":
            alpha = np.where(sdd == 0, 0.0, np.clip((sbb - sab) / np.where(sdd == 0, 1.0, sdd), 0.0, 1.0))
            s = alpha * alpha * saa + 2.0 * alpha * (1.0 - alpha) * sab + (1.0 - alpha) * (1.0 - alpha) * sbb
        elif criterion == "angle":
            prod = saa * sbb
            s = np.where(prod == 0, 1.0, sab / np.sqrt(np.where(prod == 0, 1.0, prod)))
        elif criterion == "competent":
            s = np.sqrt(sbb / np.where(sdd == 0, 1.0, sdd)) * (1.0 + np.abs(np.sqrt(saa) - np.sqrt(sbb)))
            s = np.where(sdd == 0, np.inf, s)
        else:
            raise ValueError(criterion)
    nan = np.isnan(saa + sbb + sab + sdd)
    return np.where(nan | np.isnan(s), np.inf, s)


def choose(score, cand):
    """``(right (E,), best (E,), slot (E,))``: the lowest score, ties to the lowest slot, slot 0 when every slot is +inf"""
    score, cand = np.asarray(score, np.float64), np.asarray(cand)
    slot = np.zeros(len(score), np.int64)
    for e in range(len(score)):
        for m in range(1, score.shape[1]):
            if score[e, m] < score[e, slot[e]]:
                slot[e] = m
    rows = np.arange(len(score))
    return cand[rows, slot], score[rows, slot], slot
