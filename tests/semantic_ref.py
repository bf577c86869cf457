"""TEST-ONLY: numpy restatement of semantic duplicate classes (include/evogp_hip.h evogp_hip_sr_semantic_hash /
evogp_hip_sr_semantic_classes, csrc/sr_semantic.hip) over a ``(pop, D)`` float32 prediction matrix ``P`` and a well-formed mask.

    key      the bit pattern of a prediction with -0.0 -> +0.0 and every NaN -> 0x7FC00000
    equal    two trees are equal when both are well formed and their keys agree on every row; a malformed row equals only itself
    sig[t]   mix64((sum_{d<D} mix64(key[t][d] ^ ((d + 1) * GOLD))) + D) mod 2^64, 0 for a malformed row
    class_id[t]   the smallest index of a tree equal to tree t -- by comparing the key rows themselves, no hashing
The predictions are the caller's: the CPU oracle's on the CPU, ``Forest.batch_forward``'s on the GPU."""
import numpy as np

from dedup_ref import GOLD, mix64
from subtree_ref import live_len, well_formed

CANONICAL_NAN = np.uint32(0x7FC00000)


def formed_mask(type_, size):
    """bool (pop,): the rows the SR kernels' structural pre-pass accepts (length clamped to [0, gp_len], single-output mode)"""
    L = type_.shape[1]
    return np.array([well_formed(type_[t], live_len(size[t], L)) for t in range(type_.shape[0])], bool)


def oracle_predictions(oracle, value, type_, size, X):
    """``(P (pop, D) float32, formed)`` from the CPU oracle's batch evaluation; a malformed row is not evaluated (its P row is NaN)"""
    formed = formed_mask(type_, size)
    v, t, s = value.copy(), type_.copy(), size.copy()
    v[~formed, 0], t[~formed, 0], s[~formed, 0] = 0.0, 1, 1   # (a CONST 0 in its place)
    P = oracle.batch_evaluate(v, t, s, np.ascontiguousarray(X, np.float32), 1)[:, :, 0].copy()
    P[~formed] = np.nan
    return P, formed


def keys(P):
    """uint32 (pop, D)"""
    u = np.ascontiguousarray(P, np.float32).view(np.uint32).copy()
    mag = u & np.uint32(0x7FFFFFFF)
    u[mag == 0] = 0
    u[mag > np.uint32(0x7F800000)] = CANONICAL_NAN
    return u


def signature(P, formed):
    """uint64 (pop,)"""
    k = keys(P).astype(np.uint64)
    D = k.shape[1]
    with np.errstate(over="ignore"):
        terms = mix64(k ^ (np.arange(1, D + 1, dtype=np.uint64) * GOLD)[None, :])
        sig = mix64(terms.sum(axis=1, dtype=np.uint64) + np.uint64(D))
    return np.where(np.asarray(formed, bool), sig, np.uint64(0))


def class_id(P, formed):
    """int32 (pop,): first-index classes by exact comparison of the key rows"""
    k = np.ascontiguousarray(keys(P))
    seen = {}
    out = np.empty(k.shape[0], np.int32)
    for t in range(k.shape[0]):
        out[t] = seen.setdefault(k[t].tobytes(), t) if formed[t] else t
    return out


def smallest_representative(first_class, nodes):
    """int32 (pop,): per class of ``first_class`` the member with the fewest ``nodes``, ties to the smallest index"""
    first_class, nodes = np.asarray(first_class), np.asarray(nodes)
    best = {}
    for t in range(first_class.shape[0]):
        c = int(first_class[t])
        if c not in best or (int(nodes[t]), t) < (int(nodes[best[c]]), best[c]):
            best[c] = t
    return np.array([best[int(c)] for c in first_class], np.int32)
