"""TEST-ONLY: numpy restatement of the per-subtree signatures and of the library's choice (include/evogp_hip.h
evogp_hip_sr_subtree_signatures / evogp_hip_subtree_library_select, csrc/sr_subtree_sig.hip).

    signatures   every subtree of a well-formed tree extracted into a row of its own (subtree_ref.extract_subtrees), the C oracle's
                 predictions of those rows, semantic_ref.signature of each; 0 on tails and malformed trees.  No tape, no operand table
    select       a dict loop over the contract: eligible nodes by signature, the (size, flat index)-smallest member of each class, the
                 classes by (count descending, representative ascending)
    extract      the verbatim-copy rule of Forest.subtree_library"""
import numpy as np

import semantic_ref as S
from subtree_ref import extract_subtrees, live_len

MAX_LIB = 1024


def forest_signatures(oracle, value, type_, size, X):
    """uint64 (pop, L)"""
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    X = np.ascontiguousarray(X, np.float32)
    pop, L = value.shape
    sig = np.zeros((pop, L), np.uint64)
    formed = S.formed_mask(type_, size)
    trees = np.flatnonzero(formed)
    if not len(trees):
        return sig
    clamped = size.copy()
    clamped[:, 0] = [live_len(size[t], L) for t in range(pop)]   # (the root's word may overstate a well-formed tree only by clamping)
    parts = [extract_subtrees(value, type_, clamped, int(t)) for t in trees]
    rows = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    with np.errstate(all="ignore"):
        P = oracle.batch_evaluate(*rows, X, 1)[:, :, 0]
        words = S.signature(P, np.ones(len(P), bool))
    at = 0
    for t, p in zip(trees, parts):
        n = p[0].shape[0]
        sig[t, :n] = words[at:at + n]
        at += n
    return sig


def select(sig, size, min_size, max_size, k):
    """``(member int32 (k,), count int32 (k,), n_classes int)``"""
    assert 1 <= k <= MAX_LIB and 1 <= min_size <= max_size
    sig, size = np.asarray(sig).reshape(-1).view(np.uint64), np.asarray(size).reshape(-1)
    classes = {}
    for f in range(sig.shape[0]):
        if sig[f] != 0 and min_size <= int(size[f]) <= max_size:
            c = classes.setdefault(int(sig[f]), [0, None])
            c[0] += 1
            if c[1] is None or (int(size[f]), f) < c[1]:
                c[1] = (int(size[f]), f)
    order = sorted(((-n, rep[1]) for n, rep in classes.values()))
    member, count = np.full(k, -1, np.int32), np.zeros(k, np.int32)
    for j, (neg, f) in enumerate(order[:k]):
        member[j], count[j] = f, -neg
    return member, count, len(order)


def extract(value, type_, size, member):
    """the rows of the chosen subtrees: nodes [node, node + size) from position 0, zero tails -> ``((value, type, size), tree, node)``"""
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    L = value.shape[1]
    member = np.asarray(member, np.int64)
    member = member[member >= 0]
    tree, node = member // L, member % L
    out = tuple(np.zeros((len(member), L), a.dtype) for a in (value, type_, size))
    for j, (t, i) in enumerate(zip(tree, node)):
        n = int(size[t, i])
        for o, a in zip(out, (value, type_, size)):
            o[j, :n] = a[t, i:i + n]
    return out, tree, node
