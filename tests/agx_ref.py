"""TEST-ONLY: a numpy restatement of the midpoint builds of semantic backpropagation (approximately geometric semantic crossover,
csrc/sr_backprop.hip with MID), built on tests/backprop_ref.py.

``forest_desired_mid(value, type, size, mvalue, mtype, msize, X, pos, mate, dtype)`` -> ``(desired (pop, D) dtype, state (pop, D) uint8,
status (pop,) int32)``.  The recipient is tree t, its mate row ``mate[t]`` of the second forest; with a and b their values on a row (by
tests/subtree_ref.py in ``dtype``) the root target is ``mid = 0.5 * a + 0.5 * b``: two scalings and ONE addition in ``dtype``.  Where mid
is finite the row starts as (mid, REQUIRED) and goes down the path by ``backprop_ref.tree_desired``, unchanged; where it is not (a NaN or
an infinity in either parent, inf - inf) the row is IMPOSSIBLE from the start, at every position, pos = 0 included.  status gains 4: the
mate index is outside the mates or the mate's row is malformed; the codes are decided in the order 1 (malformed recipient), 2 (position),
4 (mate), 3 (blocked).  The match is ``backprop_ref.match``, unchanged."""
import numpy as np

import backprop_ref as BR
from subtree_ref import live_len, node_values, well_formed

BAD_MATE = 4


def midpoint(a, b, dtype):
    with np.errstate(all="ignore"):
        return (dtype(0.5) * np.asarray(a, dtype) + dtype(0.5) * np.asarray(b, dtype)).astype(dtype)


def tree_desired_mid(value, type_, size, mvalue, mtype, msize, X, pos, mate, dtype=np.float32):
    """one recipient row against the forest of mates; mate: the index of its mate"""
    X = np.asarray(X)
    D = X.shape[0]
    nan_row = (np.full(D, np.nan, dtype), np.full(D, BR.IMPOSSIBLE, np.uint8))
    n = live_len(size, len(value))
    if not well_formed(type_, n):
        return (*nan_row, BR.MALFORMED)
    if not 0 <= int(pos) < n:
        return (*nan_row, BR.POSITION)
    m = int(mate)
    if not 0 <= m < len(mvalue) or not well_formed(mtype[m], live_len(msize[m], len(mvalue[m]))):
        return (*nan_row, BAD_MATE)
    with np.errstate(all="ignore"):
        a = node_values(value, type_, size, X, dtype)[0]
        b = node_values(mvalue[m], mtype[m], msize[m], X, dtype)[0]
    mid = midpoint(a, b, dtype)
    d, state, status = BR.tree_desired(value, type_, size, X, mid, pos, dtype)
    if status != BR.OK:
        return (*nan_row, status)
    bad = ~np.isfinite(mid)
    return np.where(bad, dtype(np.nan), d).astype(dtype), np.where(bad, BR.IMPOSSIBLE, state).astype(np.uint8), BR.OK


def forest_desired_mid(value, type_, size, mvalue, mtype, msize, X, pos, mate, dtype=np.float32):
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    mvalue, mtype, msize = np.asarray(mvalue), np.asarray(mtype), np.asarray(msize)
    pop, D = value.shape[0], np.asarray(X).shape[0]
    desired, state, status = np.empty((pop, D), dtype), np.empty((pop, D), np.uint8), np.empty(pop, np.int32)
    for t in range(pop):
        desired[t], state[t], status[t] = tree_desired_mid(value[t], type_[t], size[t], mvalue, mtype, msize, X, pos[t], mate[t], dtype)
    return desired, state, status
