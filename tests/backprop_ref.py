"""TEST-ONLY: a numpy restatement of semantic backpropagation (csrc/sr_backprop.hip): the inversion of a single-output
tree from its root down to one node on the rows of a dataset, and the match of the desired values against a library.

``forest_desired(value, type, size, X, y, pos, dtype)`` -> ``(desired (pop, D) dtype, state (pop, D) uint8, status (pop,) int32)``
    dtype=np.float32 is what the device must reproduce: the forward values by tests/subtree_ref.py in float32 and every rule ONE float32
    operation (logf / expf: the float64 function rounded to float32, which the device meets within its library's ulp bound);
    dtype=np.float64 is the same table in float64.
``match(desired, state, status, lib)`` -> ``(best, dist, const, const_dist, counts)`` in float64: plain sums, a two-pass centred sum.

The rule.  status: 0 ok, 1 malformed, 2 pos outside [0, len), 3 blocked (a function on the path has no rule).  Per row a target t and a
state, (y[d], REQUIRED) at the root; FREE and IMPOSSIBLE are absorbing.  k: the operand the path takes, s: the sibling's value, c: the
child's present value.  Before a rule looks at anything: a NaN t, or a NaN s of a BINARY function, is IMPOSSIBLE; after it: a d that is
not finite is IMPOSSIBLE.  The condition of an IF and the child of an ABS are not siblings: a NaN condition is "not > 0", as the
interpreter decides it, and the ABS rule is d = c < 0 ? -t : t (copysign(t, c) but for a child of -0.0 or NaN, where the sign of the
child says nothing about which of the two solutions is nearer).  On a row where an IF does not take the branch the path enters, the tree
returns the other branch whatever the subtree does: FREE where that branch's value equals t, IMPOSSIBLE where it does not."""
import numpy as np

import sr_grad_ref as R
from subtree_ref import live_len, node_values, well_formed

REQUIRED, FREE, IMPOSSIBLE = 0, 1, 2
OK, MALFORMED, POSITION, BLOCKED = 0, 1, 2, 3
RATIONAL = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV, R.F_NEG, R.F_INV, R.F_MAX, R.F_MIN, R.F_ABS, R.F_IF]     # every rule a rational operation
EXACT32 = RATIONAL + [R.F_SQRT]                                                                            # ... or one correctly rounded one
BINARY_RULES = (R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV, R.F_MAX, R.F_MIN)
UNARY_RULES = (R.F_NEG, R.F_INV, R.F_SQRT, R.F_ABS, R.F_EXP, R.F_LOG)


def arity_of(t):
    t = int(t)
    return 0 if t in (R.T_VAR, R.T_CONST) else 1 if t == R.T_UFUNC else 2 if t == R.T_BFUNC else 3


def children(type_row, n):
    """for every node of a well-formed prefix row its operands' indices in prefix order -- from the node types alone"""
    span = [0] * n
    kids = [None] * n
    for i in reversed(range(n)):
        j, ks = i + 1, []
        for _ in range(arity_of(type_row[i])):
            ks.append(j)
            j += span[j]
        span[i], kids[i] = j - i, ks
    return kids


def path_to(kids, pos):
    """[(node, k)] from the root down: the path enters operand k of node"""
    steps, node = [], 0
    while node != pos:
        for k, c in enumerate(kids[node]):
            nxt = kids[node][k + 1] if k + 1 < len(kids[node]) else None
            if c <= pos and (nxt is None or pos < nxt):
                steps.append((node, k))
                node = c
                break
    return steps


def _step(kind, f, k, t, s, state, dtype, b=None):
    """one step for all rows: (t, state) of the parent -> of the child.  s: the sibling / the condition / the child (ABS); b: the other
    branch of an IF"""
    with np.errstate(all="ignore"):
        d = t.copy()
        ns = np.zeros(len(t), np.uint8)
        imp = lambda c: np.where(c, IMPOSSIBLE, REQUIRED).astype(np.uint8)  # noqa: E731
        if kind == "T":
            other = np.where(t == b, FREE, IMPOSSIBLE)
            ns = np.where((s > 0) == (k == 1), REQUIRED, other).astype(np.uint8)
        elif f == R.F_ADD:
            d = t - s
        elif f == R.F_SUB:
            d = t + s if k == 0 else s - t
        elif f == R.F_MUL:
            d = np.where(s != 0, t / np.where(s != 0, s, 1), t)
            ns = np.where(s != 0, REQUIRED, np.where(t == 0, FREE, IMPOSSIBLE)).astype(np.uint8)
        elif f == R.F_DIV and k == 0:
            d, ns = t * s, imp(s == 0)
        elif f == R.F_DIV:
            both = (t != 0) & (s != 0)
            d = np.where(both, s / np.where(both, t, 1), t)
            ns = np.where(both, REQUIRED, np.where((t == 0) & (s == 0), FREE, IMPOSSIBLE)).astype(np.uint8)
        elif f == R.F_MAX:
            ns = imp(~(t >= s))
        elif f == R.F_MIN:
            ns = imp(~(t <= s))
        elif f == R.F_NEG:
            d = -t
        elif f == R.F_INV:
            d, ns = np.where(t != 0, dtype(1) / np.where(t != 0, t, 1), t), imp(~(t != 0))
        elif f == R.F_SQRT:
            d, ns = t * t, imp(~(t >= 0))
        elif f == R.F_ABS:
            d, ns = np.where(s < 0, -t, t), imp(~(t >= 0))
        elif f == R.F_EXP:
            d, ns = np.log(np.where(t > 0, t, 1).astype(np.float64)).astype(dtype), imp(~(t > 0))
        elif f == R.F_LOG:
            d = np.exp(t.astype(np.float64)).astype(dtype)
        else:
            raise AssertionError("no rule")
        d = np.asarray(d, dtype)
        ns = np.where(np.isnan(t) | ((kind == "B") & np.isnan(s)), IMPOSSIBLE, ns).astype(np.uint8)
        ns = np.where((ns == REQUIRED) & ~np.isfinite(d), IMPOSSIBLE, ns).astype(np.uint8)
        go = state == REQUIRED
        return np.where(go, d, t).astype(dtype), np.where(go, ns, state).astype(np.uint8)


def tree_desired(value, type_, size, X, y, pos, dtype=np.float32):
    D = X.shape[0]
    nan_row = (np.full(D, np.nan, dtype), np.full(D, IMPOSSIBLE, np.uint8))
    n = live_len(size, len(value))
    if not well_formed(type_, n):
        return (*nan_row, MALFORMED)
    pos = int(pos)
    if not 0 <= pos < n:
        return (*nan_row, POSITION)
    kids = children(type_, n)
    steps = path_to(kids, pos)
    nodes = [R.decode(type_[i], value[i], False, X.shape[1], 1) for i, _ in steps]
    for (kind, f, _), (_, k) in zip(nodes, steps):
        ok = (kind == "B" and f in BINARY_RULES) or (kind == "U" and f in UNARY_RULES) or (kind == "T" and k > 0)
        if not ok:
            return (*nan_row, BLOCKED)
    val = node_values(value, type_, size, X, dtype)
    t = np.asarray(y, dtype).reshape(-1).copy()
    state = np.zeros(D, np.uint8)
    for (kind, f, _), (i, k) in zip(nodes, steps):
        s = val[kids[i][1 - k]] if kind == "B" else val[kids[i][0]]
        b = val[kids[i][3 - k]] if kind == "T" else None
        t, state = _step(kind, f, k, t, s, state, dtype, b)
    return np.where(state == REQUIRED, t, np.nan).astype(dtype), state, OK


def forest_desired(value, type_, size, X, y, pos, dtype=np.float32):
    value, type_, size = np.asarray(value), np.asarray(type_), np.asarray(size)
    pop, D = value.shape[0], np.asarray(X).shape[0]
    desired, state, status = np.empty((pop, D), dtype), np.empty((pop, D), np.uint8), np.empty(pop, np.int32)
    for t in range(pop):
        desired[t], state[t], status[t] = tree_desired(value[t], type_[t], size[t], np.asarray(X), np.asarray(y), pos[t], dtype)
    return desired, state, status


def match(desired, state, status, lib):
    """float64: dist (pop, K), best, const, const_dist (two passes), counts (pop, 3) -- from (pop, D) arrays of desired values"""
    desired, lib = np.asarray(desired, np.float64), np.asarray(lib, np.float64)
    pop, K = desired.shape[0], lib.shape[0]
    dist, best = np.zeros((pop, K)), np.full(pop, -1, np.int32)
    const, const_dist = np.full(pop, np.nan), np.full(pop, np.nan)
    counts = np.stack([(state == s).sum(1) for s in (REQUIRED, FREE, IMPOSSIBLE)], 1).astype(np.int32)
    for t in range(pop):
        req = state[t] == REQUIRED
        if status[t] != OK or not req.any():
            continue
        d = desired[t, req]
        with np.errstate(all="ignore"):
            e = ((d[None, :] - lib[:, req]) ** 2).sum(1)
        e[~np.isfinite(lib[:, req]).all(1)] = np.inf
        dist[t] = e
        if np.isfinite(e).any():
            best[t] = int(np.argmin(e))   # (the first of equal minima)
        const[t] = d.mean()
        const_dist[t] = ((d - d.mean()) ** 2).sum()
    return best, dist, const, const_dist, counts
