"""TEST-ONLY: a float64 numpy restatement of the input-gradient pass (csrc/sr_xgrad.hip): the forward semantics and the adjoint table are
those of tests/sr_grad_ref.py (imported, not copied); what is new is the seed (1 at the root), the sum over the occurrences of a variable
and the two epilogues.

``forest_xgrad(value, type, size, X, wrt)`` -> ``(pred (pop, D), d (V, pop, D), scale (V, pop, D))``
    d[k][t][r]      d tree_t / d x_{wrt[k]} at X[r]: the sum, in prefix order, of the adjoints of the VAR nodes that hold wrt[k]
    scale[k][t][r]  sum |adjoint| over those occurrences: the scale of the per-entry tolerances (what sr_grad_ref calls gabs, per row)
    Malformed trees: NaN everywhere.  A variable the tree does not hold: d = +0.0, scale = 0.
``derivative_loss(...)`` -> ``(loss (pop, 1 + V) float64, viol (pop, V) int32)``: the fused epilogue on the float32-rounded pred and d.
``comparable(...)``: the exclusion rule of the tolerance tests -- see its docstring."""
import numpy as np

from sr_grad_ref import ARITY, _where, binary, binary_adjoint, decode, unary, unary_adjoint

JITTER = 3.0 * 2.0 ** -24


def well_formed(nodes):
    h = 0
    for kind, _, _ in reversed(nodes):
        h += 1 - ARITY[kind]
        if h < 1:
            return False
    return len(nodes) > 0 and h == 1


def tree_xgrad(value, type_, size, X, wrt, jitter_seed=None, dtype=np.float64):
    """one tree: (pred[D], d[V][D], scale[V][D]).  ``jitter_seed``: multiply the result of every function node and every adjoint handed to an
    operand by 1 +- 3 * 2^-24, the sign drawn per node and row (the perturbation of ``comparable``).  ``dtype``: the arithmetic
    (float32 for measurements of the rule itself; the restatement is float64)"""
    L = len(value)
    D, var_len = X.shape
    V = len(wrt)
    n = min(max(int(size[0]), 0), L)
    nodes = [decode(type_[i], value[i], False, var_len, 1) for i in range(n)]
    if not well_formed(nodes):
        nan = np.full(D, np.nan)
        return nan, np.full((V, D), np.nan), np.full((V, D), np.nan)
    rng = None if jitter_seed is None else np.random.default_rng(jitter_seed)

    def jit(x):
        if rng is None:
            return x
        return (x * (1.0 + JITTER * rng.choice([-1.0, 1.0], D))).astype(dtype)

    X = X.astype(dtype)
    val, kids = [None] * n, [None] * n
    stack = []
    with np.errstate(all="ignore"):
        for i in reversed(range(n)):
            kind, f, _ = nodes[i]
            if kind == "C":
                val[i] = np.full(D, f, dtype)
            elif kind == "V":
                val[i] = X[:, f]
            else:
                k = [stack.pop() for _ in range(ARITY[kind])]   # top of stack first: a, b, c
                kids[i] = k
                ops = [val[j] for j in k]
                if kind == "U":
                    r = unary(f, ops[0])
                elif kind == "B":
                    r = binary(f, ops[0], ops[1])
                else:
                    r = _where(ops[0] > 0, ops[1], ops[2])
                val[i] = jit(np.asarray(r, dtype))
            stack.append(i)
        adj = [None] * n
        adj[0] = np.ones(D, dtype)
        d = np.zeros((V, D), dtype)
        scale = np.zeros((V, D), dtype)
        col = {v: k for k, v in enumerate(wrt)}
        zero = np.zeros(D, dtype)
        for i in range(n):
            kind, f, _ = nodes[i]
            if kind == "V":
                if f in col:
                    d[col[f]] = d[col[f]] + adj[i]
                    scale[col[f]] = scale[col[f]] + np.abs(adj[i])
                continue
            if kind == "C":
                continue
            g, k = adj[i], kids[i]
            ops = [val[j] for j in k]
            if kind == "U":
                out = [unary_adjoint(f, ops[0], val[i], g)]
            elif kind == "B":
                out = list(binary_adjoint(f, ops[0], ops[1], val[i], g))
            else:
                take_b = ops[0] > 0
                out = [zero, _where(take_b, g, 0.0), _where(take_b, 0.0, g)]
            for j, dj in zip(k, out):
                adj[j] = jit(np.asarray(dj, dtype) + zero)
    return val[0], d, scale


def forest_xgrad(value, type_, size, X, wrt, jitter_seed=None, dtype=np.float64):
    value, type_, size, X = np.asarray(value), np.asarray(type_), np.asarray(size), np.asarray(X)
    wrt = [int(v) for v in wrt]
    pop, D, V = value.shape[0], X.shape[0], len(wrt)
    pred, d, scale = np.zeros((pop, D), dtype), np.zeros((V, pop, D), dtype), np.zeros((V, pop, D), dtype)
    for t in range(pop):
        seed = None if jitter_seed is None else [jitter_seed, t]
        pred[t], d[:, t], scale[:, t] = tree_xgrad(value[t], type_[t], size[t], X, wrt, seed, dtype)
    return pred, d, scale


def loss_columns(pred32, d32, y, dy=None, dmin=None, dmax=None):
    """the fused epilogue from float32 predictions (pop, D) and derivatives (V, pop, D): ``(loss (pop, 1 + V) float64, viol (pop, V) int32)``.
    A column is NaN exactly when one of its row terms is not finite; a violation is a row with !(dmin <= g <= dmax), NaN included."""
    pred32, d32 = np.asarray(pred32, np.float32), np.asarray(d32, np.float32)
    V, pop, D = d32.shape
    y = np.asarray(y, np.float32).reshape(D).astype(np.float64)
    dy = np.zeros((D, V)) if dy is None else np.asarray(dy, np.float32).astype(np.float64)
    lo = np.full(V, -np.inf, np.float32) if dmin is None else np.asarray(dmin, np.float32)
    hi = np.full(V, np.inf, np.float32) if dmax is None else np.asarray(dmax, np.float32)
    loss = np.zeros((pop, 1 + V))
    viol = np.zeros((pop, V), np.int32)
    with np.errstate(all="ignore"):
        terms = [(pred32.astype(np.float64) - y[None, :]) ** 2] + [(d32[k].astype(np.float64) - dy[None, :, k]) ** 2 for k in range(V)]
        for c, term in enumerate(terms):
            loss[:, c] = np.where(np.isfinite(term).all(1), term.sum(1) / D, np.nan)
        for k in range(V):
            viol[:, k] = (~((lo[k] <= d32[k]) & (d32[k] <= hi[k]))).sum(1)
    return loss, viol


def derivative_loss(value, type_, size, X, y, dy, wrt, dmin=None, dmax=None):
    pred, d, _ = forest_xgrad(value, type_, size, X, wrt)
    with np.errstate(all="ignore"):
        return loss_columns(pred.astype(np.float32), d.astype(np.float32), y, dy, dmin, dmax)


def comparable(value, type_, size, X, wrt, base=None):
    """bool (V, pop, D): the entries (tree, row, variable) a tolerance test compares.  All of: the float64 prediction, derivative and
    scale are finite; under two draws (seeds 0 and 1) of the 3-ulp node jitter the derivative moves by at most 1e-4 * scale + 1e-9; the
    re-evaluation stays finite.  ``base``: the unjittered ``forest_xgrad`` result, if the caller has it."""
    pred, d, scale = base if base is not None else forest_xgrad(value, type_, size, X, wrt)
    with np.errstate(all="ignore"):
        ok = np.isfinite(pred)[None] & np.isfinite(d) & np.isfinite(scale)
        for seed in (0, 1):
            pj, dj, sj = forest_xgrad(value, type_, size, X, wrt, jitter_seed=seed)
            ok &= np.isfinite(pj)[None] & np.isfinite(dj) & np.isfinite(sj)
            ok &= ~(np.abs(dj - d) > 1e-4 * scale + 1e-9)
    return ok
