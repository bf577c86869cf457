"""TEST-ONLY: numpy restatement of exact semantic intron removal (include/evogp_hip.h evogp_hip_sr_subtree_introns /
evogp_hip_remove_introns, csrc/sr_introns.hip), and the test forests the CPU and GPU tests share.

    equal         E(a, b): one float32 bit pattern, or both NaN (+0.0 and -0.0 differ)
    spans         n = size[0] kept inside [0, L]; span(i) = size[i] kept inside [1, n - i] (what prune_rows_kernel reads)
    candidates    sig[i] != 0: the j in (i, i + span(i)) with sig[j] == sig[i] of smallest (span(j), j); else i
    tree_rep      rep[i] = cand(i) when it is not i and the VALUES of node i and of cand(i) are E-equal on every row; else i.  The values
                  come from the caller (one row per live node): the restatement has no interpreter of its own
    rewrite_row   R(i) emits node rep[i], then R(c) for each child c of rep[i]; written as the per-node walk from the root, so that it
                  is defined for any sizes (recursive_rewrite is the literal rule, for trees whose sizes are their subtree sizes)"""
import functools

import numpy as np

import sr_grad_ref as R
from subtree_ref import extract_subtrees, live_len, well_formed


def equal(a, b):
    """E on float32 arrays, elementwise"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def spans(size_row, n):
    return [min(max(int(size_row[i]), 1), n - i) for i in range(n)]


def candidates(sig_row, size_row, n):
    sp = spans(size_row, n)
    sig_row = np.asarray(sig_row).view(np.uint64) if np.asarray(sig_row).dtype == np.int64 else np.asarray(sig_row, np.uint64)
    cand = list(range(n))
    for i in range(n):
        if sig_row[i] == 0:
            continue
        same = [j for j in range(i + 1, i + sp[i]) if sig_row[j] == sig_row[i]]
        if same:
            cand[i] = min(same, key=lambda j: (sp[j], j))
    return cand


def tree_rep(type_row, size_row, sig_row, values):
    """int16 (L,); ``values``: (n, D) float32, row i the value of the subtree at node i on every data row (ignored for a malformed row)"""
    L = len(type_row)
    rep = np.arange(L, dtype=np.int16)
    n = live_len(size_row, L)
    if not well_formed(type_row, n):
        return rep
    cand = candidates(sig_row, size_row, n)
    for i in range(n):
        if cand[i] != i and equal(values[i], values[cand[i]]).all():
            rep[i] = cand[i]
    return rep


def forest_rep(type_, size, sig, values_of):
    """int16 (pop, L); ``values_of(t)`` -> (n_t, D) float32 for a well-formed tree t"""
    type_, size = np.asarray(type_), np.asarray(size)
    pop, L = type_.shape
    rep = np.tile(np.arange(L, dtype=np.int16), (pop, 1))
    for t in range(pop):
        if well_formed(type_[t], live_len(size[t], L)):
            rep[t] = tree_rep(type_[t], size[t], np.asarray(sig)[t], values_of(t))
    return rep


def kept_nodes(size_row, rep_row, n):
    """bool (n,): the per-node walk from the root.  A rep that is no descendant of its node by the spans counts as the node."""
    sp = spans(size_row, n)
    r_of = [int(rep_row[i]) if i < int(rep_row[i]) < i + sp[i] else i for i in range(n)]
    keep = np.zeros(n, bool)
    for k in range(n):
        cur = 0
        while True:
            r = r_of[cur]
            if k < r or k >= r + sp[r]:
                break
            if k == r:
                keep[k] = True
                break
            c = r + 1
            while k >= c + sp[c]:
                c += sp[c]
            cur = c
    return keep


def rewrite_row(value, type_, size, rep_row):
    """-> (value, type, size, removed)"""
    L = len(value)
    n = live_len(size, L)
    if not well_formed(type_, n):
        return value.copy(), type_.copy(), size.copy(), 0
    sp = spans(size, n)
    keep = kept_nodes(size, rep_row, n)
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    ov, ot, os_ = np.zeros(L, np.float32), np.zeros(L, np.int16), np.zeros(L, np.int16)
    for k in range(n):
        if keep[k]:
            at = before[k]
            ov[at], ot[at], os_[at] = value[k], type_[k], before[k + sp[k]] - at
    return ov, ot, os_, n - int(before[n])


def rewrite(value, type_, size, rep):
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    ov, ot, os_ = np.zeros_like(value), np.zeros_like(type_), np.zeros_like(size)
    removed = np.zeros(value.shape[0], np.int32)
    for t in range(value.shape[0]):
        ov[t], ot[t], os_[t], removed[t] = rewrite_row(value[t], type_[t], size[t], np.asarray(rep)[t])
    return ov, ot, os_, removed


def recursive_rewrite(value, type_, size, rep_row):
    """the rule as the contract words it, for a well-formed tree whose sizes are its subtree sizes: the list of emitted node indices"""
    out = []

    def arity(i):
        t = int(type_[i])
        return 0 if t in (R.T_VAR, R.T_CONST) else 1 if t == R.T_UFUNC else 2 if t == R.T_BFUNC else 3

    def emit(i):
        r = int(rep_row[i])
        r = r if i < r < i + int(size[i]) else i
        out.append(r)
        c = r + 1
        for _ in range(arity(r)):
            emit(c)
            c += int(size[c])

    emit(0)
    return out


# ---- values for the restatement from an evaluator of whole rows ---------------------------------------------------------------------
def subtree_rows(value, type_, size, trees):
    """every subtree of the well-formed trees ``trees`` as a row of its own -> ((value, type, size), offsets): tree trees[k] owns the rows
    [offsets[k], offsets[k + 1])"""
    L = value.shape[1]
    clamped = size.copy()
    clamped[:, 0] = [live_len(size[t], L) for t in range(size.shape[0])]
    parts = [extract_subtrees(value, type_, clamped, int(t)) for t in trees]
    offsets = np.concatenate([[0], np.cumsum([p[0].shape[0] for p in parts])]).astype(np.int64)
    if not parts:
        return tuple(np.zeros((0, L), d) for d in (np.float32, np.int16, np.int16)), offsets
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3)), offsets


def formed_trees(type_, size):
    L = type_.shape[1]
    return [t for t in range(type_.shape[0]) if well_formed(type_[t], live_len(size[t], L))]


def values_from(evaluate, value, type_, size):
    """``values_of`` for forest_rep: ``evaluate(value, type, size)`` -> (rows, D) float32 predictions of whole rows, called once on the
    extracted subtrees of every well-formed tree"""
    value, type_, size = np.asarray(value, np.float32), np.asarray(type_, np.int16), np.asarray(size, np.int16)
    trees = formed_trees(type_, size)
    rows, offsets = subtree_rows(value, type_, size, trees)
    P = np.asarray(evaluate(*rows), np.float32) if len(rows[0]) else np.zeros((0, 1), np.float32)
    at = {t: k for k, t in enumerate(trees)}
    return lambda t: P[offsets[at[t]]:offsets[at[t] + 1]]


def oracle_evaluate(oracle, X):
    X = np.ascontiguousarray(X, np.float32)

    def evaluate(v, t, s):
        with np.errstate(all="ignore"):
            return oracle.batch_evaluate(v, t, s, X, 1)[:, :, 0]
    return evaluate


# ---- hand-built trees -----------------------------------------------------------------------------------------------------------------
U, B, V, C, T = R.T_UFUNC, R.T_BFUNC, R.T_VAR, R.T_CONST, 4


def x(i):
    return [(float(i), V, 1)]


def c(v):
    return [(np.float32(v), C, 1)]


def un(f, a):
    return [(float(f), U, 1 + len(a))] + a


def op(f, a, b):
    return [(float(f), B, 1 + len(a) + len(b))] + a + b


def iff(a, b, d):
    return [(0.0, T, 1 + len(a) + len(b) + len(d))] + a + b + d


def forest(trees, L):
    value, type_, size = np.zeros((len(trees), L), np.float32), np.zeros((len(trees), L), np.int16), np.zeros((len(trees), L), np.int16)
    for t, nodes in enumerate(trees):
        assert len(nodes) <= L
        for i, (v, ty, s) in enumerate(nodes):
            value[t, i], type_[t, i], size[t, i] = v, ty, s
    return value, type_, size


# the identities of the issue, as wrappers of a subtree a (b: any other subtree)
WRAPS = {
    "x+0": lambda a, b: op(R.F_ADD, a, c(0.0)),
    "1*x": lambda a, b: op(R.F_MUL, c(1.0), a),
    "x-(y-y)": lambda a, b: op(R.F_SUB, a, op(R.F_SUB, b, b)),
    "max(x,x)": lambda a, b: op(R.F_MAX, a, a),
    "neg(neg(x))": lambda a, b: un(R.F_NEG, un(R.F_NEG, a)),
    "IF(c,a,a)": lambda a, b: iff(b, a, a),
    "(x*2)/2": lambda a, b: op(R.F_DIV, op(R.F_MUL, a, c(2.0)), c(2.0)),
}
ARITH_WRAPS = ("x+0", "1*x", "x-(y-y)", "(x*2)/2")


def random_nodes(rng, funcs, var_len, max_depth, wrap, wraps, leaf_prob=0.25):
    """a random tree (grad_trees.random_tree's shape) in which every subtree is, with probability ``wrap``, put inside one of ``wraps``"""
    def gen(depth):
        if depth >= max_depth or rng.random() < leaf_prob:
            a = c(rng.uniform(0.5, 1.5)) if rng.random() < 0.5 else x(int(rng.integers(var_len)))
        else:
            f = int(rng.choice(funcs))
            if f >= R.F_SIN:
                a = un(f, gen(depth + 1))
            elif f >= R.F_ADD:
                a = op(f, gen(depth + 1), gen(depth + 1))
            else:
                a = iff(gen(depth + 1), gen(depth + 1), gen(depth + 1))
        if wrap > 0 and rng.random() < wrap:
            a = WRAPS[wraps[int(rng.integers(len(wraps)))]](a, x(int(rng.integers(var_len))))
        return a
    return gen(0)


ALL_FUNCS = list(range(29))
ARITH = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV]
# name -> (funcs, gp_len, var_len): the forests of tests/test_gpu_introns.py; tests/test_intron_ref.py holds them to the coverage condition
FORESTS = {
    "arith_L64": ("arith", 64, 3), "all_L64": ("all", 64, 3), "arith_L1024": ("arith", 1024, 3), "all_L1024": ("all", 1024, 3),
    "all_L64_v40": ("all", 64, 40),
}
WRAPPED_SHARE = 0.5    # of the trees; inside such a tree every subtree is wrapped with probability WRAP
WRAP = 0.25
MAX_D = 300


@functools.lru_cache(maxsize=None)
def shared_forest(name, pop=257):
    """``(value, type, size), X (MAX_D, var_len)``: random trees, half of them with wrapped subtrees; in the long-row forests one tree in
    eight is deep enough to pass 64 nodes (the global tapes), and rows 0 .. 4 are malformed or degenerate.  X has both signs, so that
    few nodes are introns by accident (abs(x), IF(x, a, b) on positive data ...)"""
    import zlib
    kind, L, var_len = FORESTS[name]
    rng = np.random.default_rng([20261021, zlib.crc32(name.encode()), pop])
    funcs, wraps = (ARITH, ARITH_WRAPS) if kind == "arith" else (ALL_FUNCS, tuple(WRAPS))
    trees = []
    for t in range(pop):
        deep = L > 64 and t % 8 == 5
        while True:
            nodes = random_nodes(rng, funcs, var_len, (9 if kind == "arith" else 7) if deep else 4, WRAP if rng.random() < WRAPPED_SHARE else 0.0,
                                 wraps, leaf_prob=0.1 if deep else 0.25)
            if len(nodes) <= min(L, 400) and (not deep or len(nodes) > 64):
                break
        trees.append(nodes)
    value, type_, size = forest(trees, L)
    size[1, 0] = 0                                    # malformed: n = 0
    size[2, 0] = -3                                   # n < 0
    type_[3, :3], size[3, :3], value[3, :3] = (B, V, 0), (2, 1, 0), (R.F_ADD, 0.0, 0.0)   # an ADD with one operand under n = 2
    value[4], type_[4], size[4] = 0, 0, 0
    value[4, 0], type_[4, 0], size[4, 0] = 1.25, C, 1  # n = 1
    X = rng.normal(0.0, 1.0, (MAX_D, var_len)).astype(np.float32)
    X[rng.random(X.shape) < 0.02] = 0.0
    return (value, type_, size), X
