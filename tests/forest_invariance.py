"""TEST-ONLY: three invariants every op that takes a forest must keep, one table with a row per op, and the checker
(tests/test_forest_invariance_host.py on the CPU stand-ins, tests/test_gpu_forest_invariance.py on the device).

  A  dead words   words of an input row behind size[t][0] may hold anything (include/evogp_hip.h, head comment): no output depends on them
  B  row order    permuting the rows of the forest (and the per-tree inputs) permutes the outputs and changes nothing else
  C  slices       op(forest[a:b]) == op(forest)[a:b]: a tree's result depends on neither the population size nor its neighbours

Floats are compared as bit patterns with every NaN mapped to one pattern (helpers.fbits), integers exactly; nothing is left out.
The dead words `stale_tails` writes are words a live prefix of the same forest could hold (type codes of the alphabet, function ids
0..28, variable indices < var_len, OUT indices < out_len): a kernel that reads one computes with it and indexes no table out of range."""
import functools
import os
import sys

import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
from evogp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sr_grad_ref as R  # noqa: E402
from dedup_cases import comb  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, out_word, random_forest  # noqa: E402
from helpers import depth2leaf, fbits, roulette_uniform  # noqa: E402,F401
from test_gpu_linear_scaling import _chain  # noqa: E402

U, B, V, C = R.T_UFUNC, R.T_BFUNC, R.T_VAR, R.T_CONST
NORMAL = 44           # EVOGP_LM_NORMAL_WORDS
PLANT_FROM = 11       # the planted patterns go to the first rows from here on that have room for them


# ---- transforms -----------------------------------------------------------------------------------------------------------------------
def live_len(size):
    return np.clip(size[:, 0].astype(np.int64), 0, size.shape[1])


def dead_mask(size):
    """bool[pop][L]: the words behind the live prefix; position 0 never (it holds n, also for an out-of-range row)"""
    m = np.arange(size.shape[1])[None, :] >= live_len(size)[:, None]
    m[:, 0] = False
    return m


def _patterns(L, out_len):
    """name -> (value, type, size) words written from position n on; None keeps the base fill's word"""
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    p = {
        "nan_const": [(nan, C, 1)], "pinf_const": [(inf, C, 1)], "ninf_const": [(-inf, C, 1)], "zero_const": [(np.float32(0.0), C, 1)],
        "library_words": [(np.float32(R.F_SIN), U, 2), (np.float32(R.F_EXP), U, 2), (np.float32(R.F_LOG), U, 2), (np.float32(R.F_TAN), U, 2),
                          (np.float32(R.F_POW), B, 3)],
        "div_const0": [(np.float32(R.F_DIV), B, 3), (np.float32(0.0), C, 1)],
        "size_words": [(None, None, 0), (None, None, -3), (None, None, L + 5)],
        "second_tree": None,
    }
    if out_len > 1:
        p["out_flagged"] = [(out_word(R.F_ADD, 1), B | 0x80, 3), (out_word(R.F_SIN, out_len - 1), U | 0x80, 2)]
    return p


def stale_tails(rng, value, type_, size, out_len):
    """-> (value, type, size, planted): copies with EVERY word behind the live prefix rewritten (n = size[t][0] clamped to [0, L]; position
    0 and rows with n == L stay as they are).  Base fill: per dead position the (value, type, size) triple of a random live position of a
    random other row.  On top, planted = {pattern name: row}: the named patterns from position n of their row on."""
    value, type_, size = value.copy(), type_.copy(), size.copy()
    pop, L = value.shape
    n = live_len(size)
    dead = dead_mask(size)
    rows, cols = np.nonzero(np.arange(L)[None, :] < n[:, None])   # every live position of the forest
    assert len(rows), "no live word to copy from"
    dt, di = np.nonzero(dead)
    pick = rng.integers(0, len(rows), len(dt))
    for _ in range(8):   # a word of ANOTHER row
        own = rows[pick] == dt
        if not own.any() or len(np.unique(rows)) < 2:
            break
        pick[own] = rng.integers(0, len(rows), int(own.sum()))
    value[dt, di], type_[dt, di], size[dt, di] = value[rows[pick], cols[pick]], type_[rows[pick], cols[pick]], size[rows[pick], cols[pick]]
    planted = {}
    order = [t for t in list(range(PLANT_FROM, pop)) + list(range(min(PLANT_FROM, pop)))]
    free = [t for t in order if 1 <= n[t] <= L - 8]
    for name, words in _patterns(L, out_len).items():
        if not free:
            break
        t = free.pop(0)
        if words is None:   # a complete second tree: another row's whole live prefix
            src = [u for u in range(pop) if u != t and 3 <= n[u] <= L - n[t]]
            if not src:
                continue
            u = src[int(rng.integers(len(src)))]
            words = [(value[u, i], type_[u, i], size[u, i]) for i in range(n[u])]
        for k, (v, ty, s) in enumerate(words):
            i = n[t] + k
            if v is not None:
                value[t, i], type_[t, i] = v, ty
            size[t, i] = s
        planted[name] = t
    return value, type_, size, planted


def permute(rng, pop):
    """row permutations: a random one and the reversal"""
    return [rng.permutation(pop), np.arange(pop)[::-1].copy()]


def slices(pop):
    """[0:1], [pop-1:pop], a slice aligned to no wave or batch ([61:131] where the forest has it) and [0:pop-1]"""
    mid = (61, 131) if pop > 131 else ((pop // 4) | 1, ((3 * pop) // 4) | 1)
    out = [(0, 1), (pop - 1, pop), mid, (0, pop - 1)]
    return [(a, b) for a, b in out if 0 <= a < b <= pop]


# ---- cases ----------------------------------------------------------------------------------------------------------------------------
# the smallest shapes that still reach every path the kernels switch on
CASES = {
    "arith_L64": dict(funcs="arith", L=64, var_len=3, pop=257, D=70, out_len=1),       # LEAN builds, packed compiler, one ragged tile
    "all_L64_v13": dict(funcs="all", L=64, var_len=13, pop=257, D=1100, out_len=1),    # FULL builds, the 32-wide tuple, !single
    "all_L1024_v40": dict(funcs="all", L=1024, var_len=40, pop=24, D=70, out_len=1),   # long rows, var_len > 32: scratch-stack kernels alone
    "multi_L64": dict(funcs="all", L=64, var_len=3, pop=63, D=70, out_len=4),          # multi-output ops
}
NO_DATA_CASES = ("arith_L64", "all_L1024_v40")


class Case:
    pass


def _set(value, type_, size, t, nodes):
    value[t], type_[t], size[t] = 0, 0, 0
    for i, (v, ty, s) in enumerate(nodes):
        value[t, i], type_[t, i], size[t, i] = v, ty, s


def _spd_normal(rng, pop):
    """rows of EVOGP_LM_NORMAL_WORDS: the upper triangle of a positive definite A, then b"""
    out = np.zeros((pop, NORMAL), np.float32)
    iu = np.triu_indices(8)
    for t in range(pop):
        J = rng.normal(size=(8, 12))
        out[t, :36] = (J @ J.T / 12.0)[iu]
        out[t, 36:] = rng.normal(size=8)
    return out


@functools.lru_cache(maxsize=None)
def build_case(name, pop=None, D=None):
    """the forest of a case (zero tails), the same forest with stale tails, the dataset and every shared table; numpy throughout"""
    spec = dict(CASES[name])
    pop, D = pop or spec["pop"], D or spec["D"]
    L, var_len, out_len = spec["L"], spec["var_len"], spec["out_len"]
    assert pop >= 22, "the row layout needs 22 rows"
    import zlib
    rng = np.random.default_rng([20261020, zlib.crc32(name.encode()), pop, D])
    fs = ARITH if spec["funcs"] == "arith" else ALL_FUNCS
    value, type_, size = random_forest(rng, pop, L, fs, var_len, out_len, max_depth=7 if L > 64 else 5)
    short = random_forest(rng, pop, L, fs, var_len, out_len, max_depth=3)
    for t in range(PLANT_FROM, min(pop, PLANT_FROM + 11)):   # rows with room for a planted tail
        value[t], type_[t], size[t] = short[0][t], short[1][t], short[2][t]
    for k, t in enumerate(range(2, pop, 7)):   # deeper than the 16-entry register stack: the general kernels
        ops = 20 if L == 64 else (20, 100, 400)[k % 3]
        _set(value, type_, size, t, _chain(rng, ops, var_len, (R.F_ADD, R.F_SUB, R.F_MUL) if spec["funcs"] != "arith" else ARITH))
    _set(value, type_, size, 0, [(np.float32(1.25), C, 1)])                                          # n == 1
    if spec["funcs"] != "arith":
        value[1], type_[1], size[1] = comb(L // 2, L, rng, unary_root=True)                          # n == L
    else:
        # a tree of binary functions has an odd number of nodes: in the arithmetic case the row WITHOUT a tail is a chain of L - 1 nodes
        # and one more leaf under n = L (two values left: malformed for the evaluating ops, and still a row that must stay untouched)
        _set(value, type_, size, 1, _chain(rng, (L - 2) // 2, var_len, ARITH) + [(np.float32(0.75), C, 1)])
        size[1, 0] = L
    _set(value, type_, size, 3, [(np.float32(0.5), C, 1)]); size[3, 0] = 0          # malformed: n = 0
    size[4, 0] = -2                                                                  # n < 0
    size[5, 0] = L + 1                                                               # n > L (never the last row)
    if L > 64:
        value[6], type_[6], size[6] = comb(32, L, rng)                               # n = 63
        value[7], type_[7], size[7] = comb(32, L, rng, unary_root=True)              # n = 64
        value[8], type_[8], size[8] = comb(33, L, rng)                               # n = 65
        value[10], type_[10], size[10] = comb(40, L, rng)                            # a comb of 79 nodes
    c = Case()
    c.name, c.pop, c.D, c.L, c.var_len, c.out_len, c.funcs = name, pop, D, L, var_len, out_len, spec["funcs"]
    c.forest = (value, type_, size)
    sv, st, ss, c.planted = stale_tails(rng, value, type_, size, out_len)
    c.stale = (sv, st, ss)
    c.func_mask = int(sum(1 << f for f in fs))
    X = rng.uniform(0.5, 1.5, (D, var_len)).astype(np.float32)
    y = np.stack([(1.5 * X[:, 0] ** 2 - X[:, -1] + 0.3 * o).astype(np.float32) for o in range(out_len)], 1)
    W = rng.uniform(0.5, 1.5, (3, D)).astype(np.float32)
    W[rng.random((3, D)) < 0.3] = 0.0   # exact zeros: the 8-column build
    W[:, 0] = 1.0
    nd = 2
    cost = rng.integers(1, 5, 32).astype(np.int32)
    operand_limit = np.full((32, 3), -1, np.int32)
    operand_limit[R.F_DIV, 1], operand_limit[R.F_ADD, 0] = 3, 9
    c.shared = dict(
        D=D, var_len=var_len, out_len=out_len, func_mask=c.func_mask, X=X, y=y, y1=np.ascontiguousarray(y[:, 0]),
        cls=rng.integers(0, out_len, D).astype(np.int32), W=W, w=np.ascontiguousarray(W[1]),
        lower=np.full(var_len, -2.0, np.float32), upper=np.full(var_len, 2.0, np.float32), wrt=np.array([0, var_len - 1], np.int32),
        var_units=(rng.integers(-1, 2, (var_len, nd)) * 25200).astype(np.int32), label_units=np.array([25200, 0], np.int32),
        cost=cost, operand_limit=operand_limit, rule_outer=np.array([1 << R.F_MUL | 1 << R.F_SIN, 1 << R.F_ADD], np.int32),
        rule_inner=np.array([1 << R.F_ADD, 1 << R.F_SUB | 1 << R.F_EXP], np.int32), rule_limit=np.array([1, 0], np.int32),
        rnd=rng.integers(0, 2 ** 31 - 1, (6, 4 * pop)).astype(np.int32), seed=int(rng.integers(1, 1 << 30)),
        donors=stale_tails(rng, *random_forest(rng, pop, L, fs, var_len, out_len, max_depth=2), out_len)[:3],
    )
    cand = (value + rng.uniform(-0.05, 0.05, value.shape)).astype(np.float32)
    loss = rng.uniform(0.5, 2.0, pop).astype(np.float32)
    loss[3::9] = np.nan
    c.per_tree = dict(
        rows=rng.uniform(0.5, 1.5, (pop, var_len)).astype(np.float32),
        node_err=np.where(rng.random((pop, L)) < 0.1, np.nan, rng.uniform(0.1, 2.0, (pop, L))).astype(np.float32),
        node_const=np.where(rng.random((pop, L)) < 0.7, np.nan, rng.uniform(-1, 1, (pop, L))).astype(np.float32),
        coef=np.where(rng.random((pop, 2)) < 0.05, np.nan, rng.uniform(-2, 2, (pop, 2))).astype(np.float32),
        cand=cand, loss=loss, grad=rng.normal(size=(pop, L)).astype(np.float32),
        loss_cand=(loss * rng.choice([0.5, 1.5], pop)).astype(np.float32), grad_cand=rng.normal(size=(pop, L)).astype(np.float32),
        step=rng.uniform(0.01, 0.1, pop).astype(np.float32), normal=_spd_normal(rng, pop), normal_cand=_spd_normal(rng, pop),
        damping=rng.choice([1e-3, 1.0, 100.0], pop).astype(np.float32),
        mut_word=rng.integers(0, 2 ** 31 - 1, pop).astype(np.int64),
        donors=stale_tails(rng, *random_forest(rng, pop, L, fs, var_len, out_len, max_depth=2), out_len)[:3],
    )
    return c


# ---- adapters -------------------------------------------------------------------------------------------------------------------------
hip, cu = torch.ops.evogp_hip, torch.ops.evogp_cuda


def _d(a, device):
    """a tensor of its own on the device: an in-place op writes a clone, never the case's arrays"""
    return torch.from_numpy(np.array(a, copy=True, order="C")).to(device)


def _f(f, device):
    return [_d(a, device) for a in f]


def _o(res):
    res = res if isinstance(res, (tuple, list)) else (res,)
    return tuple(r.detach().cpu().numpy() for r in res)


def _head(f, s):
    return (f[0].shape[0], s["D"], f[0].shape[1], s["var_len"], s["out_len"])


def _data_op(op, *, mse=None, y="y", tail=()):
    """an op of the shape (pop, D, L, var_len, out_len, [use_mse,] forest, X, y, *tail)"""
    def call(f, s, p, device):
        args = list(_head(f, s)) + ([mse] if mse is not None else []) + _f(f, device) + [_d(s["X"], device)]
        if y is not None:
            args.append(_d(s[y], device))
        return _o(op(*args, *[t(s, device) if callable(t) else t for t in tail]))
    return call


def _forget(device):
    """an unhinted fitness call follows what the last call on its population shape observed; the GPU tests drop the
    observations in front of such a call (tests/gpu_capi.py sr_fitness), and so does this one"""
    if str(device).startswith("cuda"):
        assert _lib.lib.evogp_hip_debug_forget_function_classes() == 0


def _sr_fitness(f, s, p, device):
    _forget(device)
    return _o(cu.tree_SR_fitness(*_head(f, s), True, *_f(f, device), _d(s["X"], device), _d(s["y"], device), 4))


def _sr_fitness_masked(f, s, p, device):
    return _o(hip.tree_SR_fitness_masked(*_head(f, s), True, *_f(f, device), _d(s["X"], device), _d(s["y"], device), 4, s["func_mask"]))


def _evaluate(f, s, p, device):
    pop, L = f[0].shape
    return _o(cu.tree_evaluate(pop, L, s["var_len"], s["out_len"], *_f(f, device), _d(p["rows"], device)))


def _prepared(f, s, p, device):
    pop, L = f[0].shape
    fd = _f(f, device)
    ws, _ = hip.tree_evaluate_prepare(pop, L, s["var_len"], s["out_len"], *fd)
    return _o(hip.tree_evaluate_prepared(pop, L, s["var_len"], s["out_len"], *fd, ws, True, _d(p["rows"], device)))


def _weighted(op, kinds):
    """the (3, D) weight matrix with 30 % exact zeros, and one call with a single row"""
    def call(f, s, p, device):
        fd, X, y = _f(f, device), _d(s["X"], device), _d(s["y"], device)
        out = []
        for W in (s["W"], s["W"][1:2]):
            for kind in kinds:
                out += _o(op(*_head(f, s), *fd, X, y, _d(W, device), *kind))
        return tuple(out)
    return call


def _weighted_row(op, kinds):
    def call(f, s, p, device):
        fd, X, y = _f(f, device), _d(s["X"], device), _d(s["y"], device)
        out = []
        for kind in kinds:
            out += _o(op(*_head(f, s), *fd, X, y, _d(s["w"], device), *kind))
        return tuple(out)
    return call


def _plain(op, *names, tail=()):
    """an op of the shape (forest, shared tables..., scalars...)"""
    def call(f, s, p, device):
        return _o(op(*_f(f, device), *[_d(s[n], device) for n in names], *tail))
    return call


def _classes(f, s, p, device):
    fd = _f(f, device)
    return _o(hip.tree_classes(*fd, hip.tree_hash(*fd)))


def _semantic_classes(f, s, p, device):
    fd, X = _f(f, device), _d(s["X"], device)
    return _o(hip.tree_SR_semantic_classes(*_head(f, s), *fd, X, hip.tree_SR_semantic_hash(*_head(f, s), *fd, X)))


def _prune(f, s, p, device):
    return _o(hip.tree_prune(1, True, True, *_f(f, device), _d(p["node_err"], device), _d(p["node_const"], device)))


def _wrap(f, s, p, device):
    return _o(hip.tree_wrap_linear(min(f[0].shape[1] + 8, 1024), *_f(f, device), _d(p["coef"], device)))


def _const_step(f, s, p, device):
    v, t, sz = _f(f, device)   # (_d copies: the in-place op writes clones)
    cand, loss, grad, step = (_d(p[k].copy(), device) for k in ("cand", "loss", "grad", "step"))
    hip.tree_SR_const_step(3, s["out_len"], v, t, sz, cand, loss, grad, _d(p["loss_cand"], device), _d(p["grad_cand"], device), step)
    return _o((v, cand, loss, grad, step))


def _lm_step(f, s, p, device):
    v, t, sz = _f(f, device)
    cand, loss, normal, damping = (_d(p[k].copy(), device) for k in ("cand", "loss", "normal", "damping"))
    hip.tree_SR_lm_step(3, v, t, sz, cand, loss, normal, _d(p["loss_cand"], device), _d(p["normal_cand"], device), damping)
    return _o((v, cand, loss, normal, damping))


def _node(word, size):
    """a node of the live prefix from a raw word; -1 (the documented copy) for a row that is empty or longer than its storage"""
    n = size[:, 0].astype(np.int64)
    ok = (n >= 1) & (n <= size.shape[1])
    return np.where(ok, word % np.maximum(n, 1), -1).astype(np.int32)


def _mutate(f, s, p, device):
    pop, L = f[0].shape
    return _o(cu.tree_mutate(pop, L, *_f(f, device), _d(_node(p["mut_word"], f[2]), device), *_f(p["donors"], device)))


def _crossover(f, s, p, device):
    pop, L = f[0].shape
    li, ri = p["li"], p["ri"]
    ln, rn = _node(p["lw"], f[2][li]), _node(p["rw"], f[2][ri])
    return _o(cu.tree_crossover(pop, len(li), L, *_f(f, device), *[_d(a.astype(np.int32), device) for a in (li, ri, ln, rn)]))


N_OFF = 48   # offspring of a breed_rows call


def _breed_rows(f, s, p, device):
    pop, L = f[0].shape
    out_rows = 1 + N_OFF
    donors = [a[:out_rows] if a.shape[0] >= out_rows else np.concatenate([a] * (out_rows // a.shape[0] + 1))[:out_rows] for a in s["donors"]]
    return _o(hip.breed_rows(out_rows, L, *_f(f, device), _d(p["elite"].astype(np.int32), device), _d(p["parents"].astype(np.int32), device),
                             _d(s["rnd"][:, :N_OFF], device), 1 << 30, *_f(donors, device), 0, out_rows))


def _select_rows(forest, per_tree, sel):
    """the default: every per-tree input and every output is indexed by tree"""
    if len(sel) == forest[0].shape[0] and np.array_equal(sel, np.arange(len(sel))):
        return per_tree, per_tree, sel
    return per_tree, {k: (tuple(a[sel] for a in v) if isinstance(v, tuple) else v[sel]) for k, v in per_tree.items()}, sel


def _usable(forest, sel):
    n = forest[2][sel, 0].astype(np.int64)
    ok = sel[(n >= 1) & (n <= forest[2].shape[1])]
    return ok if len(ok) else sel


def _select_pairs(forest, per_tree, sel):
    """tree_crossover names its parents by row: the pairs are drawn among the rows of `sel`, by forest row for the call on the whole
    forest and by position for the call on the selection; the outputs (one row per pair) must be equal as they are"""
    k = np.arange(64)
    a, b = k % len(sel), (7 * k + 3) % len(sel)
    words = dict(lw=per_tree["mut_word"][:1].repeat(64) + 977 * k, rw=per_tree["mut_word"][-1:].repeat(64) + 3331 * k)
    return dict(words, li=sel[a], ri=sel[b]), dict(words, li=a, ri=b), None


def _select_lists(forest, per_tree, sel):
    """breed_rows names the elite and the parents by row: one elite and up to 16 parents among the rows of `sel`"""
    ok = _usable(forest, sel)
    parents = ok[:: max(1, len(ok) // 16)][:16]
    pos = {int(t): i for i, t in enumerate(sel)}
    where = lambda rows: np.array([pos[int(t)] for t in rows], np.int64)  # noqa: E731
    return dict(elite=sel[:1], parents=parents), dict(elite=where(sel[:1]), parents=where(parents)), None


def _order(f):
    n = f[2][:, 0].astype(np.int64)
    return np.flatnonzero((n >= 1) & (n <= f[2].shape[1]))[:16].astype(np.int32)


def _breed_default(f, s, p, device):
    pop, L = f[0].shape
    order = _order(f)
    donors = [a[:pop - 2] for a in s["donors"]]
    return _o(hip.breed_default(pop, L, 2, len(order), *_f(f, device), _d(order, device), _d(s["rnd"][:, :pop - 2], device), 1 << 30,
                                *_f(donors, device), True))


def _breed_default_rows(f, s, p, device):
    pop, L = f[0].shape
    order = _order(f)
    donors = [a[:pop - 2] for a in s["donors"]]
    return _o(hip.breed_default_rows(pop, L, 2, len(order), *_f(f, device), _d(order, device), _d(s["rnd"][:, :pop - 2], device), 1 << 30,
                                     *_f(donors, device), 1, pop - 2))


def _breed_rows_hashed(f, s, p, device):
    pop, L = f[0].shape
    order = _order(f)
    return _o(hip.breed_rows_hashed(pop, L, *_f(f, device), _d(order[:2], device), _d(order, device), s["seed"], 3, 1 << 30,
                                    *_f(s["donors"], device), 0, pop))


def _structural(f, s, p, device):
    fd = _f(f, device)
    return _o(hip.structural_mutate(0, 0.7, 0, False, 2, s["seed"], 5, *fd, True)) + _o(hip.structural_mutate(1, 0.7, 0, True, 0, s["seed"], 6, *fd, True))


def _insert(f, s, p, device):
    return _o(hip.insert_mutate(1 << 30, 2, s["seed"], 7, *_f(f, device), *_f(s["donors"], device), True))


def _roulettes(device):
    p = np.zeros(29, np.float32)
    p[[1, 2, 3, 4, 14, 25, 0]] = 1.0 / 7

    def of(lo, hi):
        only = np.zeros(29, np.float32)
        only[lo:hi] = p[lo:hi]
        return _d(np.cumsum(only, dtype=np.float32), device)
    return [of(14, 29), of(1, 14), of(0, 1)]


def _point(f, s, p, device):
    fd, out = _f(f, device), ()
    for mode in range(4):
        out += _o(hip.point_mutate(mode, 0.7, 0.1, False, s["out_len"] > 1, False, 2, s["var_len"], s["out_len"], s["seed"], 8 + mode, *fd,
                                   *_roulettes(device), _d(np.array([-1.0, 0.0, 1.0], np.float32), device)))
    return out


MSE, HUBER = (0, 0.0), (2, 1.0)
H = "include/evogp_hip.h"


def _malformed_rows(f_in, out):
    """tree_prune: the rows the header has 'copied as it is' (the rule of tests/subtree_ref.py, which the kernel's classify_tree follows)"""
    from subtree_ref import well_formed
    n = live_len(f_in[2])
    return np.array([not well_formed(f_in[1][t], int(n[t])) for t in range(len(n))])


def _unwrapped_rows(f_in, out):
    """tree_wrap_linear: the rows the header has 'copied unchanged', applied[t] = 0"""
    return out[3] == 0


def _row(call, cls="per-tree", out="single", data=True, cpu=None, axes=None, finite=None, select=_select_rows, tails=None, cite=None, copied=None):
    """out: which cases fit ('single': out_len 1, 'multi': out_len > 1, 'any'); data: the op reads the dataset (else the first and third
    case only); cpu: the modules whose register() gives the op a CPU stand-in; axes: the tree axis of every output (default 0); finite:
    the float per-tree output of which pop // 4 trees must be finite; tails: for a rewriter, {output index: 'zero' | 'input'} with the
    lines of the header that say so in `cite`; copied: (input forest, outputs) -> the rows the header has the op copy 'as it is', whose
    dead words are therefore the input row's where every other output row ends in zeros"""
    return dict(call=call, cls=cls, out=out, data=data, cpu=cpu, axes=axes, finite=finite, select=select, tails=tails, cite=cite, copied=copied)


ZERO3 = {0: "zero", 1: "zero", 2: "zero"}
TABLE = {
    # ---- per-tree ----
    "evogp_cuda::tree_SR_fitness": _row(_sr_fitness, out="any", cpu=("cpu_ops",), finite=0),
    "evogp_hip::tree_SR_fitness_masked": _row(_sr_fitness_masked, out="any", finite=0),
    "evogp_cuda::tree_evaluate": _row(_evaluate, out="any", cpu=("cpu_ops",), finite=0),
    "evogp_hip::tree_batch_evaluate": _row(_data_op(hip.tree_batch_evaluate, y=None), out="any", cpu=("cpu_ops",), finite=0),
    "evogp_hip::tree_batch_argmax_count": _row(_data_op(hip.tree_batch_argmax_count, y="cls"), out="multi"),
    "evogp_hip::tree_evaluate_prepare": _row(_prepared, out="multi", finite=0),
    "evogp_hip::tree_evaluate_prepared": _row(_prepared, out="multi", finite=0),
    "evogp_hip::tree_SR_gradient": _row(_data_op(hip.tree_SR_gradient, mse=True), out="any", cpu=("cpu_grad_ops",), finite=0),
    "evogp_hip::tree_SR_weighted_gradient": _row(_weighted_row(hip.tree_SR_weighted_gradient, (MSE, HUBER)), cpu=("cpu_wgrad_ops",), finite=0),
    "evogp_hip::tree_SR_normal_eq": _row(_data_op(hip.tree_SR_normal_eq), cpu=("cpu_lm_ops",), finite=0),
    "evogp_hip::tree_SR_weighted_normal_eq": _row(_weighted_row(hip.tree_SR_weighted_normal_eq, ((),)), cpu=("cpu_wgrad_ops",), finite=0),
    "evogp_hip::tree_SR_case_errors": _row(_data_op(hip.tree_SR_case_errors, mse=True), out="any", cpu=("cpu_lexicase_ops",), axes=(1,)),
    "evogp_hip::tree_SR_subtree_errors": _row(_data_op(hip.tree_SR_subtree_errors, mse=True), cpu=("cpu_subtree_ops",)),
    "evogp_hip::tree_SR_linear_scaling": _row(_data_op(hip.tree_SR_linear_scaling), cpu=("cpu_scale_ops",), finite=0),
    "evogp_hip::tree_SR_weighted_loss": _row(_weighted(hip.tree_SR_weighted_loss, (MSE, HUBER)), cpu=("cpu_wloss_ops",), finite=0),
    "evogp_hip::tree_SR_weighted_scaling": _row(_weighted(hip.tree_SR_weighted_scaling, ((),)), cpu=("cpu_wscale_ops",), finite=0),
    "evogp_hip::tree_SR_gene_fitness": _row(_data_op(hip.tree_SR_gene_fitness, y="y1"), out="any", cpu=("cpu_gene_ops",), finite=0),
    "evogp_hip::tree_SR_gene_moments": _row(_data_op(hip.tree_SR_gene_moments, y="y1"), out="any", cpu=("cpu_gene_ops",), finite=0),
    "evogp_hip::tree_SR_semantic_hash": _row(_data_op(hip.tree_SR_semantic_hash, y=None), cpu=("cpu_semantic_ops",)),
    "evogp_hip::tree_hash": _row(_plain(hip.tree_hash), out="any", data=False, cpu=("cpu_dedup_ops",)),
    "evogp_hip::tree_intervals": _row(_plain(hip.tree_intervals, "lower", "upper"), data=False, cpu=("cpu_interval_ops",)),
    "evogp_hip::tree_derivative_intervals": _row(_plain(hip.tree_derivative_intervals, "lower", "upper", "wrt"), data=False,
                                                 cpu=("cpu_derivative_ops",), axes=(0, 0, 0, 1, 1, 1)),
    "evogp_hip::tree_dimensions": _row(_plain(hip.tree_dimensions, "var_units", "label_units", tail=(True,)), data=False, cpu=("cpu_dimension_ops",)),
    "evogp_hip::tree_structure": _row(_plain(hip.tree_structure, "cost", "operand_limit", "rule_outer", "rule_inner", "rule_limit", tail=(6, 40)),
                                      data=False, cpu=("cpu_structure_ops",)),
    # ---- rewriters, deterministic ----
    "evogp_hip::tree_prune": _row(_prune, "rewriter", data=False, cpu=("cpu_subtree_ops",), tails=ZERO3,
                                  copied=_malformed_rows, cite=H + ": evogp_hip_prune_rows, '[new_len, gp_len) is zero in all three arrays'; "
                                  "'A malformed tree's row is copied as it is'"),
    "evogp_hip::tree_wrap_linear": _row(_wrap, "rewriter", data=False, cpu=("cpu_scale_ops",), tails=ZERO3,
                                        copied=_unwrapped_rows, cite=H + ": evogp_hip_wrap_linear, 'zero tail words'; a row that is not "
                                        "wrapped 'is copied unchanged (tail words beyond gp_len zero)'"),
    "evogp_hip::tree_SR_const_step": _row(_const_step, "rewriter", out="any", data=False, cpu=("cpu_grad_ops",), tails={0: "input", 1: "input"},
                                          cite=H + ": evogp_hip_sr_const_step, 'Neither type nor size nor any non-constant word of value is "
                                          "written'; value_cand row = value row"),
    "evogp_hip::tree_SR_lm_step": _row(_lm_step, "rewriter", data=False, cpu=("cpu_lm_ops",), tails={0: "input", 1: "input"},
                                       cite=H + ": evogp_hip_sr_lm_step, 'Neither type nor size nor any other word of value is written; every "
                                       "word of the value_cand row is' (the value row's)"),
    "evogp_cuda::tree_mutate": _row(_mutate, "rewriter", out="any", data=False, cpu=("cpu_ops",), tails=ZERO3,
                                    cite=H + ": head comment, 'Output rows are written on [0, len) and zero-filled on [len, gp_len)'"),
    "evogp_cuda::tree_crossover": _row(_crossover, "rewriter", out="any", data=False, cpu=("cpu_ops",), tails=ZERO3, select=_select_pairs,
                                       cite=H + ": head comment, 'Output rows are written on [0, len) and zero-filled on [len, gp_len)'"),
    "evogp_hip::breed_rows": _row(_breed_rows, "rewriter", out="any", data=False, tails=ZERO3, select=_select_lists,
                                  cite=H + ": head comment (zero-filled output rows); evogp_hip_breed_lists"),
    # ---- rewriters whose draws are counter-based words keyed by the row index: invariant A only ----
    "evogp_hip::breed_default": _row(_breed_default, "counter", out="any", data=False, tails=ZERO3, cite=H + ": head comment (zero-filled output rows)"),
    "evogp_hip::breed_default_rows": _row(_breed_default_rows, "counter", out="any", data=False, tails=ZERO3,
                                          cite=H + ": head comment (zero-filled output rows)"),
    "evogp_hip::breed_rows_hashed": _row(_breed_rows_hashed, "counter", out="any", data=False, tails=ZERO3,
                                         cite=H + ": head comment (zero-filled output rows)"),
    "evogp_hip::structural_mutate": _row(_structural, "counter", out="any", data=False, tails={0: "zero", 1: "zero", 2: "zero", 4: "zero", 5: "zero", 6: "zero"},
                                         cite=H + ": head comment (zero-filled output rows); evogp_hip_structural_mutate"),
    "evogp_hip::insert_mutate": _row(_insert, "counter", out="any", data=False, tails=ZERO3,
                                     cite=H + ": head comment (zero-filled output rows); evogp_hip_insert_mutate"),
    "evogp_hip::point_mutate": _row(_point, "counter", out="any", data=False, tails={0: "input", 1: "input", 2: "input", 3: "input"},
                                    cite=H + ": evogp_hip_point_mutate, 'only the value array changes'"),
    # ---- class ops: A is whole-output equality, B equality of the partition, C does not apply ----
    "evogp_hip::tree_classes": _row(_classes, "classes", out="any", data=False, cpu=("cpu_dedup_ops",)),
    "evogp_hip::tree_SR_semantic_classes": _row(_semantic_classes, "classes", cpu=("cpu_semantic_ops",)),
}

EXEMPT = {op: "takes no forest: " + why for op, why in {
    "evogp_cuda::tree_generate": "it writes one", "evogp_hip::tree_generate_offset": "it writes one",
    "evogp_hip::tree_generate_masked": "it writes one", "evogp_hip::tree_generate_masked_hashed": "it writes one",
    "evogp_hip::random_words": "counter-based words", "evogp_hip::fitness_scores": "a vector of errors",
    "evogp_hip::select_survivors": "a fitness vector", "evogp_hip::tournament_select": "a fitness vector",
    "evogp_hip::lexicase_select": "case-major errors", "evogp_hip::pareto_rank": "two objective vectors",
    "evogp_hip::nsga2_select": "an order of rows"}.items()}


def cases_for(op):
    row = TABLE[op]
    names = list(CASES) if row["data"] else [n for n in CASES if n in NO_DATA_CASES or (row["out"] == "multi" and CASES[n]["out_len"] > 1)]
    keep = {"single": lambda o: o == 1, "multi": lambda o: o > 1, "any": lambda o: True}[row["out"]]
    return [n for n in names if keep(CASES[n]["out_len"])]


# ---- the checker ----------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return fbits(a)
    if a.dtype == np.float64:
        u = a.view(np.uint64).copy()
        u[np.isnan(a)] = 0x7FF8000000000000
        return u
    return a


def _take(a, sel, axis):
    return a if sel is None else np.take(a, sel, axis=axis)


def _fail(op, inv, k, axis, got, want, trees, planted, what=""):
    """AssertionError naming the op, the invariant, the tree, its planted pattern and the first differing words"""
    diff = np.argwhere(_bits(got) != _bits(want))
    at = tuple(diff[0])
    t = int(at[axis]) if got.ndim else 0
    tree = int(trees[t]) if trees is not None and t < len(trees) else t
    pat = [n for n, r in (planted or {}).items() if r == tree]
    words = ", ".join(f"{tuple(int(i) for i in d)}: {got[tuple(d)]!r} != {want[tuple(d)]!r}" for d in diff[:4])
    raise AssertionError(f"{op}: invariant {inv}{what}: output {k} differs at tree {tree}" + (f" (planted: {', '.join(pat)})" if pat else "")
                         + f"; {len(diff)} words differ, first {words}")


def _compare(op, inv, got, want, axes, trees, planted, what=""):
    assert len(got) == len(want), f"{op}: invariant {inv}{what}: {len(got)} outputs against {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{op}: invariant {inv}{what}: output {k} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        if not np.array_equal(_bits(g), _bits(w)):
            _fail(op, inv, k, axes[k], g, w, trees, planted, what)


def _partition(ids, trees):
    """class ids over the rows of a selection -> per tree, the smallest TREE index of its class"""
    canon = np.empty(len(ids), np.int64)
    first = {}
    for k in np.argsort(trees, kind="stable"):
        first.setdefault(int(ids[k]), int(trees[k]))
    for k in range(len(ids)):
        canon[trees[k]] = first[int(ids[k])]
    return canon


def _copied_dead(row, f_in, out):
    """bool[pop][L of the outputs]: the dead words of the rows the op copies as they are (their length is the input row's)"""
    Lout = out[0].shape[1]
    m = np.zeros((f_in[0].shape[0], Lout), bool)
    if row.get("copied") is not None:
        L = f_in[0].shape[1]
        m[:, :L] = dead_mask(f_in[2]) & np.asarray(row["copied"](f_in, out), bool)[:, None]
    return m


def _check_tails(op, row, f_in, out, planted):
    """invariant A for a rewriter: the dead words of an output row"""
    for k, rule in row["tails"].items():
        if rule == "zero":
            base = 4 * (k // 4)   # (the triple this output belongs to: outputs come as value, type, size[, more])
            if row.get("copied") is None:   # every output row is written in full
                dead = dead_mask(out[base + 2])
                bad = np.argwhere(dead & (_bits(out[k]) != 0))
                assert not len(bad), (f"{op}: invariant A (dead words of an output row, zero by {row['cite']}): output {k} holds "
                                      f"{out[k][tuple(bad[0])]!r} at tree {bad[0][0]} word {bad[0][1]}, behind its length {out[base + 2][bad[0][0], 0]}")
                continue
            asis = _copied_dead(row, f_in, out)
            copied_rows = np.asarray(row["copied"](f_in, out), bool)
            dead = dead_mask(out[base + 2]) & ~copied_rows[:, None]
            bad = np.argwhere(dead & (_bits(out[k]) != 0))
            assert not len(bad), (f"{op}: invariant A (dead words of an output row, zero by {row['cite']}): output {k} holds {out[k][tuple(bad[0])]!r} "
                                  f"at tree {bad[0][0]} word {bad[0][1]}, behind its length {out[base + 2][bad[0][0], 0]}")
            L = f_in[0].shape[1]
            want = np.zeros_like(out[k])
            want[:, :L] = f_in[k - base]
            bad = np.argwhere(asis & (_bits(out[k]) != _bits(want)))
            assert not len(bad), (f"{op}: invariant A (a row copied as it is, {row['cite']}): output {k} holds {out[k][tuple(bad[0])]!r} at tree "
                                  f"{bad[0][0]} word {bad[0][1]}, the input row {want[tuple(bad[0])]!r}")
            beyond = copied_rows[:, None] & (np.arange(out[k].shape[1])[None, :] >= L)
            assert not (_bits(out[k])[beyond] != 0).any(), f"{op}: invariant A: output {k} of a copied row is not zero beyond the input's gp_len"
        else:
            dead = dead_mask(f_in[2])
            bad = np.argwhere(dead & (_bits(out[k]) != _bits(f_in[0])))
            assert not len(bad), (f"{op}: invariant A (dead words are the input row's by {row['cite']}): output {k} holds {out[k][tuple(bad[0])]!r} "
                                  f"at tree {bad[0][0]} word {bad[0][1]}, the input {f_in[0][tuple(bad[0])]!r}")


def check(op, row, case, device, invariants="ABC"):
    """asserts the invariants of the row's class on the case; raises an AssertionError that names op, invariant, tree, planted pattern and
    the first differing words"""
    call, select, cls = row["call"], row["select"], row["cls"]
    f, fs, s, planted = case.forest, case.stale, case.shared, case.planted
    pop, L = f[0].shape
    everything = np.arange(pop)
    # non-vacuity of the case
    n = live_len(f[2])
    room = n < L
    changed = np.array([any(not np.array_equal(_bits(a[t]), _bits(b[t])) for a, b in zip(f, fs)) for t in range(pop)])
    assert changed[room].mean() >= 0.9, f"{case.name}: only {changed[room].mean():.0%} of the rows with n < L carry a changed dead word"
    assert not changed[~room].any(), f"{case.name}: a row without a tail was changed"
    for a, b in zip(f, fs):
        assert np.array_equal(_bits(a)[~dead_mask(f[2])], _bits(b)[~dead_mask(f[2])]), f"{case.name}: a live word was changed"
    want_patterns = set(_patterns(L, case.out_len))
    assert set(planted) == want_patterns, f"{case.name}: planted patterns missing: {sorted(want_patterns - set(planted))}"

    pf, _, _ = select(f, case.per_tree, everything)
    base = call(f, s, pf, device)
    axes = row["axes"] or (0,) * len(base)
    if row["finite"] is not None and cls == "per-tree":
        o = base[row["finite"]]
        fin = np.isfinite(o.reshape(pop, -1) if axes[row["finite"]] == 0 else np.moveaxis(o, axes[row["finite"]], 0).reshape(pop, -1)).all(1)
        assert fin.sum() >= pop // 4, f"{op} on {case.name}: only {fin.sum()} of {pop} trees are finite in the baseline call"

    if "A" in invariants:
        got = call(fs, s, pf, device)
        if row["tails"] is None:
            _compare(op, "A (dead words)", got, base, axes, everything, planted)
        else:
            live = ~dead_mask(f[2])
            for k, (g, w) in enumerate(zip(got, base)):
                assert g.shape == w.shape and g.dtype == w.dtype
                if row["tails"].get(k) == "input":   # the live prefixes are equal, the dead words each call's own input's
                    g, w = np.where(live, g, 0), np.where(live, w, 0)
                elif row["tails"].get(k) == "zero" and row["copied"] is not None:   # ... and so are those of a row copied as it is
                    ga, wa = _copied_dead(row, fs, got), _copied_dead(row, f, base)
                    assert np.array_equal(ga, wa), f"{op}: invariant A (dead words): the two calls copy different rows as they are"
                    g, w = np.where(ga, 0, g), np.where(wa, 0, w)
                if not np.array_equal(_bits(g), _bits(w)):
                    _fail(op, "A (dead words)", k, axes[k], g, w, everything, planted)
            _check_tails(op, row, fs, got, planted)
            _check_tails(op, row, f, base, planted)
    if cls == "counter":
        return
    # B and C run on the forest with the stale tails: a neighbour's dead words are part of what a tree must not depend on
    whole = call(fs, s, pf, device) if "B" in invariants or "C" in invariants else None
    sels = []
    if "B" in invariants:
        import zlib
        prng = np.random.default_rng([7, zlib.crc32(op.encode()), pop])
        sels += [("B (row order)", f" under the permutation starting {perm[:4].tolist()}", perm) for perm in permute(prng, pop)]
    if "C" in invariants and cls != "classes":
        sels += [("C (slices)", f" on the slice [{a}:{b}]", np.arange(a, b)) for a, b in slices(pop)]
    for inv, what, sel in sels:
        p_full, p_sel, out_sel = select(fs, case.per_tree, sel)
        full = whole if p_full is pf else call(fs, s, p_full, device)
        got = call(tuple(a[sel] for a in fs), s, p_sel, device)
        if cls == "classes":
            g, w = _partition(got[0], sel), _partition(full[0], everything)
            if not np.array_equal(g, w):
                t = int(np.flatnonzero(g != w)[0])
                raise AssertionError(f"{op}: invariant {inv}{what}: tree {t} is in the class of tree {g[t]}, in the original order of tree {w[t]}")
            continue
        want = tuple(_take(o, out_sel, ax) for o, ax in zip(full, axes))
        _compare(op, inv, got, want, axes, out_sel, planted, what)
