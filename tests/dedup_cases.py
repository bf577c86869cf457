"""TEST-ONLY: forests with planted structural duplicates and near-duplicates for the tests of csrc/dedup.hip (tests/test_dedup_ref.py,
tests/test_dedup_host.py, tests/test_gpu_dedup.py)."""
import numpy as np

import sr_grad_ref as R
from grad_trees import ALL_FUNCS, ARITH, random_forest


def comb(n_consts, gp_len, rng, unary_root=False):
    """c + (c + (... + c)) with random constants, 2 n_consts - 1 nodes; ``unary_root`` puts a sin on top (one node more)"""
    value, type_, size = np.zeros(gp_len, np.float32), np.zeros(gp_len, np.int16), np.zeros(gp_len, np.int16)
    n = 2 * n_consts - 1
    o = 1 if unary_root else 0
    if unary_root:
        value[0], type_[0], size[0] = R.F_SIN, R.T_UFUNC, n + 1
    for k in range(n_consts - 1):
        value[o + 2 * k], type_[o + 2 * k], size[o + 2 * k] = R.F_ADD, R.T_BFUNC, n - 2 * k
        value[o + 2 * k + 1], type_[o + 2 * k + 1], size[o + 2 * k + 1] = rng.uniform(0.5, 1.5), R.T_CONST, 1
    value[o + n - 1], type_[o + n - 1], size[o + n - 1] = rng.uniform(0.5, 1.5), R.T_CONST, 1
    return value, type_, size


def _set(value, type_, size, t, nodes):
    for i, (v, ty, s) in enumerate(nodes):
        value[t, i], type_[t, i], size[t, i] = v, ty, s


def garbage_tails(rng, value, type_, size):
    """random words behind every live prefix (no row may depend on them)"""
    pop, L = value.shape
    n = np.clip(size[:, :1].astype(np.int64), 0, L)
    tail = np.arange(L)[None, :] >= n
    tail[:, 0] = False   # (position 0 holds n itself, also for an out-of-range row)
    value[tail] = rng.uniform(-4, 4, int(tail.sum())).astype(np.float32)
    type_[tail] = rng.integers(0, 6, int(tail.sum())).astype(np.int16)
    size[tail] = rng.integers(-3, L, int(tail.sum())).astype(np.int16)


def planted_forest(rng, pop, gp_len):
    """(value, type, size): half the rows single-output arithmetic trees, half trees over all 29 functions with multi-output (out_len 2)
    type words; at gp_len > 64 also combs longer than 64 nodes and one row with n == gp_len; garbage tails everywhere.  From 63 rows on:
      rows 10, 40, pop - 20, pop - 1   copies of row 3 (same class, own tails)
      rows 20 / 21   differ in tail words only (same class)           rows 22 / 23   differ in the sign of a zero constant
      rows 24 / 25   differ in the OUT flag of one type word          rows 26 / 27   differ in n only
      rows 28 / 29   differ in one size word inside the prefix        rows 30, 31, 32, 33   n = 0, -1, gp_len + 1, 0: singletons"""
    half = pop // 2
    a = random_forest(rng, pop - half, gp_len, ARITH, 3, 1, max_depth=4)
    if half:
        b = random_forest(rng, half, gp_len, ALL_FUNCS, 3, 2, max_depth=4)
        value, type_, size = (np.concatenate([x, y]) for x, y in zip(a, b))
        order = rng.permutation(pop)
        value, type_, size = value[order], type_[order], size[order]
    else:
        value, type_, size = a
    if gp_len > 64 and pop >= 63:
        for t in range(41, 61, 3):
            value[t], type_[t], size[t] = comb(int(rng.integers(33, gp_len // 2)), gp_len, rng)
        value[44], type_[44], size[44] = value[41], type_[41], size[41]          # a long duplicate ...
        value[47], type_[47], size[47] = value[41].copy(), type_[41], size[41]   # ... and a long row that differs in its last word
        value[47, size[41, 0] - 1] += 1.0
    if pop >= 63:
        value[50], type_[50], size[50] = comb(gp_len // 2, gp_len, rng, unary_root=True)   # n == gp_len
        value[53], type_[53], size[53] = value[50], type_[50], size[50]
        value[20] = value[21]; type_[20] = type_[21]; size[20] = size[21]
        _set(value, type_, size, 22, [(R.F_ADD, R.T_BFUNC, 3), (0.0, R.T_CONST, 1), (0, R.T_VAR, 1)])
        _set(value, type_, size, 23, [(R.F_ADD, R.T_BFUNC, 3), (-0.0, R.T_CONST, 1), (0, R.T_VAR, 1)])
        _set(value, type_, size, 24, [(R.F_MUL, R.T_BFUNC, 3), (0, R.T_VAR, 1), (1, R.T_VAR, 1)])
        _set(value, type_, size, 25, [(R.F_MUL, R.T_BFUNC | 0x80, 3), (0, R.T_VAR, 1), (1, R.T_VAR, 1)])
        five = [(R.F_SUB, R.T_BFUNC, 5), (R.F_ADD, R.T_BFUNC, 3), (0, R.T_VAR, 1), (1, R.T_VAR, 1), (2.0, R.T_CONST, 1)]
        for t in (26, 27, 28, 29):
            _set(value, type_, size, t, five)
        size[27, 0] = 4
        size[29, 1] = 2
        for t, n in ((30, 0), (31, -1), (32, gp_len + 1), (33, 0)):
            size[t, 0] = n
    garbage_tails(rng, value, type_, size)
    if pop >= 63:
        for t in (10, 40, pop - 20, pop - 1):
            n = int(size[3, 0])
            value[t, :n], type_[t, :n], size[t, :n] = value[3, :n], type_[3, :n], size[3, :n]
            if t not in (10, 40):   # (rows 10 and 40 keep their own tails; the two last ones get fresh ones)
                value[t, n:] = rng.uniform(-4, 4, gp_len - n).astype(np.float32)
        value[27, 1:], type_[27, 1:], size[27, 1:] = value[26, 1:], type_[26, 1:], size[26, 1:]   # only n differs
        value[33], type_[33], size[33] = value[30], type_[30], size[30]                           # whole-row copy of an n = 0 row
    return value, type_, size


def half_copies(rng, pop, gp_len, max_depth=4):
    """single-output arithmetic forest whose second half are shuffled copies of the first half's live prefixes with tails of their own;
    row 1 is an empty tree (n = 0), row 2 a malformed in-range row (an operator without operands), and both have copies"""
    half = pop // 2
    value, type_, size = random_forest(rng, pop, gp_len, ARITH, 3, 1, max_depth=max_depth)
    if gp_len > 64:
        value[5], type_[5], size[5] = comb(60, gp_len, rng)
        value[6], type_[6], size[6] = comb(gp_len // 2, gp_len, rng, unary_root=True)
    size[1, 0] = 0
    _set(value, type_, size, 2, [(R.F_ADD, R.T_BFUNC, 2), (0, R.T_VAR, 1)])
    garbage_tails(rng, value, type_, size)
    src = rng.permutation(half)
    for k in range(half):
        t, u = half + k, int(src[k])
        n = max(int(size[u, 0]), 1)   # (position 0 always: it carries n)
        value[t, :n], type_[t, :n], size[t, :n] = value[u, :n], type_[u, :n], size[u, :n]
    return value, type_, size
