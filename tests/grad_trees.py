"""TEST-ONLY: random prefix-order trees over a chosen function set (single- or multi-output), as raw (value, type, size) rows, for
the constant-gradient tests (tests/test_sr_grad_*.py)."""
import numpy as np

import sr_grad_ref as R

UNARY = list(range(R.F_SIN, R.F_LOOSE_SQRT + 1))
BINARY = list(range(R.F_ADD, R.F_GE + 1))
ALL_FUNCS = [R.F_IF] + BINARY + UNARY
ARITH = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV]


def out_word(f, o):
    """the value word of a function node with the OUT flag: function id in the low 16 bits, output index in the high 16"""
    return np.uint32((f & 0xFFFF) | (o << 16)).view(np.float32)


def random_tree(rng, funcs, var_len, out_len, max_depth, const_range=(0.5, 1.5), out_prob=0.5):
    nodes = []

    def gen(depth):
        if depth >= max_depth or rng.random() < 0.25:
            if rng.random() < 0.5:
                nodes.append([np.float32(rng.uniform(*const_range)), R.T_CONST, 1])
            else:
                nodes.append([np.float32(rng.integers(var_len)), R.T_VAR, 1])
            return 1
        f = int(rng.choice(funcs))
        typ = R.T_UFUNC if f >= R.F_SIN else R.T_BFUNC if f >= R.F_ADD else 4
        me = len(nodes)
        nodes.append([np.float32(f), typ, 0])
        if out_len > 1 and rng.random() < out_prob:
            nodes[me][0] = out_word(f, int(rng.integers(out_len)))
            nodes[me][1] = typ | 0x80
        n = 1
        for _ in range({R.T_UFUNC: 1, R.T_BFUNC: 2}.get(typ, 3)):
            n += gen(depth + 1)
        nodes[me][2] = n
        return n

    gen(0)
    return nodes


def random_forest(rng, pop, gp_len, funcs, var_len, out_len, max_depth, **kw):
    value = np.zeros((pop, gp_len), np.float32)
    type_ = np.zeros((pop, gp_len), np.int16)
    size = np.zeros((pop, gp_len), np.int16)
    for t in range(pop):
        while True:
            nodes = random_tree(rng, funcs, var_len, out_len, max_depth, **kw)
            if len(nodes) <= gp_len:
                break
        for i, (v, ty, s) in enumerate(nodes):
            value[t, i], type_[t, i], size[t, i] = v, ty, s
    return value, type_, size
