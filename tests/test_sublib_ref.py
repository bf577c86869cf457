"""CPU: the numpy restatement of the per-subtree signatures and of the library's choice (tests/sublib_ref.py) on hand-built forests:
which subtrees are one class, who represents a class, how the classes are ordered, what the size window and k do, and what is never
eligible."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semantic_ref as S  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import sublib_ref as SL  # noqa: E402

B, V, C = R.T_BFUNC, R.T_VAR, R.T_CONST
L = 8


def x(i):
    return [(float(i), V, 1)]


def c(v):
    return [(float(v), C, 1)]


def op(f, a, b):
    return [(float(f), B, 1 + len(a) + len(b))] + a + b


def forest(*trees):
    value, type_, size = np.zeros((len(trees), L), np.float32), np.zeros((len(trees), L), np.int16), np.zeros((len(trees), L), np.int16)
    for t, nodes in enumerate(trees):
        for i, (v, ty, s) in enumerate(nodes):
            value[t, i], type_[t, i], size[t, i] = v, ty, s
    return value, type_, size


@pytest.fixture(scope="module")
def X():
    return np.random.default_rng(5).uniform(0.5, 1.5, (37, 2)).astype(np.float32)


def sigs(oracle, f, X):
    return SL.forest_signatures(oracle, *f, X)


def test_signatures_are_the_tree_signature_of_the_extracted_row(oracle, X):
    f = forest(op(R.F_MUL, op(R.F_ADD, x(0), x(1)), c(2.0)), x(1), op(R.F_SUB, x(0), c(0.25)))
    sig = sigs(oracle, f, X)
    P, formed = S.oracle_predictions(oracle, *f, X)
    assert formed.all() and np.array_equal(sig[:, 0], S.signature(P, formed))
    live = np.arange(L)[None, :] < f[2][:, :1]
    assert (sig[live] != 0).all() and (sig[~live] == 0).all()
    assert sig[0, 2] == sig[2, 1] and sig[0, 3] == sig[1, 0] and sig[0, 1] != sig[0, 0]   # x0 twice, x1 twice


def test_identities_and_commuted_operands_are_one_class(oracle, X):
    f = forest(op(R.F_MUL, x(0), c(1.0)), op(R.F_ADD, x(0), c(0.0)), op(R.F_ADD, x(0), x(1)), op(R.F_ADD, x(1), x(0)), x(0))
    sig = sigs(oracle, f, X)
    assert sig[0, 0] == sig[1, 0] == sig[4, 0] == sig[0, 1] == sig[1, 1]
    assert sig[2, 0] == sig[3, 0] != sig[0, 0]
    member, count, n = SL.select(sig, f[2], 1, L, 16)
    # classes: x0 (t0 n0, t0 n1, t1 n0, t1 n1, t2 n1, t3 n2, t4 n0: 7), x1 (t2 n2, t3 n1: 2), x0 + x1 (2), the constants 1 and 0 (1 each)
    assert n == 5 and count[:5].tolist() == [7, 2, 2, 1, 1]
    assert member[0] == 0 * L + 1, "the lone leaf of smallest flat index represents the class of x0, not the three-node tree at index 0"
    assert member[1:3].tolist() == [2 * L + 0, 2 * L + 2], "a tie in count is broken by the representative's flat index"
    assert member[3:5].tolist() == [0 * L + 2, 1 * L + 2] and (member[5:] == -1).all() and not count[5:].any()


def test_all_nan_subtrees_are_one_class(oracle, X):
    f = forest(op(R.F_DIV, x(0), c(0.0)), op(R.F_DIV, x(1), c(0.0)), op(R.F_ADD, x(1), op(R.F_DIV, x(0), c(0.0))))
    sig = sigs(oracle, f, X)
    assert sig[0, 0] == sig[1, 0] == sig[2, 0] == sig[2, 2] != 0
    member, count, n = SL.select(sig, f[2], 2, L, 4)
    assert n == 1 and member[0] == 0 and count[0] == 4


def test_the_size_window(oracle, X):
    f = forest(op(R.F_MUL, op(R.F_ADD, x(0), x(1)), c(2.0)), op(R.F_ADD, x(0), x(1)))
    sig = sigs(oracle, f, X)
    member, count, n = SL.select(sig, f[2], 2, L, 8)          # min_size 2 drops the leaves
    assert n == 2 and member[:2].tolist() == [1, 0] and count[:2].tolist() == [2, 1]
    member, count, n = SL.select(sig, f[2], 1, 3, 8)          # max_size 3 drops the five-node root
    assert n == 4 and 0 not in member.tolist() and member[0] == 1 and count[0] == 2   # x0 + x1: the first of its class (size 3 both)
    member, count, n = SL.select(sig, f[2], 1, 1, 8)
    assert n == 3 and sorted(member[:3].tolist()) == [2, 3, 4] and (f[2].reshape(-1)[member[:3]] == 1).all()


def test_k_truncates_and_fills(oracle, X):
    f = forest(op(R.F_ADD, x(0), x(1)), x(0))
    sig = sigs(oracle, f, X)
    member, count, n = SL.select(sig, f[2], 1, L, 1)
    assert n == 3 and member.tolist() == [1] and count.tolist() == [2]
    member, count, n = SL.select(sig, f[2], 1, L, 6)
    assert n == 3 and member.tolist() == [1, 0, 2, -1, -1, -1] and count.tolist() == [2, 1, 1, 0, 0, 0]


def test_malformed_rows_and_a_planted_zero(oracle, X):
    bad = forest(c(1.0) * 3, x(0), [(float(R.F_ADD), B, 1)])
    bad[2][0, 0], bad[2][1, 0] = 3, 0     # three leaves under n = 3; an empty row; a root without operands
    sig = sigs(oracle, bad, X)
    assert not sig.any()
    member, count, n = SL.select(sig, bad[2], 1, L, 4)
    assert n == 0 and (member == -1).all() and not count.any()
    f = forest(op(R.F_ADD, x(0), x(1)), x(0))
    sig = sigs(oracle, f, X)
    sig[0, 1] = 0                         # a live subtree whose signature is exactly 0 is dropped
    member, count, n = SL.select(sig, f[2], 1, L, 4)
    assert n == 3 and member[:3].tolist() == [0, 2, L] and count[:3].tolist() == [1, 1, 1]


def test_extraction_copies_the_nodes_verbatim(oracle, X):
    f = forest(op(R.F_MUL, op(R.F_ADD, x(0), x(1)), c(2.0)), x(1))
    (v, t, s), tree, node = SL.extract(*f, np.array([1, L, 4, -1, -1], np.int32))
    assert tree.tolist() == [0, 1, 0] and node.tolist() == [1, 0, 4]
    assert s[:, 0].tolist() == [3, 1, 1] and t[0, :4].tolist() == [B, V, V, 0] and v[0, :3].tolist() == [float(R.F_ADD), 0.0, 1.0]
    assert v[2, 0] == 2.0 and t[2, 0] == C and not v[:, 3:].any() and not s[:, 3:].any()
    sig = sigs(oracle, f, X)
    assert np.array_equal(sigs(oracle, (v, t, s), X)[:, 0], sig.reshape(-1)[[1, L, 4]])
