"""CPU: the numpy twin of epsilon-lexicase selection (tests/lexicase_ref.py) -- its permutation and words against the engine's
counter words, lexicase_epsilon in torch against it bit for bit, and the properties the operator must have."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lexicase_ref as R  # noqa: E402

from evogp_amd.algorithm import lexicase_epsilon  # noqa: E402
from evogp_amd.algorithm.selection import LEXICASE_ROW_SAMPLE, _counter_row  # noqa: E402
from evogp_amd.parallel import random_words  # noqa: E402


@pytest.mark.parametrize("n", [1, 2, 3, 4, 1000, 1024, 1025, 5000])
def test_perm_is_a_bijection(n):
    for k in (0, 1, 7, 123456):
        p = R.perm(99, 3, k, n)
        assert sorted(p.tolist()) == list(range(n))
        # position by position gives the same numbers
        pos = np.array([0, n // 2, n - 1])
        assert np.array_equal(R.perm(99, 3, k, n, positions=pos), p[pos])
    if n >= 1000:   # different events, different orders
        assert not np.array_equal(R.perm(99, 3, 0, n), R.perm(99, 3, 1, n))


def test_twin_words_equal_random_words():
    for seed, gen in ((0, 0), (12345, 7), (2**40 - 1, 99)):
        for row in (R.ROW_FEISTEL, R.ROW_PICK, R.ROW_SAMPLE, 16):
            want = random_words(seed, gen, 1, 0, 300, "cpu", first_row=row)[0].numpy()
            assert np.array_equal(R.counter_words(seed, gen, row, np.arange(300)).astype(np.int64), want)
        got = _counter_row(seed, gen, LEXICASE_ROW_SAMPLE, 300, "cpu").numpy()
        assert np.array_equal(got, random_words(seed, gen, 1, 0, 300, "cpu", first_row=LEXICASE_ROW_SAMPLE)[0].numpy())


def test_epsilon_torch_equals_twin(rng):
    inf, nan = float("inf"), float("nan")
    for pop, n in ((1, 3), (2, 5), (7, 4), (64, 33), (501, 17)):
        e = rng.exponential(1.0, (pop, n)).astype(np.float32)
        e[rng.random((pop, n)) < 0.1] = nan
        e[rng.random((pop, n)) < 0.05] = inf
        e[rng.random((pop, n)) < 0.05] = -inf
        e[:, 0] = nan                          # a case without a finite error
        if n > 2:
            e[:, 1] = rng.integers(0, 3, pop)  # ties
        got = lexicase_epsilon(torch.from_numpy(e)).numpy()
        want = R.epsilon(e)
        assert got.dtype == np.float32 and got.shape == (n,)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (got, want)
        # any strides: the transposed view of case-major storage
        t = torch.from_numpy(np.ascontiguousarray(e.T)).t()
        assert np.array_equal(lexicase_epsilon(t).numpy().view(np.uint32), want.view(np.uint32))
    assert lexicase_epsilon(torch.full((6, 2), nan)).tolist() == [0.0, 0.0]


def test_best_on_every_case_always_wins(rng):
    E = rng.uniform(1, 2, (12, 40)).astype(np.float32)
    E[:, 17] = 0.5
    for eps in (np.zeros(12, np.float32), R.epsilon(E.T)):
        assert set(R.select(E, eps, 60, 5, 0).tolist()) == {17}


def test_all_equal_errors_give_uniform_winners():
    pop, events = 10, 5000
    E = np.full((8, pop), 0.25, dtype=np.float32)
    w = R.select(E, np.zeros(8, np.float32), events, 11, 2)
    counts = np.bincount(w, minlength=pop)
    chi2 = ((counts - events / pop) ** 2 / (events / pop)).sum()
    assert chi2 < 27.9   # 9 degrees of freedom, p = 0.001


def test_specialists_win_their_block_share():
    blocks = [2, 6, 12]                    # cases per specialist
    n = sum(blocks)
    pop = len(blocks) + 5                  # five generalists, never uniquely best
    E = np.full((n, pop), 0.5, dtype=np.float32)
    c = 0
    for b, size in enumerate(blocks):
        E[:, b] = 1.0
        E[c:c + size, b] = 0.0
        c += size
    events = 3000
    w = R.select(E, np.zeros(n, np.float32), events, 3, 1)
    assert set(w.tolist()) <= set(range(len(blocks)))
    for b, size in enumerate(blocks):
        assert abs((w == b).mean() - size / n) < 0.04


def test_nan_trees_never_win_unless_all_are():
    rng = np.random.default_rng(4)
    E = rng.uniform(0, 1, (6, 20)).astype(np.float32)
    E[:, [3, 8, 9]] = np.nan
    w = R.select(E, R.epsilon(E.T), 400, 1, 0)
    assert not set(w.tolist()) & {3, 8, 9}
    E[:] = np.nan
    w = R.select(E, np.zeros(6, np.float32), 2000, 1, 0)
    assert set(w.tolist()) == set(range(20))


def test_clone_class_wins_in_proportion_to_its_size():
    # class A = trees {0, 2, 5} (identical rows), B = {1}, C = {3, 4}: nobody leaves the pool with an infinite epsilon
    E = np.array([[1, 2, 1, 3, 3, 1], [0.5, 0.1, 0.5, 0.2, 0.2, 0.5]], dtype=np.float32)
    cl = R.Classes(E)
    assert len(cl) == 3 and cl.members(0).tolist() == [0, 2, 5] and cl.members(2).tolist() == [3, 4]
    events = 6000
    w = R.select(E, np.full(2, np.inf, np.float32), events, 8, 0)
    share = np.bincount(w, minlength=6) / events
    assert abs(share[[0, 2, 5]].sum() - 0.5) < 0.03 and abs(share[1] - 1 / 6) < 0.03 and abs(share[[3, 4]].sum() - 1 / 3) < 0.03
    # -0 and +0, NaN and +inf are the same key: still three classes
    E3 = np.array([[0.0, -0.0, np.nan, np.inf]], dtype=np.float32)
    assert len(R.Classes(E3)) == 2


def test_sample_rows():
    rows = R.sample_rows(5, 3, 1000, 0.1)
    assert len(rows) == 100 and np.all(np.diff(rows) > 0)
    assert R.sample_rows(5, 3, 1000, 1.0) is None and len(R.sample_rows(5, 3, 7, 0.01)) == 1
    assert not np.array_equal(rows, R.sample_rows(5, 4, 1000, 0.1))
