"""CPU: the numpy restatement of structural duplicate detection (tests/dedup_ref.py) -- class_id against a brute-force comparison of
every pair of rows, its idempotence, and the properties of the hash."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dedup_ref as D  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from dedup_cases import planted_forest  # noqa: E402


def _brute(value, type_, size):
    pop = value.shape[0]
    out = np.empty(pop, np.int32)
    for t in range(pop):
        out[t] = next(u for u in range(t + 1) if D.rows_equal(value, type_, size, t, u))
    return out


@pytest.mark.parametrize("gp_len", [64, 1024])
def test_class_id_is_the_smallest_equal_row(rng, gp_len):
    value, type_, size = planted_forest(rng, 300, gp_len)
    cid = D.class_id(value, type_, size)
    assert cid.dtype == np.int32 and np.array_equal(cid, _brute(value, type_, size))
    assert np.all(cid <= np.arange(300)) and np.array_equal(cid[cid], cid)   # idempotent: a representative represents itself
    # the planted rows (tests/dedup_cases.py)
    assert cid[10] == cid[40] == cid[280] == cid[299] == cid[3]
    assert cid[21] == cid[20] and cid[53] == cid[50]
    for a, b in ((22, 23), (24, 25), (26, 27), (28, 29)):
        assert cid[a] != cid[b]
    assert [int(cid[t]) for t in (30, 31, 32, 33)] == [30, 31, 32, 33]
    if gp_len > 64:
        assert cid[44] == cid[41] and cid[47] == 47 and size[41, 0] > 64
    assert size[50, 0] == gp_len
    assert 1 < len(np.unique(cid)) < 300
    # equal rows carry equal hashes, and the out-of-range rows hash to 0
    h = D.tree_hash(value, type_, size)
    assert h.dtype == np.uint64 and np.array_equal(h[cid], h)
    assert all(h[t] == 0 for t in (30, 31, 32, 33))
    reps = np.unique(cid)
    reps = reps[(size[reps, 0] >= 1) & (size[reps, 0] <= gp_len)]
    # the hash does not read the size words behind n: rows 28 / 29 collide by construction, and equality still separates them.  No other
    # pair among a few hundred distinct trees shares 64 bits
    assert h[28] == h[29] and len(np.unique(h[reps[reps != 29]])) == len(reps) - 1


def test_hash_reads_the_live_prefix_only_and_is_keyed_by_position(rng):
    value, type_, size = planted_forest(rng, 100, 64)
    h = D.tree_hash(value, type_, size)
    v2, t2, s2 = value.copy(), type_.copy(), size.copy()
    tail = np.arange(64)[None, :] >= np.clip(size[:, :1].astype(np.int64), 1, 64)
    v2[tail], t2[tail], s2[tail] = 7.5, 3, 9
    assert np.array_equal(D.tree_hash(v2, t2, s2), h) and np.array_equal(D.class_id(v2, t2, s2), D.class_id(value, type_, size))
    # swapping two different leaves changes the hash: x0 - x1 against x1 - x0
    value[0, :3], type_[0, :3], size[0, :3] = [R.F_SUB, 0, 1], [R.T_BFUNC, R.T_VAR, R.T_VAR], [3, 1, 1]
    value[1, :3], type_[1, :3], size[1, :3] = [R.F_SUB, 1, 0], [R.T_BFUNC, R.T_VAR, R.T_VAR], [3, 1, 1]
    h = D.tree_hash(value, type_, size)
    assert h[0] != h[1] and D.class_id(value, type_, size)[1] == 1
    # the formula, spelled out with python integers
    M = (1 << 64) - 1

    def mix(x):
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M
        return x ^ (x >> 31)

    for t in (0, 5, 22, 23, 50):
        n = int(size[t, 0])
        acc = 0
        for i in range(n):
            w = (int(type_[t, i]) & 0xFFFF) << 32 | int(value[t, i:i + 1].view(np.uint32)[0])
            acc = (acc + mix(w ^ (((i + 1) * 0x9E3779B97F4A7C15) & M))) & M
        assert int(h[t]) == mix((acc + n) & M)
    assert int(D.mix64(np.array([12345], np.uint64))[0]) == mix(12345)
