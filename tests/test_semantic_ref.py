"""CPU: the numpy restatement of semantic duplicate classes (tests/semantic_ref.py) on the CPU oracle's predictions satisfies every
assertion about the planted forest (tests/semantic_cases.py) that the GPU test repeats, and its own definitions hold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import semantic_ref as S  # noqa: E402
from dedup_ref import GOLD, mix64  # noqa: E402
from semantic_cases import COPY_OF, COPY_ROW, DEEP_ROW, DIFFERENT, FULL_ROW, MALFORMED, SAME, dataset, planted_forest  # noqa: E402


def check_planted(c, sig, K, size, gp_len, D):
    """what the reference and the device must both satisfy on a planted forest of at least 63 rows: c (pop,) class ids, sig (pop,)
    uint64 signatures, K (pop, D) keys"""
    pop = len(c)
    for group in SAME:
        assert len({int(c[t]) for t in group}) == 1 and len({int(sig[t]) for t in group}) == 1, group
        assert int(c[group[0]]) <= group[0]
    for a, b in DIFFERENT:
        differ = bool((K[a] != K[b]).any())
        if D >= 130 or (a, b) != (26, 27):   # (one row may not tell (a + b) + c from a + (b + c))
            assert differ, (a, b)
        assert (c[a] != c[b]) == differ
    assert c[COPY_ROW] == c[COPY_OF] and c[pop - 1] == c[9]
    assert size[FULL_ROW, 0] == gp_len and c[FULL_ROW + 1] == c[FULL_ROW]
    assert [int(c[t]) for t in MALFORMED] == MALFORMED and all(sig[t] == 0 for t in MALFORMED)
    assert np.isnan(K[15].view(np.float32)).all() and (K[15] == S.CANONICAL_NAN).all()   # NaN on every row, canonical
    # the last row alone separates 28 / 29 and 32 / 33, and it is where 30 / 31 differ by the sign of a zero
    assert (K[28, :-1] == K[29, :-1]).all() and K[28, -1] != K[29, -1]
    assert (K[32, :-1] == K[33, :-1]).all() and K[32, -1] == np.float32(-np.inf).view(np.uint32) and K[33, -1] == S.CANONICAL_NAN
    if gp_len > 64:
        assert size[41, 0] == 79 and c[44] == c[41]
    assert int(size[DEEP_ROW, 0]) > 40


@pytest.mark.parametrize("gp_len, D", [(64, 1), (64, 130), (1024, 130), (64, 1100)])
def test_the_reference_satisfies_the_planted_cases(rng, oracle, gp_len, D):
    pop = 200
    value, type_, size = planted_forest(rng, pop, gp_len)
    X = dataset(rng, D)
    with np.errstate(all="ignore"):
        P, formed = S.oracle_predictions(oracle, value, type_, size, X)
    assert P.shape == (pop, D) and P.dtype == np.float32
    c, sig, K = S.class_id(P, formed), S.signature(P, formed), S.keys(P)
    check_planted(c, sig, K, size, gp_len, D)
    # raw bits: rows 30 / 31 really differ by a signed zero, which the keys identify
    raw = P.view(np.uint32)
    assert raw[30, -1] == 0x80000000 and raw[31, -1] == 0 and (raw[30, :-1] == raw[31, :-1]).all()
    # class ids are idempotent first indices, and equal signatures inside a class
    assert (c <= np.arange(pop)).all() and (c[c] == c).all()
    assert all(sig[t] == sig[c[t]] for t in range(pop))
    # the random part has classes of its own (small trees repeat), the planted part is not the whole story
    assert 63 < len(np.unique(c)) < pop


def test_keys_signature_and_representatives():
    P = np.array([[0.0, -0.0, np.inf, -np.inf, 1.5],
                  [-0.0, 0.0, np.inf, -np.inf, 1.5],
                  [0.0, 0.0, -np.inf, np.inf, 1.5],
                  [np.nan, 1.0, 2.0, 3.0, 4.0],
                  [-np.nan, 1.0, 2.0, 3.0, 4.0]], np.float32)
    P.view(np.uint32)[4, 0] = 0xFFC12345   # a NaN with a sign and a payload
    K = S.keys(P)
    assert (K[0] == K[1]).all() and K[0, 0] == 0 and K[0, 2] == 0x7F800000 and K[0, 3] == 0xFF800000
    assert (K[0] != K[2]).sum() == 2 and K[3, 0] == K[4, 0] == 0x7FC00000
    formed = np.array([True, True, True, True, False])
    sig = S.signature(P, formed)
    with np.errstate(over="ignore"):
        want = mix64(np.array([mix64(K[0].astype(np.uint64) ^ (np.arange(1, 6, dtype=np.uint64) * GOLD)).sum(dtype=np.uint64) + np.uint64(5)]))[0]
    assert sig[0] == sig[1] == want and sig[2] != sig[0] and sig[4] == 0 and sig[3] != 0
    # position-keyed: swapping two columns changes the signature
    assert S.signature(P[:, [1, 0, 2, 3, 4]], formed)[3] != sig[3]
    assert S.class_id(P, formed).tolist() == [0, 0, 2, 3, 4]
    assert S.class_id(P, np.ones(5, bool)).tolist() == [0, 0, 2, 3, 3]
    # smallest member, ties to the smallest index; a singleton stays
    first = np.array([0, 0, 2, 0, 2, 5])
    assert S.smallest_representative(first, [7, 3, 4, 3, 4, 9]).tolist() == [1, 1, 2, 1, 2, 5]
