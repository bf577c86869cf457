"""CPU: the numpy restatement of evogp_hip_batch_class_stats (tests/cls_ref.py) on cases whose answers are worked out by hand here, and
against scikit-learn's metrics.  The hand cases use IDENTITY trees -- output o is x_o * 1 -- so a row of X is the row of outputs: margins,
NaN and infinities are written straight into the data."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cls_ref as CR  # noqa: E402

LN2 = math.log(2.0)
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def identity_forest(pop, C, L=64, scale=None):
    """ADD(OUT_0: x_0 * s_0, ADD(OUT_1: x_1 * s_1, ...)): output o of tree t is x_o * scale[t][o] (default 1)"""
    v = np.zeros((pop, L), np.float32); t = np.zeros((pop, L), np.int16); s = np.zeros((pop, L), np.int16)
    n = 4 * C - 1
    assert n <= L
    for r in range(pop):
        pos = 0
        for o in range(C):
            if o < C - 1:
                v[r, pos] = 1.0; t[r, pos] = 3; s[r, pos] = n - pos; pos += 1
            v[r, pos:pos + 1].view(np.uint32)[:] = (o << 16) | 3             # OUT node: {function MUL, output index o}
            t[r, pos] = 3 | 0x80; s[r, pos] = 3
            v[r, pos + 1] = o; t[r, pos + 1] = 0; s[r, pos + 1] = 1          # x_o
            v[r, pos + 2] = 1.0 if scale is None else scale[r, o]; t[r, pos + 2] = 1; s[r, pos + 2] = 1
            pos += 3
    return v, t, s


def _one(X, labels, groups=None, G=1, C=2):
    h, p, l32, l64 = CR.forest_stats(identity_forest(1, C), np.asarray(X, np.float32), np.asarray(labels), C, groups, G)
    return h[0], p[0], l32[0], l64[0]


def test_two_classes_with_known_margins():
    # outputs (0, 0) label 0: tie -> class 0, l = ln 2; (1, 0) label 0: class 0, l = ln(1 + e^-1); (1, 0) label 1: l = 1 + ln(1 + e^-1);
    # (0, 3) label 1: class 1, l = ln(1 + e^-3)
    X = [[0, 0], [1, 0], [1, 0], [0, 3]]
    h, p, l32, l64 = _one(X, [0, 0, 1, 1])
    assert h.tolist() == [[2, 1]] and p.tolist() == [[3, 1]]
    want = (LN2 + math.log1p(math.exp(-1)) + 1 + math.log1p(math.exp(-1)) + math.log1p(math.exp(-3))) / 4
    assert abs(l64[0] - want) < 1e-12 and abs(l32[0] - want) < 1e-6


def test_a_poisoned_row_inside_and_outside_a_split():
    X = [[0, 0], [NAN, 0], [0, 0], [INF, 0], [0, -INF]]
    labels = [0, 0, 1, 0, 0]
    # the NaN row in split 1, the +inf row not counted: split 0 = rows 0, 2, 4, all of loss ln 2 but row 4 (x_1 = -inf: s = 1, l = 0)
    h, p, l32, l64 = _one(X, labels, np.array([0, 1, 0, -1, 0]), 2)
    assert math.isnan(l32[1]) and math.isnan(l64[1]) and abs(l32[0] - 2 * LN2 / 3) < 1e-6
    assert p.tolist() == [[3, 0], [1, 0]] and h.tolist() == [[2, 0], [1, 0]]       # the NaN row is predicted as class 0, its label
    # the same rows with the infinite one inside split 0: that split is NaN, class 0 predicted there
    h, p, l32, _ = _one(X, labels, np.array([0, 1, 0, 0, 0]), 2)
    assert math.isnan(l32[0]) and math.isnan(l32[1]) and p.tolist() == [[4, 0], [1, 0]]
    # outside every split both are harmless
    h, p, l32, _ = _one(X, labels, np.array([0, 7, 0, -1, 0]), 2)
    assert abs(l32[0] - 2 * LN2 / 3) < 1e-6 and math.isnan(l32[1]) and p.tolist() == [[3, 0], [0, 0]]


def test_a_skipped_row_an_empty_split_and_an_out_of_range_label():
    X = [[2, 0], [0, 2], [0, 2], [2, 0]]
    h, p, l32, _ = _one(X, [0, 1, 2, -1], np.array([0, 0, 0, 0]), 3)     # labels 2 and -1 name no class of a 2-class tree
    assert h.tolist() == [[1, 1], [0, 0], [0, 0]] and p.tolist() == [[1, 1], [0, 0], [0, 0]]
    assert abs(l32[0] - math.log1p(math.exp(-2))) < 1e-6 and math.isnan(l32[1]) and math.isnan(l32[2])
    h, p, l32, _ = _one(X, [0, 1, 0, 1], np.array([0, 9, 2, -5]), 3)     # rows 1 and 3 skipped, split 1 empty
    assert p.tolist() == [[1, 0], [0, 0], [0, 1]] and h.tolist() == [[1, 0], [0, 0], [0, 0]]
    assert math.isnan(l32[1]) and abs(l32[2] - (2 + math.log1p(math.exp(-2)))) < 1e-6


def test_the_clip_at_minus_log_1e_15():
    h, p, l32, l64 = _one([[0, 100], [0, 34], [0, 35]], [0, 0, 0])
    # l = 100 -> 34.538776; 34 + ln(1 + e^-34) stays; 35 -> clipped
    want = (2 * -math.log(1e-15) + 34.0) / 3
    assert abs(l64[0] - want) < 1e-9 and abs(l32[0] - want) < 1e-5
    assert float(CR.row_loss(np.array([[[0, 100]]], np.float32), [0], np.float32)[0, 0]) == float(np.float32(34.538776))


def test_a_malformed_tree_predicts_class_zero_with_loss_nan():
    f = identity_forest(2, 2)
    f[2][1, 0] = 5                      # cut in the middle of a subtree
    h, p, l32, _ = CR.forest_stats(f, np.array([[0, 1], [1, 0]], np.float32), np.array([0, 1]), 2)
    assert p[1].tolist() == [[2, 0]] and h[1].tolist() == [[1, 0]] and math.isnan(l32[1, 0]) and np.isfinite(l32[0, 0])


@pytest.mark.filterwarnings("ignore")
def test_against_sklearn(rng):
    import sklearn.metrics as sk
    pop, C, D = 12, 4, 200
    scale = rng.uniform(-2, 2, (pop, C)).astype(np.float32)
    X = rng.normal(size=(D, C)).astype(np.float32) * 2
    y = rng.integers(0, C - 1, D)          # class 3 has no support: the averages leave it out
    y[:3] = [0, 1, 2]
    forest = identity_forest(pop, C, scale=scale)
    h, p, l32, l64 = CR.forest_stats(forest, X, y, C)
    outs = CR.outputs(*forest, X, C).astype(np.float64)
    support = CR.support_of(y, None, 1, C)[0]
    assert support.tolist() == np.bincount(y, minlength=C).tolist() and support[3] == 0
    for t in range(pop):
        z = outs[t] - outs[t].max(1, keepdims=True)
        prob = np.exp(z) / np.exp(z).sum(1, keepdims=True)
        pred = prob.argmax(1)
        cm = sk.confusion_matrix(y, pred, labels=list(range(C)))
        assert np.array_equal(np.diag(cm), h[t, 0]) and np.array_equal(cm.sum(0), p[t, 0])
        want = sk.log_loss(y, np.clip(prob, 1e-15, 1.0), labels=list(range(C)))
        assert abs(l64[t, 0] - want) < 1e-9 and abs(l32[t, 0] - want) < 1e-5
        m = lambda name: float(CR.metric(name, h[t:t + 1, 0], p[t:t + 1, 0], l32[t:t + 1, 0], support)[0])  # noqa: E731
        assert abs(m("accuracy") - sk.accuracy_score(y, pred)) < 1e-12
        assert abs(m("balanced_accuracy") - sk.balanced_accuracy_score(y, pred)) < 1e-12
        assert abs(m("f1_macro") - sk.f1_score(y, pred, average="macro", labels=[0, 1, 2])) < 1e-12
        assert abs(m("mcc") - sk.matthews_corrcoef(y, pred)) < 1e-12
        assert m("cross_entropy") == -l32[t, 0]


def test_mcc_is_zero_for_a_constant_prediction_and_nan_scores_minus_infinity():
    support = np.array([3.0, 2.0])
    assert CR.metric("mcc", [[3, 0]], [[5, 0]], [0.0], support)[0] == 0.0
    assert CR.metric("cross_entropy", [[3, 0]], [[5, 0]], [np.nan], support)[0] == -np.inf
    assert CR.metric("accuracy", [[0, 0]], [[0, 0]], [np.nan], np.zeros(2))[0] == -np.inf     # an empty split
