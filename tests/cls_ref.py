"""TEST-ONLY: a numpy restatement of evogp_hip_batch_class_stats (include/evogp_hip.h; csrc/cls_stats.hip) and of the metrics
Classification derives from it.  The outputs of the trees come from the oracle's batch evaluation (as tests/cpu_ops.py obtains them; a
malformed tree has every output NaN, the rule of classify_tree), the prediction is torch.argmax(clip(softmax(.))) as tests/helpers.py
states it (on the CPU, or on the device torch's own kernels run on), the loss is taken step by step in float32 as the header specifies
-- and once more in float64, the same formula without the float32 roundings: the truth the device's loss is held to.  No GPU import."""
import numpy as np
import torch

from oracle.pyoracle import Oracle

_O = Oracle("port")
CAP32 = np.float32(34.538776)            # -log(1e-15), the reference's clip, as the kernel holds it
CAP64 = float(-np.log(1e-15))
T_MASK = 0x7F


def well_formed(type_row, n):
    """the stack discipline classify_tree checks in multi-output mode (the type is masked, the OUT flag changes no arity)"""
    if n <= 0:
        return False
    h = 0
    for i in reversed(range(n)):
        t = int(type_row[i]) & T_MASK
        h += 1 - (0 if t in (0, 1) else 1 if t == 2 else 2 if t == 3 else 3)
        if h < 1:
            return False
    return h == 1


def outputs(value, type_, size, X, out_len):
    """float32 [pop][D][out_len]: the trees' outputs on the rows of X, NaN throughout for a malformed tree"""
    value, type_, size = (np.array(a, copy=True, order="C") for a in (value, type_, size))
    X = np.ascontiguousarray(X, np.float32)
    pop, L = value.shape
    n = np.clip(size[:, 0].astype(np.int64), 0, L)
    bad = np.array([not well_formed(type_[t], int(n[t])) for t in range(pop)])
    value[bad, 0], type_[bad, 0], size[bad, 0] = 0.0, 1, 1      # (the oracle walks whatever it is given: a malformed row becomes one leaf)
    outs = _O.batch_evaluate(value, type_, size, X, out_len)
    outs[bad] = np.nan
    return outs


def predict(outs, device="cpu", block=256):
    """int64 [pop][D]: torch.argmax(torch.clip(torch.softmax(outs), 1e-15, 1 - 1e-15)) with torch's kernels on `device`"""
    out = []
    for i in range(0, outs.shape[0], block):
        o = torch.from_numpy(np.ascontiguousarray(outs[i:i + block])).to(device)
        out.append(torch.argmax(torch.clip(torch.softmax(o, dim=2), 1e-15, 1 - 1e-15), dim=2).cpu())
    return torch.cat(out).numpy()


def splits(labels, groups, n_groups, out_len):
    """int64 [D]: the split a row is counted in, -1 for a row that is not counted"""
    labels = np.asarray(labels).astype(np.int64)
    g = np.zeros(len(labels), np.int64) if groups is None else np.asarray(groups).astype(np.int64)
    ok = (g >= 0) & (g < n_groups) & (labels >= 0) & (labels < out_len)
    return np.where(ok, g, -1)


def row_loss(outs, labels, dtype=np.float32):
    """[pop][D]: the clamped cross-entropy of every row against its label (rows whose label is out of range: against class 0, unused),
    NaN for a poisoned row; dtype float32 follows the header step by step, float64 is the same formula without those roundings"""
    x = np.asarray(outs, np.float32).astype(dtype)
    C = x.shape[2]
    y = np.clip(np.asarray(labels).astype(np.int64), 0, C - 1)
    with np.errstate(all="ignore"):
        m = x.max(2)                                       # (NaN where an output is NaN)
        poisoned = np.isnan(x).any(2) | np.isinf(m)
        s = np.zeros(m.shape, dtype)
        for o in range(C):                                 # o ascending
            s = (s + np.exp((x[:, :, o] - m).astype(dtype)).astype(dtype)).astype(dtype)
        xy = np.take_along_axis(x, np.broadcast_to(y[None, :, None], x.shape[:2] + (1,)), 2)[:, :, 0]
        l = (np.log(s).astype(dtype) - (xy - m).astype(dtype)).astype(dtype)
        cap = CAP32 if dtype == np.float32 else CAP64
        l = np.where(l < 0, dtype(0), np.where(l > cap, dtype(cap), l)).astype(dtype)
    return np.where(poisoned, dtype(np.nan), l)


def mean_loss(l, rows):
    """float64 [pop]: the mean of l over `rows` as the kernel takes it -- every l as a part on the 2^-20 grid plus its remainder, both
    column sums exact, one addition, one division; NaN for no rows"""
    l = np.asarray(l, np.float64)[:, rows]
    with np.errstate(all="ignore"):
        hi = (l + 2.0 ** 32) - 2.0 ** 32
        lo = l - hi
        return (hi.sum(1) + lo.sum(1)) / np.float64(l.shape[1]) if l.shape[1] else np.full(l.shape[0], np.nan)


def stats_of(outs, pred, labels, groups=None, n_groups=1, dtype=np.float32):
    """-> hits int32 [pop][G][C], predicted int32 [pop][G][C], loss float64 [pop][G] from the outputs and the predictions"""
    pop, D, C = outs.shape
    slot = splits(labels, groups, n_groups, C)
    y = np.asarray(labels).astype(np.int64)
    l = row_loss(outs, labels, dtype)
    hits, predicted = np.zeros((pop, n_groups, C), np.int32), np.zeros((pop, n_groups, C), np.int32)
    loss = np.zeros((pop, n_groups), np.float64)
    for g in range(n_groups):
        rows = np.flatnonzero(slot == g)
        for c in range(C):
            predicted[:, g, c] = (pred[:, rows] == c).sum(1)
            hits[:, g, c] = ((pred[:, rows] == c) & (y[rows] == c)[None, :]).sum(1)
        loss[:, g] = mean_loss(l, rows) if dtype == np.float32 else (l[:, rows].mean(1) if len(rows) else np.nan)
    return hits, predicted, loss


def forest_stats(forest, X, labels, out_len, groups=None, n_groups=1, device="cpu"):
    """-> (hits, predicted, loss as the device computes it, loss in float64: the truth)"""
    outs = outputs(*forest, X, out_len)
    pred = predict(outs, device)
    h, p, loss32 = stats_of(outs, pred, labels, groups, n_groups, np.float32)
    _, _, loss64 = stats_of(outs, pred, labels, groups, n_groups, np.float64)
    return h, p, loss32, loss64


# ---- the metrics of Classification, from the counts of one split --------------------------------------------------------------------
def support_of(labels, groups, n_groups, out_len):
    """float64 [G][C]: the counted rows of every split by label"""
    slot, y = splits(labels, groups, n_groups, out_len), np.asarray(labels).astype(np.int64)
    return np.array([[((slot == g) & (y == c)).sum() for c in range(out_len)] for g in range(n_groups)], np.float64)


def metric(name, hits, predicted, loss, support):
    """float64 [pop]: one split's metric; hits, predicted [pop][C], loss [pop], support [C]; NaN -> -inf"""
    hits, predicted = np.asarray(hits, np.float64), np.asarray(predicted, np.float64)
    n, seen = support.sum(), support > 0
    with np.errstate(all="ignore"):
        if name == "cross_entropy":
            out = -np.asarray(loss, np.float64)
        elif name == "accuracy":
            out = hits.sum(1) / n
        elif name == "balanced_accuracy":
            out = (hits[:, seen] / support[seen]).sum(1) / seen.sum()
        elif name == "f1_macro":
            out = (2.0 * hits[:, seen] / (support[seen] + predicted[:, seen])).sum(1) / seen.sum()
        elif name == "mcc":
            cov = hits.sum(1) * n - (predicted * support).sum(1)
            den = np.sqrt((n * n - (predicted * predicted).sum(1)) * (n * n - (support * support).sum()))
            out = np.where(den == 0, 0.0, cov / np.where(den == 0, 1.0, den))
        else:
            raise ValueError(name)
    return np.where(np.isnan(out), -np.inf, out)
