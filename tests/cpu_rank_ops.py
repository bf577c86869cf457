"""TEST-ONLY: CPU implementations of the two rank ops on the numpy restatement (tests/rank_ref.py) and the CPU oracle's predictions, for
the host logic of Forest and RankFitness.  The product registers no CPU implementation.  ``calls`` counts the invocations."""
import functools

import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import rank_ref as RR
import semantic_ref as S
from oracle.pyoracle import Oracle

calls = {"rank_rows": 0, "rank_stats": 0}
_np = lambda t: t.detach().cpu().numpy()  # noqa: E731


@functools.lru_cache(maxsize=None)
def register():
    oracle = Oracle("port")

    def rank_rows(values, payload, seg_start, max_segment):
        calls["rank_rows"] += 1
        seg = _np(seg_start).astype(np.int64)
        r2, c, st = RR.rank_rows(_np(values), seg)
        if payload is not None:
            c = RR.consts(_np(payload), seg)
        return torch.from_numpy(r2.astype(np.int32)), torch.from_numpy(c), torch.from_numpy(st.astype(np.int32))

    def rank_stats(v, t, s, X, payload, seg_start, max_segment, metric, want_words, want_fused, want_scores):
        calls["rank_stats"] += 1
        seg = _np(seg_start).astype(np.int64)
        assert payload.dtype == torch.int32 and seg[-1] == X.shape[0] and 1 <= np.diff(seg).min() and np.diff(seg).max() <= max_segment <= 8192
        with np.errstate(all="ignore"):
            P, formed = S.oracle_predictions(oracle, _np(v), _np(t), _np(s), _np(X))
        w, st = RR.words(P, formed, _np(payload), seg)
        sc = RR.scores(w, RR.consts(_np(payload), seg), seg, ["spearman", "auc"][metric])
        fu = RR.fused(sc, st)
        return (torch.from_numpy(w if want_words else w[:0]), torch.from_numpy(fu if want_fused else fu[:0]),
                torch.from_numpy(sc if want_scores else sc[:0]), torch.from_numpy(st))

    torch.library.impl("evogp_hip::rank_rows", "CPU")(rank_rows)
    torch.library.impl("evogp_hip::tree_SR_rank_stats", "CPU")(rank_stats)
