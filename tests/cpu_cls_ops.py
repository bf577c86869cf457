"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_batch_class_stats backed by the numpy restatement (tests/cls_ref.py), so
that the host logic of Forest.class_stats and of Classification's metrics and validation mask can be exercised without a GPU.  The
product registers no CPU implementation."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import cls_ref as CR

_done = False
calls = {"class_stats": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def class_stats(pop, D, L, var_len, out_len, v, t, s, X, labels, groups, n_groups):
        calls["class_stats"] += 1
        assert v.shape == (pop, L) == t.shape == s.shape and v.dtype == torch.float32 and t.dtype == s.dtype == torch.int16
        assert X.shape == (D, var_len) and X.dtype == torch.float32 and labels.shape == (D,) and labels.dtype == torch.int32
        assert 2 <= out_len <= 16 and 1 <= n_groups <= 8
        assert (groups is None and n_groups == 1) or (groups.shape == (D,) and groups.dtype == torch.int32)
        h, p, loss, _ = CR.forest_stats((_np(v), _np(t), _np(s)), _np(X), _np(labels), out_len, None if groups is None else _np(groups), n_groups)
        return torch.from_numpy(h), torch.from_numpy(p), torch.from_numpy(np.ascontiguousarray(loss))

    torch.library.impl("evogp_hip::tree_batch_class_stats", "CPU")(class_stats)
