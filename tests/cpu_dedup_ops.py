"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_hash / tree_classes backed by the numpy restatement
(tests/dedup_ref.py), so that the host logic of Forest.structure_hash / duplicate_classes / unique, the ``dedup=True`` paths and
GeneticProgramming(regenerate_duplicates=) can be exercised without a GPU, and of tree_generate_masked (the oracle's generator for
every row: the rows a mask leaves out are unspecified, and the callers never read them).  The product registers no CPU
implementation.  ``calls`` counts the invocations of each."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import dedup_ref
from oracle.pyoracle import Oracle

_done = False
calls = {"tree_hash": 0, "tree_classes": 0, "generate_masked": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True
    oracle = Oracle("port")

    def tree_hash(v, t, s):
        calls["tree_hash"] += 1
        return torch.from_numpy(dedup_ref.tree_hash(_np(v), _np(t), _np(s)).view(np.int64))

    def tree_classes(v, t, s, h):
        calls["tree_classes"] += 1
        assert h.dtype == torch.int64 and h.shape == (v.shape[0],)
        return torch.from_numpy(dedup_ref.class_id(_np(v), _np(t), _np(s)))

    def generate_masked(pop, L, var_len, out_len, n_const, out_prob, const_prob, keys, d2l, rou, cs, offset, word, below):
        calls["generate_masked"] += 1
        assert word.dtype == torch.int32 and word.shape == (pop,)
        k = _np(keys.to(torch.int64)).astype(np.uint32)
        return tuple(torch.from_numpy(a) for a in
                     oracle.generate(pop, L, var_len, out_len, out_prob, const_prob, k, _np(d2l), _np(rou), _np(cs), offset))

    torch.library.impl("evogp_hip::tree_hash", "CPU")(tree_hash)
    torch.library.impl("evogp_hip::tree_classes", "CPU")(tree_classes)
    torch.library.impl("evogp_hip::tree_generate_masked", "CPU")(generate_masked)
