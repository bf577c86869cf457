"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_subtree_signatures / subtree_library_select backed by the numpy
restatement (tests/sublib_ref.py) on the CPU oracle's predictions, so that the host logic of Forest.SR_subtree_signatures /
subtree_library, SemanticLibrary.update_library(source="subtrees") and the operators' refresh_every can be exercised without a GPU.
The product registers no CPU implementation.  ``calls`` counts the invocations of each."""
import numpy as np
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import sublib_ref as SL
from oracle.pyoracle import Oracle

_done = False
calls = {"subtree_signatures": 0, "library_select": 0}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True
    oracle = Oracle("port")

    def subtree_signatures(pop, D, L, vl, ol, v, t, s, X):
        calls["subtree_signatures"] += 1
        assert ol == 1 and v.shape == t.shape == s.shape == (pop, L) and X.shape == (D, vl) and X.dtype == torch.float32
        return torch.from_numpy(SL.forest_signatures(oracle, _np(v), _np(t), _np(s), _np(X)).view(np.int64))

    def library_select(sig, size, min_size, max_size, k):
        calls["library_select"] += 1
        assert sig.dtype == torch.int64 and size.dtype == torch.int16 and sig.shape == size.shape and sig.dim() == 2
        if not (1 <= k <= SL.MAX_LIB and 1 <= min_size <= max_size):
            raise RuntimeError(f"k, min_size, max_size out of range: {k}, {min_size}, {max_size}")
        member, count, n = SL.select(_np(sig), _np(size), min_size, max_size, k)
        return torch.from_numpy(member), torch.from_numpy(count), torch.tensor([n], dtype=torch.int32)

    torch.library.impl("evogp_hip::tree_SR_subtree_signatures", "CPU")(subtree_signatures)
    torch.library.impl("evogp_hip::subtree_library_select", "CPU")(library_select)
