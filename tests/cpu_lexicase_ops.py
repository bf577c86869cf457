"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.tree_SR_case_errors / lexicase_select backed by the numpy twin
(tests/lexicase_ref.py) and the oracle-backed batch evaluation (tests/cpu_ops.py), so that the host logic of LexicaseSelection and
Forest.SR_case_errors can be exercised without a GPU.  The product registers no CPU implementation."""
import numpy as np
import torch

import cpu_ops
import evogp_amd  # noqa: F401  (defines the schemas)
import lexicase_ref

_done = False


def register():
    global _done
    if _done:
        return
    _done = True
    cpu_ops.register()

    def case_errors(pop, D, L, vl, ol, mse, v, t, s, X, y):
        pred = torch.ops.evogp_hip.tree_batch_evaluate(pop, D, L, vl, ol, v, t, s, X).numpy()
        return torch.from_numpy(lexicase_ref.case_errors(pred, y.numpy(), mse))

    def select(errors, eps, n_events, seed, generation):
        assert errors.is_contiguous() and errors.dtype == torch.float32 and errors.dim() == 2
        w = lexicase_ref.select(errors.numpy(), eps.numpy(), n_events, seed, generation)
        return torch.from_numpy(w.astype(np.int32))

    torch.library.impl("evogp_hip::tree_SR_case_errors", "CPU")(case_errors)
    torch.library.impl("evogp_hip::lexicase_select", "CPU")(select)
