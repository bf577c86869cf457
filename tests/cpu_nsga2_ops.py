"""TEST-ONLY: CPU implementations of torch.ops.evogp_hip.pareto_rank / nsga2_select backed by the numpy twin (tests/nsga2_ref.py), so
that the host logic of NSGA2Selection can be exercised without a GPU.  The product registers no CPU implementation."""
import torch

import cpu_ops
import evogp_amd  # noqa: F401  (defines the schemas)
import nsga2_ref

_done = False


def register():
    global _done
    if _done:
        return
    _done = True
    cpu_ops.register()

    def pareto_rank(err, cx, cx_bound):
        assert err.is_contiguous() and err.dtype == torch.float32 and err.dim() == 1
        assert cx.is_contiguous() and cx.dtype == torch.int32 and cx.shape == err.shape
        front, crowding, order = nsga2_ref.rank(err.numpy(), cx.numpy(), cx_bound)
        return torch.from_numpy(front), torch.from_numpy(crowding), torch.from_numpy(order)

    def select(order, pool, n, t_size, seed, generation):
        assert order.is_contiguous() and order.dtype == torch.int32 and order.dim() == 1
        return torch.from_numpy(nsga2_ref.select(order.numpy(), pool, n, t_size, seed, generation))

    torch.library.impl("evogp_hip::pareto_rank", "CPU")(pareto_rank)
    torch.library.impl("evogp_hip::nsga2_select", "CPU")(select)
