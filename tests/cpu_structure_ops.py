"""TEST-ONLY: a CPU implementation of torch.ops.evogp_hip.tree_structure backed by the integer restatement (tests/structure_ref.py), so
that the host logic of Forest.SR_structure / structure_mask / complexity and SymbolicRegression(max_depth=, ...) can be exercised
without a GPU.  The product registers no CPU implementation.  ``calls`` counts the invocations, ``last`` keeps the arguments of the
latest one."""
import torch

import evogp_amd  # noqa: F401  (defines the schemas)
import structure_ref as SR

_done = False
calls = {"tree_structure": 0}
last = {}


def _np(t):
    return t.detach().cpu().numpy()


def register():
    global _done
    if _done:
        return
    _done = True

    def tree_structure(v, t, s, cost, operand_limit, rule_outer, rule_inner, rule_limit, max_depth, max_complexity):
        calls["tree_structure"] += 1
        tables = (cost, operand_limit, rule_outer, rule_inner, rule_limit)
        assert all(a.dtype == torch.int32 for a in tables)
        assert cost.shape == (32,) and operand_limit.shape == (32, 3) and rule_outer.shape == rule_inner.shape == rule_limit.shape
        last.update(cost=_np(cost).copy(), operand_limit=_np(operand_limit).copy(), rule_outer=_np(rule_outer).copy(),
                    rule_inner=_np(rule_inner).copy(), rule_limit=_np(rule_limit).copy(), max_depth=int(max_depth),
                    max_complexity=int(max_complexity))
        out = SR.forest_structure(_np(v), _np(t), _np(s), *(_np(a) for a in tables), int(max_depth), int(max_complexity))
        return tuple(torch.from_numpy(a) for a in out)

    torch.library.impl("evogp_hip::tree_structure", "CPU")(tree_structure)
