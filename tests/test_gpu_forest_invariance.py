"""GPU: the forest invariants (tests/forest_invariance.py) on the device, op by op and case by case: no output depends on a word behind
size[t][0] (A), on the order of the rows (B) or on the population a tree stands in (C).  Bit for bit; the cases are the smallest shapes
that reach every path the kernels switch on.  One more test goes through the Python API with a forest built from stale-tailed tensors."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
from helpers import fbits  # noqa: E402

from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("op,case", [(op, c) for op in sorted(FI.TABLE) for c in FI.cases_for(op)])
def test_op_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


def test_every_op_that_takes_a_forest_is_in_the_table():
    takes = set()
    for n in torch._C._dispatch_get_all_op_names():
        if n.startswith(("evogp_cuda::", "evogp_hip::")):
            name = n.split(".")[0]
            schema = str(torch._C._get_schema(name, "")).split("->")[0]   # (the arguments: the generators RETURN such a triple)
            if re.search(r"Tensor(\(\w!\))? value, Tensor node_type, Tensor subtree_size", schema) or name in (
                    "evogp_cuda::tree_mutate", "evogp_cuda::tree_crossover", "evogp_cuda::tree_evaluate", "evogp_cuda::tree_SR_fitness"):
                takes.add(name)   # (the reference's own five schemas name their tensors t1, t2, ...)
    assert takes == set(FI.TABLE), (sorted(takes - set(FI.TABLE)), sorted(set(FI.TABLE) - takes))
    have = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(("evogp_cuda::", "evogp_hip::"))}
    assert have == set(FI.TABLE) | set(FI.EXEMPT), (sorted(have - set(FI.TABLE) - set(FI.EXEMPT)), sorted((set(FI.TABLE) | set(FI.EXEMPT)) - have))


def _same(a, b, what):
    a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    x, y = (fbits(a), fbits(b)) if a.dtype == np.float32 else (a, b)
    assert a.shape == b.shape and np.array_equal(x, y), f"{what}: {int((x != y).sum())} words differ, first at {np.argwhere(x != y)[0].tolist()}"


def _live(forest):
    """the three arrays with every word behind the live prefix zeroed (word 0 stays)"""
    size = forest.batch_subtree_size.cpu().numpy()
    keep = torch.from_numpy(~FI.dead_mask(size)).to(forest.batch_node_value.device)
    return [torch.where(keep, a, torch.zeros_like(a)) for a in forest._tensors()]


def test_the_api_on_a_forest_built_from_stale_tailed_tensors():
    case = FI.build_case("arith_L64")
    s = case.shared
    X, y = torch.from_numpy(s["X"]).cuda(), torch.from_numpy(s["y"]).cuda()
    lower, upper = torch.from_numpy(s["lower"]).cuda(), torch.from_numpy(s["upper"]).cuda()

    def forest(triple):
        return Forest(case.var_len, 1, *[torch.from_numpy(a.copy()).cuda() for a in triple])

    zero, stale = forest(case.forest), forest(case.stale)
    fz, fs = zero.SR_fitness(X, y), stale.SR_fitness(X, y)
    _same(fs, fz, "SR_fitness")
    for a, b, what in zip(stale.SR_scaled_fitness(X, y), zero.SR_scaled_fitness(X, y), ("loss", "slope", "intercept")):
        _same(a, b, "SR_scaled_fitness " + what)
    for method in ("descent", "lm"):
        (gs, ls), (gz, lz) = stale.optimize_constants(X, y, steps=2, method=method), zero.optimize_constants(X, y, steps=2, method=method)
        _same(ls, lz, f"optimize_constants({method}) loss")
        for a, b, what in zip(_live(gs), _live(gz), ("value", "type", "size")):
            _same(a, b, f"optimize_constants({method}) live {what}")
    (gs, ls), (gz, lz) = stale.simplify(X, y), zero.simplify(X, y)
    _same(ls, lz, "simplify loss")
    for a, b, what in zip(_live(gs), _live(gz), ("value", "type", "size")):
        _same(a, b, "simplify live " + what)
    ok = torch.from_numpy(~FI._malformed_rows(case.stale, None)).cuda()[:, None]   # (a malformed row is copied as it is, dead words included)
    for a, b, what in zip(gs._tensors(), gz._tensors(), ("value", "type", "size")):
        _same(torch.where(ok, a, torch.zeros_like(a)), torch.where(ok, b, torch.zeros_like(b)), "simplify " + what)   # whole rows: zero tails
    _same(stale.safe_mask(lower, upper), zero.safe_mask(lower, upper), "safe_mask")

    desc = GenerateDescriptor(max_tree_len=case.L, input_len=case.var_len, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=3,
                              const_samples=[-1, 0, 1])
    nxt = []
    for f, fit in ((zero, fz), (stale, fs)):
        torch.manual_seed(11)
        algo = GeneticProgramming(initial_forest=f, crossover=DefaultCrossover(), mutation=DefaultMutation(0.3, desc),
                                  selection=DefaultSelection(survival_rate=0.3, elite_rate=0.02))
        nxt.append(algo.step(torch.ops.evogp_hip.fitness_scores(fit, True)))
    for a, b, what in zip(nxt[1]._tensors(), nxt[0]._tensors(), ("value", "type", "size")):
        _same(a, b, "the next generation's " + what)
    dead = FI.dead_mask(nxt[1].batch_subtree_size.cpu().numpy())
    for a, what in zip(nxt[1]._tensors(), ("value", "type", "size")):
        assert not fbits(a.cpu().numpy())[dead].any() if a.dtype == torch.float32 else not a.cpu().numpy()[dead].any(), f"the next generation's {what} tail"
    torch.cuda.synchronize()
