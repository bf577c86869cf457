"""GPU: the structural kernel (csrc/sr_structure.hip) against the integer restatement (tests/structure_ref.py), word for word:
complexity, height, depth, nest, flags and violations of every row.  All arithmetic of the definition is integer, so there is no
tolerance anywhere."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimension_cases as DC  # noqa: E402
import interval_cases as IC  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import structure_cases as SC  # noqa: E402
import structure_ref as SR  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402
from test_gpu_subtree import _malform  # noqa: E402

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("complexity", "height", "depth", "nest", "flags", "violations")


# The new op joins the binding-contract table (tests/test_gpu_binding_contract.py: one row per op, every argument faulted in turn; its
# test_the_table_covers_every_op reads the table when it runs).  The row is checked below, by that module's own test body, with no
# rule (empty tensors) and with two.
def _structure_row(n_rules):
    return dict(args=BC._forest() + [BC._i("cost", 32), BC._i("operand_limit", 32, 3), BC._i("rule_outer", n_rules), BC._i("rule_inner", n_rules),
                                     BC._i("rule_limit", n_rules), ("max_depth", -1), ("max_complexity", -1)],
                outs=[((BC.POP, BC.L), BC.I32), ((BC.POP, BC.L), BC.I16), ((BC.POP, BC.L), BC.I16), ((BC.POP, BC.L, n_rules), BC.U8),
                      ((BC.POP, BC.L), BC.U8), ((BC.POP,), BC.I32)],
                scalars={"max_depth": (-2,), "max_complexity": (-2, 1 << 31)},
                tensors={"rule_outer": [("nine rules", torch.zeros(9, dtype=BC.I32))]})


_ROWS = {"evogp_hip::tree_structure": lambda: _structure_row(2)}
BC.TABLE.update(_ROWS)


@pytest.mark.parametrize("n_rules", [0, 2])
def test_binding_contract_of_the_new_op(n_rules, monkeypatch):
    monkeypatch.setitem(BC.TABLE, "evogp_hip::tree_structure", lambda: _structure_row(n_rules))
    BC.test_valid_call_and_one_fault_at_a_time("evogp_hip::tree_structure")


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _kernel(value, type_, size, p):
    args = _dev(value, type_, size, *(np.asarray(a, np.int32) for a in p[:5]))
    keep = [a.clone() for a in args]
    out = torch.ops.evogp_hip.tree_structure(*args, int(p[5]), int(p[6]))
    got = [o.cpu().numpy() for o in out]
    for a, b in zip(args, keep):      # the inputs are not written
        assert a.numel() == 0 or torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return got


def _same_words(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


def _check(value, type_, size, p, what):
    got = _kernel(value, type_, size, p)
    _same_words(got, SR.forest_structure(value, type_, size, *p), what)
    return got


def test_hand_table():
    """one row per rule and per cause of a violation (tests/structure_cases.py), each under its own parameters"""
    for c, value, type_, size in SC.table_rows():
        got = _check(value, type_, size, c["params"], c["name"])
        n = int(size[0, 0])
        assert got[5][0] == c["viol"] and got[4][0, :n].tolist() == [c["flags"].get(i, 0) for i in range(n)], c["name"]


def test_malformed_rows_of_the_hand_table():
    """a size word that is not its subtree's size (only the size check catches it: the stack discipline of the row is intact), a stack
    underflow, an empty row, a length beyond the row (clamped to L), next to a good row and a full row (n == L)"""
    value, type_, size = DC.malformed_rows(8)
    p = SC.params(rules=[([R.F_ADD], [R.F_MUL], 0)], max_depth=2, cost={R.F_MUL: 7})
    cx, ht, dp, nest, flags, viol = _check(value, type_, size, p, "malformed rows")
    assert viol.tolist() == [2, -1, -1, -1, -1, 1]
    assert flags[1].tolist() == [4] * 5 + [0] * 3 and flags[3].tolist() == [4] + [0] * 7 and flags[4].tolist() == [4] * 8
    for a in (cx, ht, dp, nest):
        assert not a[1:5].any()
    assert dp[5].tolist() == list(range(8)) and cx[0, 0] == 11


def test_every_function_over_leaf_and_non_leaf_operands():
    """each of the 29 functions as a single-operation tree over every combination of {a variable, a constant, sin(x), x + c} operands"""
    kids = [IC.V(0), IC.C(2.0), IC.U(R.F_SIN, IC.V(1)), IC.B(R.F_ADD, IC.V(2), IC.C(1.0))]
    exprs = []
    for f in range(29):
        arity = 3 if f == R.F_IF else 1 if f >= R.F_SIN else 2
        for ks in itertools.product(kids, repeat=arity):
            exprs.append(IC.IF(*ks) if arity == 3 else IC.U(f, ks[0]) if arity == 1 else IC.B(f, *ks))
    assert len(exprs) == 64 + 13 * 16 + 15 * 4
    value, type_, size = IC.rows(exprs, 16)
    every = list(range(29))
    # every function is an outer symbol: no sine below it, at most one leaf of each kind; operands of at most 2, 2 and 1
    p = SC.params(cost={f: 1 + f % 3 for f in every}, oplim={f: (2, 2, 1) for f in every},
                  rules=[(every, [R.F_SIN], 0), (every, [SR.VAR], 1), (every, [SR.CONST], 1), ([R.F_SIN], every, 0)], max_depth=2, max_complexity=6)
    viol = _check(value, type_, size, p, "single operations")[5]
    assert (viol == 0).any() and (viol > 0).any()


@pytest.mark.parametrize("n_rules", [0, 1, 3, 8])
@pytest.mark.parametrize("pop", [1, 63, 64, 65, 257])
def test_random_forests_word_for_word(pop, n_rules, rng):
    """random trees over all 29 functions, unknown ids among them, L = 64, random costs, rules and limits; planted malformed rows (a
    broken stack discipline, an empty row, a missing operand, a bad size word, a length beyond the row) inside full waves.  The
    parameters are drawn until the restatement alone yields passing and violating trees (checked on the CPU, asserted here)."""
    value, type_, size = SC.random_forest(rng, pop, 64)
    bad = ()
    if pop >= 63:
        bad = tuple(_malform(value, type_, size)) + (20, 21)
        for t, (word, s) in ((20, (1, 2)), (21, (0, 64 + 5))):      # a bad size word under an intact stack discipline, a length beyond the row
            value[t], type_[t], size[t] = IC.rows([IC.B(R.F_ADD, IC.B(R.F_MUL, IC.V(0), IC.C(2.0)), IC.V(0))], 64)
            size[t, word] = s
    for attempt in range(50):
        p = SC.random_params(rng, n_rules, tight=True)
        want = SR.forest_structure(value, type_, size, *p)
        if pop == 1 or ((want[5] == 0).any() and (want[5] > 0).any()):
            break
    assert pop == 1 or ((want[5] == 0).any() and (want[5] > 0).any())
    got = _kernel(value, type_, size, p)
    _same_words(got, want, f"pop {pop} R {n_rules}")
    cx, ht, dp, nest, flags, viol = got
    assert nest.shape == (pop, 64, n_rules)
    for t in bad:
        assert viol[t] == -1 and flags[t, 0] == SR.MALFORMED and not cx[t].any() and not ht[t].any() and not dp[t].any() and not nest[t].any()
    live = np.arange(64)[None, :] < np.maximum(size[:, :1], 1)
    assert not flags[~live].any() and not cx[~live].any() and not ht[~live].any() and not dp[~live].any() and not nest[~live].any()
    # and with every cost 1 the complexity is the subtree size
    unit = _check(value, type_, size, (SR.unit_cost(),) + tuple(p[1:]), f"pop {pop} R {n_rules}, unit costs")
    good = unit[5] >= 0
    assert np.array_equal(unit[0][good][live[good]], size[good][live[good]].astype(np.int32))


@pytest.mark.parametrize("L", [1, 2])
def test_shortest_rows(L):
    exprs = [IC.V(0), IC.C(1.0), IC.V(1)] + ([IC.U(R.F_NEG, IC.C(1.0)), IC.U(R.F_SIN, IC.V(0)), IC.U(R.F_SQRT, IC.V(2))] if L == 2 else [])
    value, type_, size = IC.rows(exprs, L)
    size[2, 0] = 0      # an empty row
    p = SC.params(rules=[([R.F_SIN], [SR.VAR], 0)], max_depth=1)
    viol = _check(value, type_, size, p, f"L {L}")[5]
    assert viol.tolist() == ([0, 0, -1] if L == 1 else [0, 0, -1, 1, 2, 1])


def test_longest_rows():
    """L = 1024: the chain of 1024 unary nodes (nest saturates at 255, height 1024, depth 1023), a right-leaning comb of 340 sums whose
    second operands lie up to 1020 words away, a left-leaning chain and a full row of ternary nodes (children 2 and 3 at far offsets)"""
    comb = SC.right_comb(340)
    ifs = []      # if(x, if(x, .. , c), c) nested through the SECOND operand: 341 ternary nodes, 1024 words
    depth = 341
    for k in range(depth):
        ifs += [[np.float32(R.F_IF), 4, 3 * (depth - k) + 1], [np.float32(k % 3), R.T_VAR, 1]]
    ifs.append([np.float32(1.0), R.T_VAR, 1])
    ifs += [[np.float32(0.5), R.T_CONST, 1]] * depth
    value, type_, size = IC.rows([SC.unary_chain(1024), comb, IC.chain(R.F_ADD, 511, True), ifs], 1024)
    assert size[:, 0].tolist() == [1024, len(comb), 1023, 1024] and len(comb) > 800
    p = SC.params(cost={R.F_SIN: 65535, SR.VAR: 65535},
                  rules=[([R.F_SIN], [R.F_SIN], 254), ([R.F_SIN, R.F_ADD, R.F_IF], [R.F_SIN, R.F_ADD, R.F_IF], 100), ([R.F_ADD], [R.F_SIN], 0),
                         ([R.F_IF], [SR.CONST], 0)], oplim={R.F_ADD: (-1, 1 << 20), R.F_IF: (-1, 1 << 20, 1)}, max_depth=1023,
                  max_complexity=65535 * 1024 - 1)
    cx, ht, dp, nest, flags, viol = _check(value, type_, size, p, "L 1024")
    i = np.arange(1024)
    assert np.array_equal(ht[0], 1024 - i) and np.array_equal(dp[0], i) and np.array_equal(nest[0, :, 0], np.minimum(255, 1023 - i))
    assert cx[0, 0] == 65535 * 1024 and flags[0, 0] == (1 | 8 | 16) and viol[0] == 922 + 2
    assert ht[1, 0] == 342 and dp[1].max() == 341 and ht[3, 0] == 342 and dp[3].max() == 341 and (viol[1:] > 0).all()


def test_input_integrity_and_determinism(rng):
    """the inputs are bit-unchanged after the call (``_kernel`` asserts it), two calls give equal words, and so does a graph replay"""
    value, type_, size = SC.random_forest(rng, 300, 64)
    p = SC.random_params(rng, 3, tight=True)
    first = _kernel(value, type_, size, p)
    _same_words(_kernel(value, type_, size, p), first, "second call")
    _same_words(first, SR.forest_structure(value, type_, size, *p), "eager")
    args = _dev(value, type_, size, *(np.asarray(a, np.int32) for a in p[:5])) + [int(p[5]), int(p[6])]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        torch.ops.evogp_hip.tree_structure(*args)      # warm-up outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = torch.ops.evogp_hip.tree_structure(*args)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(2):
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _same_words([o.cpu().numpy() for o in out], first, f"replay {k}")


def test_problem_paths_on_the_device(rng):
    """SymbolicRegression scores / evaluate on the device under mask and penalty, against the host composition: the plain problem's
    values, the restatement's violations"""
    options = dict(nested_constraints={"sin": {"sin": 0, "cos": 0}, "cos": {"sin": 0, "cos": 0}}, operand_constraints={"pow": (-1, 1)},
                   max_depth=5, complexity_of={"sin": 3, "cos": 3}, max_complexity=30)
    funcs = [R.F_ADD, R.F_SUB, R.F_MUL, R.F_POW, R.F_SIN, R.F_COS, R.F_NEG]
    value, type_, size = SC.random_forest(rng, 300, 64, max_depth=6, funcs=funcs)
    size[17, 0] = 0      # a malformed row
    X = rng.uniform(0.5, 2.0, (96, 3)).astype(np.float32)
    y = (X[:, :1] * X[:, 1:2] + np.sin(X[:, 2:3])).astype(np.float32)
    Xd, yd = _dev(X, y)
    forest = Forest(3, 1, *_dev(value, type_, size))
    from evogp_amd.tree.utils import parse_structure

    cost, oplim, rules = parse_structure(options["complexity_of"], options["nested_constraints"], options["operand_constraints"])
    want = SR.forest_structure(value, type_, size, cost, oplim, [r[0] for r in rules], [r[1] for r in rules], [r[2] for r in rules], 5, 30)
    viol = torch.from_numpy(want[5])
    assert (viol == 0).sum() > 20 and (viol > 0).sum() > 20 and viol[17] == -1
    plain = SymbolicRegression(datapoints=Xd, labels=yd)
    hard = SymbolicRegression(datapoints=Xd, labels=yd, **options)
    soft = SymbolicRegression(datapoints=Xd, labels=yd, structure_penalty=0.125, **options)
    _same_words([o.cpu().numpy() for o in hard.structure(forest)], want, "problem.structure")
    assert torch.equal(hard.structure_mask(forest).cpu(), viol == 0)
    assert torch.equal(hard.complexity(forest).cpu(), torch.from_numpy(want[0][:, 0])) and torch.equal(forest.complexity().cpu()[viol >= 0], torch.from_numpy(size[:, 0].astype(np.int32))[viol >= 0])
    sc0, ev0 = plain.scores(forest).cpu(), plain.evaluate(forest).cpu()
    ok = viol == 0
    sc, ev = hard.scores(forest).cpu(), hard.evaluate(forest).cpu()
    assert torch.equal(sc[ok].view(torch.int32), sc0[ok].view(torch.int32)) and torch.equal(ev[ok].view(torch.int32), ev0[ok].view(torch.int32))
    assert (sc[~ok] == float("-inf")).all() and torch.isnan(ev[~ok]).all()
    sc, ev = soft.scores(forest).cpu(), soft.evaluate(forest).cpu()
    assert torch.equal(sc[ok].view(torch.int32), sc0[ok].view(torch.int32)) and torch.equal(ev[ok].view(torch.int32), ev0[ok].view(torch.int32))
    pen = viol > 0
    assert torch.equal(sc[pen], sc0[pen] - 0.125 * viol[pen].float()) and sc[17] == float("-inf") and torch.isnan(ev[17])
    fin = pen & torch.isfinite(ev0)
    assert fin.any() and torch.equal(ev[fin], ev0[fin] - 0.125 * viol[fin].float())
