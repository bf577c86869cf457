"""GPU: the dimensional-analysis kernel (csrc/sr_dims.hip) against the integer restatement (tests/dimension_ref.py), word for word:
units, flags and violations of every row.  All arithmetic of the definition is integer, so there is no tolerance anywhere."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dimension_cases as DC  # noqa: E402
import dimension_ref as DR  # noqa: E402
import interval_cases as IC  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402
from test_gpu_subtree import _malform  # noqa: E402

from evogp_amd.problem import SymbolicRegression  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor  # noqa: E402

pytestmark = pytest.mark.gpu

# The new op joins the binding-contract table (tests/test_gpu_binding_contract.py: one row per op, every argument faulted in turn; its
# test_the_table_covers_every_op reads the table when it runs).  The row is checked below, by that module's own test body.
_DIM_ROWS = {
    "evogp_hip::tree_dimensions": lambda: dict(args=BC._forest() + [BC._i("var_units", BC.V, 2), BC._i("label_units", 2), ("check_root", True)],
                                               outs=[((BC.POP, BC.L, 2), BC.I32), ((BC.POP, BC.L), BC.U8), ((BC.POP,), BC.I32)]),
}
BC.TABLE.update(_DIM_ROWS)


@pytest.mark.parametrize("op", sorted(_DIM_ROWS))
def test_binding_contract_of_the_new_op(op):
    BC.test_valid_call_and_one_fault_at_a_time(op)


def _dev(*arrs):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrs]


def _kernel(value, type_, size, var_units, label, check_root):
    args = _dev(value, type_, size, np.asarray(var_units, np.int32), np.asarray(label, np.int32))
    keep = [a.clone() for a in args]
    out = torch.ops.evogp_hip.tree_dimensions(*args, bool(check_root))
    got = [o.cpu().numpy() for o in out]
    for a, b in zip(args, keep):      # the inputs are not written
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    return got


def _same_words(got, want, what):
    for name, g, w in zip(("units", "flags", "violations"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert len(bad) == 0, f"{what}: {name} differs at {bad[:5].tolist()}: {g[tuple(bad[0])]!r} != {w[tuple(bad[0])]!r}"


def _check(value, type_, size, var_units, label, check_root, what):
    got = _kernel(value, type_, size, var_units, label, check_root)
    want = DR.forest_dimensions(value, type_, size, var_units, label, check_root)
    _same_words(got, want, what)
    return got


def test_hand_table():
    """one row per rule and per cause of a violation (tests/dimension_cases.py), each with its own variables and label"""
    for c, value, type_, size, var_units, label, check_root in DC.table_rows():
        units, flags, viol = _check(value, type_, size, var_units, label, check_root, c["name"])
        assert viol[0] == c["viol"], c["name"]


def test_malformed_rows_of_the_hand_table():
    """the table's malformed rows on the device: a size word that is not its subtree's size (only the size check catches it: the stack
    discipline of the row is intact), a stack underflow, an empty row, a length beyond the row (clamped to L), next to a good row and a
    full row (n == L)"""
    value, type_, size = DC.malformed_rows(8)
    units, flags, viol = _check(value, type_, size, DC.VARS, DC.M, True, "malformed rows")
    assert viol.tolist() == [0, -1, -1, -1, -1, 0]
    assert flags[1].tolist() == [4] * 5 + [0] * 3 and flags[3].tolist() == [4] + [0] * 7 and flags[4].tolist() == [4] * 8
    assert not units[1:5].any() and (units[5] == np.array(DC.M)).all()


def test_every_function_over_every_kind_of_operand():
    """each of the 29 functions as a single-operation tree over every combination of {free, dimensionless, m, m/s} operands, with the
    root held to m and with the root free"""
    leaves = [IC.C(2.0), IC.V(3), IC.V(0), IC.V(2)]
    exprs = []
    for f in range(29):
        arity = 3 if f == R.F_IF else 1 if f >= R.F_SIN else 2
        for kids in itertools.product(leaves, repeat=arity):
            exprs.append(IC.IF(*kids) if arity == 3 else IC.U(f, kids[0]) if arity == 1 else IC.B(f, *kids))
    assert len(exprs) == 64 + 13 * 16 + 15 * 4
    value, type_, size = IC.rows(exprs, 8)
    for label, check_root in ((DC.M, True), (DC.ONE, False)):
        viol = _check(value, type_, size, DC.VARS, label, check_root, f"single operations, check_root {check_root}")[2]
        assert (viol == 0).any() and (viol > 0).any()


@pytest.mark.parametrize("K", [1, 3, 8])
@pytest.mark.parametrize("pop", [1, 63, 64, 65, 257])
def test_random_forests_word_for_word(pop, K, rng):
    """random trees over all 29 functions, NaN / inf / fractional exponents and unknown ids among them, L = 64; planted malformed rows
    (a broken stack discipline, an empty row, a missing operand, a bad size word, a length beyond the row) where the forest has room"""
    value, type_, size = DC.random_dim_forest(rng, pop, 64, 5)
    bad = _malform(value, type_, size) if pop >= 63 else ()
    if pop >= 63:      # and, in a wave of good rows: a bad size word under an intact stack discipline, a length beyond the row
        for t, (word, s) in ((20, (1, 2)), (21, (0, 64 + 5))):
            value[t], type_[t], size[t] = IC.rows([IC.B(R.F_ADD, IC.B(R.F_MUL, IC.V(0), IC.C(2.0)), IC.V(0))], 64)
            size[t, word] = s
        bad = tuple(bad) + (20, 21)
    var_units, label = DC.random_units(rng, 5, K), DC.random_units(rng, 1, K)[0]
    for check_root in (True, False):
        units, flags, viol = _check(value, type_, size, var_units, label, check_root, f"pop {pop} K {K} check_root {check_root}")
        for t in bad:
            assert viol[t] == -1 and flags[t, 0] == DR.MALFORMED and not units[t].any()
    if pop >= 63:
        assert (viol == 0).any() and (viol > 0).any()
    live = np.arange(64)[None, :] < np.maximum(size[:, :1], 1)
    assert not flags[~live].any() and not units[~live].any()


@pytest.mark.parametrize("var_len", [512, 600])
def test_many_variables(var_len, rng):
    """var_len * K = 4096 words is the largest table of units the kernel stages in LDS; 4800 words are read from memory"""
    value, type_, size = DC.random_dim_forest(rng, 130, 32, var_len, funcs=IC.ARITH + [R.F_SQRT, R.F_NEG, R.F_MAX], max_depth=4)
    var_units, label = DC.random_units(rng, var_len, 8), DC.random_units(rng, 1, 8)[0]
    _check(value, type_, size, var_units, label, True, f"var_len {var_len}")


@pytest.mark.parametrize("L", [1, 2])
def test_shortest_rows(L):
    exprs = [IC.V(0), IC.C(1.0), IC.V(1)] + ([IC.U(R.F_NEG, IC.C(1.0)), IC.U(R.F_SIN, IC.V(0)), IC.U(R.F_SQRT, IC.V(2))] if L == 2 else [])
    value, type_, size = IC.rows(exprs, L)
    size[2, 0] = 0      # an empty row
    viol = _check(value, type_, size, DC.VARS, DC.M, True, f"L {L}")[2]
    assert viol.tolist() == ([0, 0, -1] if L == 1 else [0, 0, -1, 0, 2, 1])


def test_longest_rows():
    """L = 1024: a left-deep chain and a right-deep chain of 511 operations (the walk has no operand stack to overflow), and a full row
    (n == L, no dead word) that is consistent, so that pass 2 walks all of it"""
    leaf = lambda k: [np.float32(k % 3), R.T_VAR, 1] if k % 2 else [np.float32(0.5 + (k % 5) * 0.25), R.T_CONST, 1]   # noqa: E731
    same = lambda k: [np.float32(0), R.T_VAR, 1] if k % 2 else [np.float32(2.0), R.T_CONST, 1]   # noqa: E731
    full = [[np.float32(R.F_NEG), 2, 1024]] + IC.chain(R.F_ADD, 511, True, same)
    value, type_, size = IC.rows([IC.chain(R.F_MUL, 511, True, leaf), IC.chain(R.F_DIV, 511, False, leaf), full], 1024)
    assert size[:, 0].tolist() == [1023, 1023, 1024]
    small = np.array([[3, -1, 0], [0, 2, 5], [-4, 0, 1]], np.int32)
    units, flags, viol = _check(value, type_, size, small, small[0], True, "L 1024")
    assert viol.tolist() == [0, 0, 0] and (units[2] == small[0]).all()
    _check(value, type_, size, DC.random_units(np.random.default_rng(3), 3, 3), small[0], False, "L 1024, large units")


def test_deterministic_and_graph_replay(rng):
    """two calls and a graph replay give the same words"""
    value, type_, size = DC.random_dim_forest(rng, 300, 64, 5)
    var_units, label = DC.random_units(rng, 5, 3), DC.random_units(rng, 1, 3)[0]
    args = _dev(value, type_, size, var_units, label) + [True]
    first = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_dimensions(*args)]
    second = [o.cpu().numpy() for o in torch.ops.evogp_hip.tree_dimensions(*args)]
    _same_words(second, first, "second call")
    _same_words(first, DR.forest_dimensions(value, type_, size, var_units, label, True), "eager")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        torch.ops.evogp_hip.tree_dimensions(*args)      # warm-up outside the capture
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = torch.ops.evogp_hip.tree_dimensions(*args)
    torch.cuda.current_stream().wait_stream(side)
    for k in range(2):
        for o in out:
            o.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        _same_words([o.cpu().numpy() for o in out], first, f"replay {k}")


def test_pipeline_best_tree_is_consistent(rng):
    """through the public API: SymbolicRegression(input_units=) under StandardPipeline, three generations on 512 trees; the reported
    best tree is dimensionally consistent, and the problem's mask is the restatement's"""
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, DefaultSelection, GeneticProgramming
    from evogp_amd.pipeline import StandardPipeline

    units, label = [[1, 0], [0, 1], [1, -1]], [1, -1]      # x0 m, x1 s, x2 m/s; the target in m/s
    X = rng.uniform(0.5, 2.0, (128, 3)).astype(np.float32)
    y = (X[:, :1] / X[:, 1:2] + 0.5 * X[:, 2:3]).astype(np.float32)
    Xd, yd = _dev(X, y)
    d = GenerateDescriptor(max_tree_len=32, input_len=3, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4, const_samples=[-1, 0, 1, 2])
    algo = GeneticProgramming(Forest.random_generate(512, d, keys=torch.tensor([7, 11], dtype=torch.uint32, device="cuda")), DefaultCrossover(),
                              DefaultMutation(0.2, d), DefaultSelection(0.3, 2))
    prob = SymbolicRegression(datapoints=Xd, labels=yd, input_units=units, label_units=label)
    start = algo.forest
    mask = prob.dimension_mask(start).cpu().numpy()
    want = DR.forest_dimensions(*(a.cpu().numpy() for a in start._tensors()), np.array(units) * DR.DEN, np.array(label) * DR.DEN, True)[2]
    assert np.array_equal(mask, want == 0) and 0 < mask.sum() < 512
    plain = SymbolicRegression(datapoints=Xd, labels=yd)
    sc, sc0 = prob.scores(start).cpu(), plain.scores(start).cpu()
    m = torch.from_numpy(mask)
    assert torch.equal(sc[m].view(torch.int32), sc0[m].view(torch.int32)) and (sc[~m] == float("-inf")).all()
    pipe = StandardPipeline(algo, prob, generation_limit=3, is_show_details=False)
    for _ in range(3):
        pipe.step()
    best = pipe.best_tree
    one = Forest(3, 1, best.node_value[None, :].cuda(), best.node_type[None, :].cuda(), best.subtree_size[None, :].cuda())
    assert int(prob.dimensions(one)[2][0]) == 0 and np.isfinite(float(pipe.best_fitness))
