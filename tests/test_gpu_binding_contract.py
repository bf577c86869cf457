"""GPU: what the torch binding (csrc/torch_ops.cpp) checks and what it allocates, op by op.  One table, one row per op of both
namespaces: a minimal valid call (4 trees of one CONST leaf in rows of 8 words, 8 data points, 2 variables) with the shape and dtype of
every output, then one fault at a time -- every tensor argument with a wrong dtype, with a wrong shape and non-contiguous, and the
scalar faults the row lists -- each of which must raise a RuntimeError that names the offending argument.  Every fault fails in the
binding's host checks, before an allocation or a launch.  A row may list further valid calls (`also`): the breed ops with NO donor
rows, which a range or a generation of elites only has."""
import os
import re
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)
from evogp_amd import _lib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import depth2leaf, roulette_uniform  # noqa: E402

pytestmark = pytest.mark.gpu

POP, L, D, V = 4, 8, 8, 2
F32, I16, I32, I64, U8 = torch.float32, torch.int16, torch.int32, torch.int64, torch.uint8
WRONG = {F32: torch.float64, I16: I32, I32: I64, I64: I32, U8: I32, torch.uint32: F32}
NORMAL = 44   # EVOGP_LM_NORMAL_WORDS


def _t(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def _forest(rows=POP, gp_len=L, names=("value", "type", "subtree_size")):
    """rows of one CONST leaf (T_CONST = 1)"""
    value, type_, size = np.zeros((rows, gp_len), np.float32), np.zeros((rows, gp_len), np.int16), np.zeros((rows, gp_len), np.int16)
    value[:, 0], type_[:, 0], size[:, 0] = 1.0, 1, 1
    return [(n, _t(a)) for n, a in zip(names, (value, type_, size))]


def _donors(rows):
    return _forest(rows, L, ("donor_value", "donor_type", "donor_size"))


def _f(name, *shape):
    return (name, torch.full(shape, 0.5, dtype=F32, device="cuda"))


def _i(name, *shape):
    return (name, torch.zeros(shape, dtype=I32, device="cuda"))


def _arange(name, n):
    return (name, torch.arange(n, dtype=I32, device="cuda"))


def _gen_tables():
    return [("depth2leaf_probs", _t(depth2leaf(3))), ("roulette_funcs", _t(roulette_uniform([1, 2, 3, 4]))),
            ("const_samples", _t(np.array([-1, 0, 1], np.float32)))]


def _gen_head():
    return [("pop_size", POP), ("gp_len", L), ("var_len", V), ("out_len", 1), ("const_samples_len", 3), ("out_prob", 0.5), ("const_prob", 0.5)]


def _keys():
    return ("keys", torch.tensor([42, 0], dtype=torch.uint32, device="cuda"))


def _data_head(out_len=1, use_mse=True):
    head = [("pop_size", POP), ("data_points", D), ("gp_len", L), ("var_len", V), ("out_len", out_len)]
    return head + ([("use_mse", True)] if use_mse else [])


def _xy():
    return [_f("variables", D, V), _f("labels", D, 1)]


FOREST_OUT = [((POP, L), F32), ((POP, L), I16), ((POP, L), I16)]
ELITE_RANGE_OUT = [((2, L), F32), ((2, L), I16), ((2, L), I16)]
SIZES = {"pop_size": (0,), "gp_len": (0, 1025)}
ORDER = r"\border\b"   # check_order's text says "order" for whichever list it checks
LIST_SAYS = {(a, k): ORDER for a in ("elite_rows", "parent_rows") for k in ("dtype", "contig")}


def _no_donors(**other):
    """the arguments of a call whose rows are all elites: donor arrays of no rows"""
    return dict(dict(_donors(0)), **other)


def _ws_bytes():
    return int(_lib.lib.evogp_hip_evaluate_workspace_bytes(POP, L))


def _prepared_ws():
    return torch.ops.evogp_hip.tree_evaluate_prepare(POP, L, V, 2, *[a for _, a in _forest()])[0]


def _roulettes():
    p = np.zeros(29, np.float32)
    p[[1, 2, 3, 4, 14, 25, 0]] = 1.0 / 7

    def of(lo, hi):
        only = np.zeros(29, np.float32)
        only[lo:hi] = p[lo:hi]
        return _t(np.cumsum(only, dtype=np.float32))
    return [("roulette_ufuncs", of(14, 29)), ("roulette_bfuncs", of(1, 14)), ("roulette_tfuncs", of(0, 1))]


# op -> () -> dict(args [(name, value)], outs [(shape, dtype)] or None for an in-place op, scalars {name: faulty values},
#              says {(argument, "dtype" | "shape" | "contig"): pattern} where the binding's text names something else than the argument,
#              also [(label, {name: value} replacing arguments of the valid call, outs)]: further calls that must succeed)
TABLE = {
    # ---- evogp_cuda: the reference's five ----
    "evogp_cuda::tree_generate": lambda: dict(args=_gen_head() + [_keys()] + _gen_tables(), outs=FOREST_OUT, scalars=SIZES),
    "evogp_cuda::tree_mutate": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L)] + _forest(names=("value_ori", "type_ori", "subtree_size_ori")) + [_i("mutateIndices", POP)]
        + _forest(names=("value_new", "type_new", "subtree_size_new")), outs=FOREST_OUT, scalars=SIZES),
    "evogp_cuda::tree_crossover": lambda: dict(
        args=[("pop_size_ori", POP), ("pop_size_new", 3), ("gp_len", L)] + _forest(names=("value_ori", "type_ori", "subtree_size_ori"))
        + [_i("left_idx", 3), _i("right_idx", 3), _i("left_node_idx", 3), _i("right_node_idx", 3)],
        outs=[((3, L), F32), ((3, L), I16), ((3, L), I16)], scalars={"pop_size_ori": (0,), "pop_size_new": (0,), "gp_len": (0, 1025)}),
    "evogp_cuda::tree_evaluate": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L), ("var_len", V), ("out_len", 1)] + _forest() + [_f("variables", POP, V)],
        outs=[((POP, 1), F32)], scalars=SIZES),
    "evogp_cuda::tree_SR_fitness": lambda: dict(args=_data_head() + _forest() + _xy() + [("kernel_type", 4)], outs=[((POP,), F32)], scalars=SIZES),
    # ---- evogp_hip: generation and evaluation ----
    "evogp_hip::tree_generate_offset": lambda: dict(args=_gen_head() + [_keys()] + _gen_tables() + [("tree_index_offset", 0)], outs=FOREST_OUT,
                                                    scalars=SIZES),
    "evogp_hip::tree_generate_masked": lambda: dict(
        args=_gen_head() + [_keys()] + _gen_tables() + [("tree_index_offset", 0), _i("active_word", POP), ("active_below", 1)], outs=FOREST_OUT,
        scalars=SIZES),
    "evogp_hip::tree_generate_masked_hashed": lambda: dict(
        args=_gen_head() + _gen_tables() + [("tree_index_offset", 0), ("seed", 1), ("generation", 0), ("active_below", 1 << 31)], outs=FOREST_OUT,
        scalars=SIZES),
    "evogp_hip::tree_batch_evaluate": lambda: dict(args=_data_head(use_mse=False) + _forest() + [_f("variables", D, V)], outs=[((POP, D, 1), F32)],
                                                   scalars=SIZES),
    "evogp_hip::tree_batch_argmax_count": lambda: dict(
        args=_data_head(2, use_mse=False) + _forest() + [_f("variables", D, V), _i("labels", D)], outs=[((POP,), I32)],
        scalars=dict(SIZES, out_len=(1, 17))),
    "evogp_hip::tree_evaluate_prepare": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L), ("var_len", V), ("out_len", 2)] + _forest(), outs=[((_ws_bytes(),), U8), ((16,), I32)], scalars=SIZES),
    "evogp_hip::tree_evaluate_prepared": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L), ("var_len", V), ("out_len", 2)] + _forest()
        + [("workspace", _prepared_ws()), ("with_fallback", True), _f("variables", POP, V)], outs=[((POP, 2), F32)], scalars=SIZES),
    "evogp_hip::tree_SR_fitness_masked": lambda: dict(args=_data_head() + _forest() + _xy() + [("kernel_type", 4), ("func_mask", 0)],
                                                      outs=[((POP,), F32)], scalars=SIZES),
    # ---- the words, the selections ----
    "evogp_hip::random_words": lambda: dict(
        args=[("seed", 1), ("generation", 0), ("rows", 6), ("n_cols", 4), ("lo", 0), ("hi", 4), ("device", torch.device("cuda", torch.cuda.current_device()))],
        outs=[((6, 4), I32)]),
    "evogp_hip::fitness_scores": lambda: dict(args=[_f("errors", POP), ("negate", True)], outs=[((POP,), F32)]),
    "evogp_hip::select_survivors": lambda: dict(args=[_f("fitness", POP), ("n_elite", 1), ("n_keep", 2)], outs=[((2,), I32)]),
    "evogp_hip::tournament_select": lambda: dict(args=[_f("fitness", POP), ("n_tournaments", 3), ("t_size", 2), ("seed", 1), ("generation", 0)],
                                                 outs=[((3,), I32)]),
    "evogp_hip::lexicase_select": lambda: dict(args=[_f("errors", 3, POP), _f("eps", 3), ("n_events", 5), ("seed", 1), ("generation", 0)],
                                               outs=[((5,), I32)]),
    "evogp_hip::pareto_rank": lambda: dict(args=[_f("err", POP), _i("cx", POP), ("cx_bound", 8)], outs=[((POP,), I32), ((POP,), F32), ((POP,), I32)],
                                           scalars={"cx_bound": (65536,)}),
    "evogp_hip::nsga2_select": lambda: dict(args=[_arange("order", POP), ("pool", 2), ("n", 3), ("t_size", 2), ("seed", 1), ("generation", 0)],
                                            outs=[((3,), I32)], scalars={"pool": (0,)}),
    # ---- breeding and mutation ----
    "evogp_hip::breed_default": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L), ("n_elite", 1), ("n_surv", 2)] + _forest() + [_arange("order", POP), _i("rnd", 6, POP - 1), ("mutate_below", 0)]
        + _donors(POP - 1) + [("want_decisions", True)], outs=FOREST_OUT + [((POP - 1, 6), I32)], scalars=SIZES,
        also=[("a generation of elites only", _no_donors(n_elite=POP, rnd=_i("rnd", 6, 0)[1]), FOREST_OUT + [((0, 6), I32)])]),
    "evogp_hip::breed_default_rows": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L), ("n_elite", 1), ("n_surv", 2)] + _forest() + [_arange("order", POP), _i("rnd", 6, POP - 1), ("mutate_below", 0)]
        + _donors(POP) + [("row_begin", 0), ("row_count", POP)], outs=FOREST_OUT, scalars=SIZES,
        also=[("a range inside the elites, donors for its offspring only", _no_donors(n_elite=2, rnd=_i("rnd", 6, POP - 2)[1], row_count=2), ELITE_RANGE_OUT)]),
    "evogp_hip::breed_rows": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L)] + _forest() + [_arange("elite_rows", 1), _arange("parent_rows", 2), _i("rnd", 6, POP - 1), ("mutate_below", 0)]
        + _donors(POP) + [("row_begin", 0), ("row_count", POP)], outs=FOREST_OUT, scalars=SIZES, says=LIST_SAYS,
        also=[("a range inside the elites, donors for its offspring only",
               _no_donors(elite_rows=_arange("elite_rows", 2)[1], rnd=_i("rnd", 6, POP - 2)[1], row_count=2), ELITE_RANGE_OUT)]),
    "evogp_hip::breed_rows_hashed": lambda: dict(
        args=[("pop_size", POP), ("gp_len", L)] + _forest() + [_arange("elite_rows", 1), _arange("parent_rows", 2), ("seed", 1), ("generation", 0), ("mutate_below", 0)]
        + _donors(POP) + [("row_begin", 0), ("row_count", POP)], outs=FOREST_OUT, scalars=SIZES, says=LIST_SAYS,
        also=[("a range inside the elites, donors for its offspring only", _no_donors(elite_rows=_arange("elite_rows", 2)[1], row_count=2), ELITE_RANGE_OUT)]),
    "evogp_hip::structural_mutate": lambda: dict(
        args=[("mode", 0), ("rate", 0.0), ("max_size", L), ("inner_is_offset", False), ("skip_rows", 0), ("seed", 1), ("call", 0)] + _forest()
        + [("want_decisions", True)], outs=FOREST_OUT + [((POP, 2), I32)]),
    "evogp_hip::insert_mutate": lambda: dict(
        args=[("mutate_below", 0), ("skip_rows", 0), ("seed", 1), ("call", 0)] + _forest() + _donors(POP) + [("want_decisions", True)],
        outs=FOREST_OUT + [((POP, 2), I32)],
        # the binding checks the donors as a second forest under the forest's own names
        says={(d, k): p for k in ("dtype", "shape", "contig") for d, p in (("donor_value", r"\bvalue\b"), ("donor_type", r"(?<!scalar )\btype\b"),
                                                                   ("donor_size", r"\bsubtree_size\b"))}),
    "evogp_hip::point_mutate": lambda: dict(
        args=[("mode", 0), ("rate", 0.0), ("intensity", 0.1), ("per_node", False), ("modify_output", False), ("fix_roulette", False), ("skip_rows", 0),
              ("input_len", V), ("output_len", 1), ("seed", 1), ("call", 0)] + _forest() + _roulettes() + [("const_samples", _t(np.array([-1, 0, 1], np.float32)))],
        outs=[((POP, L), F32)]),
    # ---- the constant optimisers, the per-case and per-subtree passes ----
    "evogp_hip::tree_SR_gradient": lambda: dict(args=_data_head() + _forest() + _xy(), outs=[((POP,), F32), ((POP, L), F32)],
                                                scalars=dict(SIZES, out_len=(17,))),
    "evogp_hip::tree_SR_const_step": lambda: dict(
        args=[("phase", 3), ("out_len", 1)] + _forest() + [_f("value_cand", POP, L), _f("loss", POP), _f("grad", POP, L), _f("loss_cand", POP),
                                                           _f("grad_cand", POP, L), _f("step", POP)], outs=None, scalars={"phase": (0, 4)}),
    "evogp_hip::tree_SR_case_errors": lambda: dict(args=_data_head() + _forest() + _xy(), outs=[((D, POP), F32)], scalars=SIZES),
    "evogp_hip::tree_SR_subtree_errors": lambda: dict(args=_data_head() + _forest() + _xy(), outs=[((POP, L), F32), ((POP, L), F32)],
                                                      scalars=dict(SIZES, out_len=(2,))),
    "evogp_hip::tree_prune": lambda: dict(
        args=[("out_len", 1), ("hoist", True), ("fold", True)] + _forest() + [_f("node_err", POP, L), _f("node_const", POP, L)],
        outs=FOREST_OUT + [((POP,), I32), ((POP,), F32)], scalars={"out_len": (2,)}),
    "evogp_hip::tree_SR_normal_eq": lambda: dict(args=_data_head(use_mse=False) + _forest() + _xy(), outs=[((POP,), F32), ((POP, NORMAL), F32)],
                                                 scalars=dict(SIZES, out_len=(2,))),
    "evogp_hip::tree_SR_lm_step": lambda: dict(
        args=[("phase", 3)] + _forest() + [_f("value_cand", POP, L), _f("loss", POP), _f("normal", POP, NORMAL), _f("loss_cand", POP),
                                           _f("normal_cand", POP, NORMAL), _f("damping", POP)], outs=None, scalars={"phase": (0, 4)}),
    "evogp_hip::tree_SR_linear_scaling": lambda: dict(args=_data_head(use_mse=False) + _forest() + _xy(), outs=[((POP,), F32), ((POP, 2), F32)],
                                                      scalars=dict(SIZES, out_len=(2,))),
    "evogp_hip::tree_wrap_linear": lambda: dict(args=[("out_gp_len", 16)] + _forest() + [_f("coef", POP, 2)],
                                                outs=[((POP, 16), F32), ((POP, 16), I16), ((POP, 16), I16), ((POP,), U8)]),
    # ---- structure: duplicates, intervals ----
    "evogp_hip::tree_hash": lambda: dict(args=_forest(), outs=[((POP,), I64)]),
    "evogp_hip::tree_classes": lambda: dict(args=_forest() + [("hash", torch.zeros(POP, dtype=I64, device="cuda"))], outs=[((POP,), I32)]),
    "evogp_hip::tree_intervals": lambda: dict(args=_forest() + [_f("lower", V), _f("upper", V)], outs=[((POP, L), F32), ((POP, L), F32), ((POP, L), U8)]),
    "evogp_hip::tree_derivative_intervals": lambda: dict(
        args=_forest() + [_f("lower", V), _f("upper", V), _i("wrt", 1)],
        outs=[((POP, L), F32), ((POP, L), F32), ((POP, L), U8), ((1, POP, L), F32), ((1, POP, L), F32), ((1, POP, L), U8)],
        tensors={"wrt": [("empty", torch.zeros(0, dtype=I32))]}),
}


def _pattern(name):
    if name.startswith("donor_"):
        return r"donor"                            # "value (donor) ...", "donor arrays must have ..."
    if name.startswith("type"):
        return r"(?<!scalar )\b" + name + r"\b"    # (not the "type" of "expected scalar type Short for ...")
    return r"\b" + re.escape(name) + r"\b"


def _strided(t):
    """the same shape and values, every other element of a buffer twice as wide: not contiguous (None: one element cannot be)"""
    raw = t.view(I32) if t.dtype == torch.uint32 else t   # (copies of 32-bit patterns)
    wide = torch.zeros(raw.shape[:-1] + (2 * raw.shape[-1],), dtype=raw.dtype, device=raw.device)
    view = wide[..., ::2]
    view.copy_(raw)
    view = view.view(t.dtype)
    assert view.shape == t.shape
    return None if view.is_contiguous() else view


def _faults(row):
    """(label, argument index, faulty value, pattern) for every fault of the row"""
    says = row.get("says", {})
    for k, (name, a) in enumerate(row["args"]):
        if isinstance(a, torch.Tensor):
            yield f"{name} dtype", k, torch.zeros(a.shape, dtype=WRONG[a.dtype], device=a.device), says.get((name, "dtype"), _pattern(name))
            yield f"{name} shape", k, a.unsqueeze(0), says.get((name, "shape"), _pattern(name))
            if _strided(a) is not None:
                yield f"{name} non-contiguous", k, _strided(a), says.get((name, "contig"), _pattern(name))
            for label, bad in row.get("tensors", {}).get(name, []):
                yield f"{name} {label}", k, bad.to(a.device), _pattern(name)
        else:
            for bad in row.get("scalars", {}).get(name, ()):
                yield f"{name} = {bad}", k, bad, _pattern(name)


def _check_outputs(out, want, what):
    """a valid call's outputs: the documented shape, dtype and device, contiguous (want None: an in-place op returns nothing)"""
    torch.cuda.synchronize()
    if want is None:
        assert out is None, what
        return
    outs = list(out) if isinstance(out, (tuple, list)) else [out]
    assert len(outs) == len(want), (what, len(outs), len(want))
    dev = torch.device("cuda", torch.cuda.current_device())
    for k, (o, (shape, dtype)) in enumerate(zip(outs, want)):
        assert tuple(o.shape) == tuple(shape) and o.dtype == dtype and o.device == dev and o.is_contiguous(), (what, k, o.shape, o.dtype, o.device)


@pytest.mark.parametrize("op", sorted(TABLE))
def test_valid_call_and_one_fault_at_a_time(op):
    row = TABLE[op]()
    ns, name = op.split("::")
    fn = getattr(getattr(torch.ops, ns), name)
    args = [a for _, a in row["args"]]
    _check_outputs(fn(*args), row["outs"], op)
    names = [n for n, _ in row["args"]]
    for label, other, outs in row.get("also", []):
        assert set(other) <= set(names), (label, sorted(set(other) - set(names)))
        _check_outputs(fn(*[other.get(n, a) for n, a in row["args"]]), outs, f"{op}, {label}")
    n = 0
    for label, k, bad, pattern in _faults(row):
        call = list(args)   # (a fault fails before any launch: the in-place ops' tensors are not written)
        call[k] = bad
        with pytest.raises(RuntimeError) as e:
            fn(*call)
        assert re.search(pattern, str(e.value)), f"{op}: {label}: the text does not match {pattern!r}: {str(e.value)[:300]}"
        n += 1
    print(f"{op}: {n} faults rejected")
    torch.cuda.synchronize()


def test_the_table_covers_every_op():
    have = {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(("evogp_cuda::", "evogp_hip::"))}
    assert have == set(TABLE), (sorted(have - set(TABLE)), sorted(set(TABLE) - have))
