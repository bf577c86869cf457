"""TEST-ONLY: graph capture and replay, op by op (tests/test_gpu_graph_replay.py).  Two tables with one row per registered op between them:

  CAPTURE[op]          how to call the op so that the call can be recorded into a HIP graph: an adapter in the style of
                       tests/forest_invariance.py (FI) that makes every device tensor with ``FI._d`` and returns ``FI._o(result)``
  NOT_CAPTURABLE[op]   (reason, "file:line"): the entry point waits for the host, allocates engine memory on every call or returns host
                       values BY DESIGN; the citation shows where.  An op whose documentation says it can be captured may not be listed.

How an adapter becomes (args, call, outputs_of, inplace).  The adapters of FI and of the ``*_tables.py`` modules copy host arrays to the
device and read the result back inside the call, which a capture cannot record.  They do both through two functions, ``FI._d`` and
``FI._o``, which ``taped`` swaps for the time of a call:

  record   ``_d`` copies the host array to the device as always and appends the tensor to a tape, with a pristine clone beside it; ``_o``
           returns the device tensors.  This IS the first eager call, and the tape is ``args``: every tensor, made before the capture.
  play     ``_d`` hands out the tape's tensors in the same order and copies nothing (the host array the adapter computed for it is
           dropped: nothing of it reaches the device); ``_o`` returns the device tensors.  This is ``call(args)``: launches only.

An adapter is therefore usable only if every device tensor it makes comes from ``FI._d``, and ``taped`` checks that: a torch call that
returns a tensor on a device none of its arguments is on (a factory, a copy from the host) outside ``FI._d`` fails the call.  Those of pair_tables, gram_tables, neigh_tables
and of the two simulation losses make some with torch.arange / torch.tensor / torch.full (a host-to-device copy or a fill of their own) and
have a twin here.  The ops that take no forest (FI.EXEMPT) get adapters that draw their inputs from the case's forest and per-tree tables,
so that input set B -- the same case with its rows permuted (``FI.permute``) -- changes them too.  ``evogp_hip::random_words`` has no
tensor argument at all: nothing a replay could see changed, so its row is marked ``no_b`` and replay 3 repeats replay 2."""
import contextlib
import functools
import os
import sys

import numpy as np
import torch
from torch.utils import _pytree as pytree
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import test_gpu_binding_contract as BC  # noqa: E402,F401
import agx_tables, backprop_tables, cls_tables, gram_tables, intron_tables, neigh_tables, pair_tables  # noqa: E402,F401,E401
import rank_tables, simulate_sens_tables, simulate_tables as ST, sublib_tables, xgrad_tables  # noqa: E402,F401,E401
from helpers import depth2leaf, roulette_uniform  # noqa: E402

hip, cu = FI.hip, FI.cu

# name -> (the FI case, pop, D): pop in the tens, D a few hundred at most; the second L crosses 64 (global tapes, the general and deep
# kernels, FULL builds, var_len 40 > 32, trees of 63 / 64 / 65 nodes); the third is for the multi-output ops; the fourth puts the two
# segments of the rank ops on either side of their 1024-row threshold
# the fifth is the L > 64 case of the ops that take multi-output forests only (MULTI_LONG below: FI has no such case)
CASES = {
    "arith_L64": ("arith_L64", 48, 70),
    "all_L1024_v40": ("all_L1024_v40", 24, 70),
    "multi_L64": ("multi_L64", 40, 70),
    "arith_L64_D2049": ("arith_L64", 32, 2049),
    "multi_L160": ("multi_L160", 40, 70),
}
# what replay 2 is disturbed with: the same op on other shapes (another pop, a gp_len on the other side of 64, and one LARGER than the
# captured shape so that the stream's workspaces regrow) ...
DISTURB = {
    "arith_L64": [("all_L1024_v40", 31, 70)],
    "all_L1024_v40": [("arith_L64", 37, 70), ("all_L1024_v40", 31, 70)],
    "multi_L64": [("multi_L160", 53, 70)],
    "arith_L64_D2049": [("all_L1024_v40", 31, 70)],
    "multi_L160": [("multi_L64", 29, 70), ("multi_L160", 53, 70)],
}
# ... and where its tree_SR_fitness and tree_SR_gradient calls come from: a gp_len on the other side of 64
OTHER = {
    "arith_L64": ("all_L1024_v40", 31, 70), "all_L1024_v40": ("arith_L64", 37, 70), "multi_L64": ("all_L1024_v40", 31, 70),
    "arith_L64_D2049": ("all_L1024_v40", 31, 70), "multi_L160": ("arith_L64", 37, 70),
}
MULTI_LONG, MULTI_LONG_L = "multi_L160", 160


def _widen(a, L0, L):
    """a (pop, L0) array in rows of L words, zeros behind"""
    if isinstance(a, tuple):
        return tuple(_widen(x, L0, L) for x in a)
    if not (isinstance(a, np.ndarray) and a.ndim == 2 and a.shape[1] == L0):
        return a
    out = np.zeros((a.shape[0], L), a.dtype)
    out[:, :L0] = a
    return out


@functools.lru_cache(maxsize=None)
def build_case(name, pop, D):
    """FI.build_case, and one case of this module's own: FI's multi-output forest (4 outputs, 3 variables) in rows of 160 words, its
    chains (rows 2, 9, 16, ...) made 41, 81 and 141 nodes long, every dead word rewritten as FI.stale_tails does"""
    if name != MULTI_LONG:
        return FI.build_case(name, pop, D)
    base, L0, L = FI.build_case("multi_L64", pop, D), 64, MULTI_LONG_L
    rng = np.random.default_rng([20261126, pop, D])
    c = FI.Case()
    c.__dict__.update(base.__dict__)
    c.name, c.L = name, L
    value, type_, size = (a.copy() for a in _widen(base.forest, L0, L))
    for k, t in enumerate(range(2, pop, 7)):
        FI._set(value, type_, size, t, FI._chain(rng, (20, 40, 70)[k % 3], c.var_len, (FI.R.F_ADD, FI.R.F_SUB, FI.R.F_MUL)))
    size[5, 0] = L + 1   # (as in FI: n > L)
    c.forest = (value, type_, size)
    sv, st, ss, c.planted = FI.stale_tails(rng, value, type_, size, c.out_len)
    c.stale = (sv, st, ss)
    c.shared = {k: _widen(v, L0, L) for k, v in base.shared.items()}
    c.per_tree = {k: _widen(v, L0, L) for k, v in base.per_tree.items()}
    return c


def case(name):
    return build_case(*CASES[name])


# ---- the tape --------------------------------------------------------------------------------------------------------------------------
class Tape:
    def __init__(self):
        self.tensors, self.pristine = [], []


def _raw(t):
    """the bytes of a contiguous tensor (copies of every dtype, the unsigned ones included)"""
    return t.view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)


class _Watch(TorchDispatchMode):
    """every tensor of a taped call comes from the tape or from an op on tensors of the tape: a torch call that returns a tensor on a
    device none of its tensor arguments is on -- a factory (torch.arange, torch.full, torch.tensor) or a copy from the host -- is an
    error unless ``FI._d`` makes it.  The project's own ops are not looked at (random_words takes no tensor by design)."""
    inside_d = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        if not self.inside_d and func.namespace not in ("evogp_hip", "evogp_cuda"):
            have = {t.device for t in pytree.tree_leaves((args, kwargs)) if isinstance(t, torch.Tensor)}
            made = [t for t in pytree.tree_leaves(out) if isinstance(t, torch.Tensor) and t.device not in have]
            assert not made, f"{func}: the adapter makes a tensor that is not on the tape; make it with FI._d (tests/capture_tables.py)"
        return out


@contextlib.contextmanager
def taped(tape, mode):
    saved = FI._d, FI._o
    at = [0]
    watch = _Watch()

    def d(a, device):
        if mode == "record":
            watch.inside_d += 1
            try:
                t = saved[0](a, device)
                tape.tensors.append(t)
                tape.pristine.append(t.clone())
            finally:
                watch.inside_d -= 1
            return t
        assert at[0] < len(tape.tensors), "the adapter asks for more tensors than it recorded"
        t = tape.tensors[at[0]]
        at[0] += 1
        return t

    def o(res):
        res = res if isinstance(res, (tuple, list)) else (res,)
        return tuple(res)

    FI._d, FI._o = d, o
    try:
        with watch:
            yield
        assert mode == "record" or at[0] == len(tape.tensors), "the adapter asked for fewer tensors than it recorded"
    finally:
        FI._d, FI._o = saved


def inputs(op, c, variant):
    """(forest, shared, per-tree) of input set A (the case's stale-tail forest) or B (the same, its rows permuted)"""
    row = CAPTURE[op]
    fs, pop = c.stale, c.pop
    if variant == "A":
        return fs, c.shared, row["select"](fs, c.per_tree, np.arange(pop))[0]
    import zlib
    perm = FI.permute(np.random.default_rng([11, zlib.crc32(op.encode()), pop]), pop)[0]
    f = tuple(a[perm] for a in fs)
    if FI.TABLE.get(op, {}).get("cls") == "classes":   # a class op on a forest without duplicates returns 0 .. pop-1 in every order
        for a in f:
            a[1:12:2] = a[0:11:2]
    return f, c.shared, row["select"](fs, c.per_tree, perm)[1]


def build(op, c, device, variant="A"):
    """-> (args, call, outputs_of, inplace, first): `args` the tape of input set `variant`, recorded by one eager call whose outputs are
    `first`; call(args) launches only and returns the op's result; outputs_of(result) the tensors to compare; inplace: an output IS an
    argument"""
    row, tape = CAPTURE[op], Tape()
    f, s, p = inputs(op, c, variant)
    with taped(tape, "record"):
        first = row["call"](f, s, p, device)

    def call(args):
        assert args is tape
        with taped(tape, "play"):
            return row["call"](f, s, p, device)

    held = {t.data_ptr() for t in tape.tensors if t.numel()}
    inplace = any(o.numel() and o.data_ptr() in held for o in first)
    return tape, call, tuple, inplace, first


def restore(tape, source=None):
    for t, q in zip(tape.tensors, (source or tape).pristine):
        assert t.shape == q.shape and t.dtype == q.dtype, "input sets A and B must have the same shapes"
        if t.numel():
            _raw(t).copy_(_raw(q))


def eager(op, c, device):
    """one ordinary call (host copies, read-back): what replay 2 is disturbed with"""
    f, s, p = inputs(op, c, "A")
    return CAPTURE[op]["call"](f, s, p, device)


# ---- adapters of the ops whose FI adapter makes tensors of its own ---------------------------------------------------------------------
def _i32(a, device):
    return FI._d(np.ascontiguousarray(a, np.int32), device)


def _sr_fitness(f, s, p, device):
    """unhinted, WITHOUT dropping the observations (FI._sr_fitness does, through a host call): the second eager call and the captured one
    follow what the first observed, and every build returns the same bits"""
    return FI._o(cu.tree_SR_fitness(*FI._head(f, s), True, *FI._f(f, device), FI._d(s["X"], device), FI._d(s["y"], device), 4))


def _prepare(f, s, p, device):
    """the workspace itself: info, the record counts, and the records below each tree's count (the binding's workspace is uninitialised
    memory, and eval_prepare_kernel writes rec[slot][t] for slot < count[t] alone: csrc/evaluate_prepared.hip)"""
    pop, L = f[0].shape
    ws, info = hip.tree_evaluate_prepare(pop, L, s["var_len"], s["out_len"], *FI._f(f, device))
    maxrec = min(L, 64)
    rec = ws[:maxrec * pop * 16].view(torch.int32).view(maxrec, pop, 4)
    count = ws[maxrec * pop * 16:maxrec * pop * 16 + pop * 4].view(torch.int32)
    live = (_i32(np.arange(maxrec), device)[:, None] < count[None, :])[:, :, None]
    return FI._o((torch.where(live, rec, torch.zeros_like(rec)), count.clone(), info.clone()))


def _pairs(f, s, p, device):
    fd, X, y, donors = FI._f(f, device), FI._d(s["X"], device), FI._d(s["y1"], device), FI._f(s["donors"], device)
    pop, nd = f[0].shape[0], s["donors"][0].shape[0]
    t = _i32(np.arange(pop), device)
    against = _i32(np.tile([0, nd // 2, nd - 1], (pop, 1)), device)
    own, mom = hip.tree_SR_pair_moments(*fd, *donors, X, y, t, against)
    own0, self_ = hip.tree_SR_pair_moments(*fd, *fd, X, None, t, _i32(np.arange(pop)[:, None], device))
    return FI._o((own, mom, own0, self_))


def _gram(f, s, p, device):
    fd, X, y = FI._f(f, device), FI._d(s["X"], device), FI._d(s["y1"], device)
    t = _i32(np.arange(f[0].shape[0]), device)
    return FI._o(tuple(hip.tree_SR_gram(*fd, X, y, t, True)) + tuple(hip.tree_SR_gram(*fd, X, None, t, False)))


def _neigh(f, s, p, device):
    fd, X = FI._f(f, device), FI._d(s["X"], device)
    t = _i32(np.arange(f[0].shape[0]), device)
    return FI._o(hip.tree_SR_neighbours(*fd, X, t, 3, FI._d(np.array([1.0, 4.0]), device)))


def _targets(s, device):
    for scheme, S in ST._systems(s):
        x0, u = ST._inputs(s, S, device)
        SC = 1 if scheme == 3 else S
        rows = np.arange(ST.B * ST.T * SC) % s["D"]
        target = FI._d(s["y1"][rows].reshape((ST.B, ST.T) if scheme == 3 else (ST.B, ST.T, S)), device)
        yield scheme, x0, u, target, FI._d(np.linspace(0.5, 1.5, SC).astype(np.float32), device)


def _sim_loss(f, s, p, device):
    fd, out = FI._f(f, device), ()
    for scheme, x0, u, target, _ in _targets(s, device):
        out += FI._o(hip.tree_SR_simulation_loss(*fd, x0, u, target, scheme, 0.1))
    return out


def _sim_normal(f, s, p, device):
    fd, out = FI._f(f, device), ()
    for scheme, x0, u, target, weight in _targets(s, device):
        out += FI._o(hip.tree_SR_simulation_normal_eq(*fd, x0, u, target, weight, scheme, 0.1))
    return out


def _rank_segments(D):
    """two segments, of 1024 and 1025 rows where the case has them (the one-block sort ends at 1024)"""
    return ([0, 1024, 2049], 1025) if D >= 2049 else ([0, D // 3, D], D - D // 3)


def _rank_stats(f, s, p, device):
    seg, longest = _rank_segments(s["D"])
    payload = _i32(np.arange(s["D"]) % 7, device)
    return FI._o(hip.tree_SR_rank_stats(*FI._f(f, device), FI._d(s["X"], device), payload, _i32(seg, device), longest, 0, True, True, True))


# ---- adapters of the ops that take no forest: inputs drawn from the case's forest and per-tree tables -----------------------------------
def _gen_args(f, s, p, device, keys=True):
    pop, L = f[0].shape
    head = [pop, L, s["var_len"], 1, 3, 0.5, 0.5]
    key = [FI._d(np.array([int(p["mut_word"][0]) & 0xFFFFFFFF, 0], np.uint32), device)] if keys else []
    tables = [FI._d(depth2leaf(3), device), FI._d(roulette_uniform([1, 2, 3, 4]), device), FI._d(p["step"][:3], device)]
    return head + key + tables


def _generate(f, s, p, device):
    return FI._o(cu.tree_generate(*_gen_args(f, s, p, device)))


def _generate_offset(f, s, p, device):
    return FI._o(hip.tree_generate_offset(*_gen_args(f, s, p, device), 5))


def _generate_masked(f, s, p, device):
    """the rows of the inactive trees 'are not touched' (include/evogp_hip.h evogp_hip_generate_masked) and the binding's outputs are
    uninitialised: they are zeroed here, on the device, before the comparison"""
    word = _i32(p["mut_word"], device)
    out = hip.tree_generate_masked(*_gen_args(f, s, p, device), 5, word, 1 << 30)
    active = (word < (1 << 30))[:, None]
    return FI._o(tuple(torch.where(active, o, torch.zeros_like(o)) for o in out))


def _generate_masked_hashed(f, s, p, device):
    """every tree active (the words that decide are the op's own): no row is left unwritten"""
    return FI._o(hip.tree_generate_masked_hashed(*_gen_args(f, s, p, device, keys=False), 5, s["seed"], 3, 1 << 31))


def _random_words(f, s, p, device):
    return FI._o(hip.random_words(s["seed"], 2, 6, f[0].shape[0], 0, f[0].shape[0], torch.device(device, torch.cuda.current_device())))


def _fitness_scores(f, s, p, device):
    return FI._o(hip.fitness_scores(FI._d(p["loss"], device), True))


def _select_survivors(f, s, p, device):
    return FI._o(hip.select_survivors(FI._d(p["step"], device), 2, f[0].shape[0] // 2))


def _tournament(f, s, p, device):
    return FI._o(hip.tournament_select(FI._d(p["step"], device), 37, 3, s["seed"], 1))


def _lexicase(f, s, p, device):
    errors = np.ascontiguousarray(p["node_err"][:, :8].T)   # (8 cases, pop), a tenth of them NaN
    return FI._o(hip.lexicase_select(FI._d(errors, device), FI._d(p["step"][:8], device), 33, s["seed"], 2))


def _objectives(f, p, device):
    return FI._d(p["loss"], device), _i32(FI.live_len(f[2]), device)


def _pareto_rank(f, s, p, device):
    return FI._o(hip.pareto_rank(*_objectives(f, p, device), f[0].shape[1] + 1))


def _nsga2_select(f, s, p, device):
    pop = f[0].shape[0]
    return FI._o(hip.nsga2_select(_i32(np.argsort(p["mut_word"], kind="stable"), device), pop // 2, 41, 2, s["seed"], 3))


def _rank_rows(f, s, p, device):
    """segments of 1024, 1025 and pop values: the length follows the case, so the disturbing call has another shape"""
    n = 2049 + f[0].shape[0]
    values = np.resize(p["grad"].ravel(), n).astype(np.float32)
    values[5::97] = values[4::97][:len(values[5::97])]   # ties
    return FI._o(hip.rank_rows(FI._d(values, device), _i32(np.arange(n) % 7, device), _i32([0, 1024, 2049, n], device), 1025))


def _library_select(f, s, p, device):
    L = f[0].shape[1]
    sig = ((p["mut_word"][:, None] % 11) * (np.arange(L)[None, :] % 5 + 1)).astype(np.int64)
    return FI._o(hip.subtree_library_select(FI._d(sig, device), FI._d(np.clip(f[2], 0, L), device), 1, L, 5))


# ---- the two tables --------------------------------------------------------------------------------------------------------------------
BOTH = ("arith_L64", "all_L1024_v40")


def _row(call, cases, select=FI._select_rows, no_b=None):
    return dict(call=call, cases=tuple(cases), select=select, no_b=no_b)


def _fi_cases(op):
    """FI's cases; an op FI can show a multi-output forest only gets this module's long one as its L > 64 case"""
    names = [n for n in FI.cases_for(op) if n in CASES]
    return names + [MULTI_LONG] if FI.TABLE[op]["out"] == "multi" else names


_TWINS = {
    "evogp_hip::tree_evaluate_prepare": _prepare,
    "evogp_cuda::tree_SR_fitness": _sr_fitness, pair_tables.PAIRS: _pairs, gram_tables.GRAM: _gram, neigh_tables.NEIGH: _neigh,
    ST.LOSS: _sim_loss, simulate_sens_tables.NORMAL: _sim_normal, rank_tables.RANK: _rank_stats,
}
CAPTURE = {op: _row(_TWINS.get(op, r["call"]), _fi_cases(op), r["select"]) for op, r in FI.TABLE.items()}
CAPTURE[rank_tables.RANK]["cases"] += ("arith_L64_D2049",)
CAPTURE.update({
    "evogp_cuda::tree_generate": _row(_generate, BOTH), "evogp_hip::tree_generate_offset": _row(_generate_offset, BOTH),
    "evogp_hip::tree_generate_masked": _row(_generate_masked, BOTH),
    "evogp_hip::tree_generate_masked_hashed": _row(_generate_masked_hashed, BOTH),
    "evogp_hip::random_words": _row(_random_words, BOTH, no_b="no tensor argument: a replay has nothing new to read"),
    "evogp_hip::fitness_scores": _row(_fitness_scores, BOTH), "evogp_hip::select_survivors": _row(_select_survivors, BOTH),
    "evogp_hip::tournament_select": _row(_tournament, BOTH), "evogp_hip::lexicase_select": _row(_lexicase, BOTH),
    "evogp_hip::pareto_rank": _row(_pareto_rank, BOTH), "evogp_hip::nsga2_select": _row(_nsga2_select, BOTH),
    rank_tables.ROWS_OP: _row(_rank_rows, BOTH), sublib_tables.SELECT: _row(_library_select, BOTH),
})

# op -> (reason, "file:line").  Empty: reading csrc/torch_ops.cpp and the entry points found no op that waits for the host, allocates
# engine memory on every call or returns host values.  The waits that exist are outside a capture by construction: the one look at a
# new shape's forest (csrc/sr_tc.hip, the function-class observation) and the XCD probe (csrc/common.hip xcc_regions) both test
# hipStreamIsCapturing first, and StreamWorkspaces::get (csrc/common.hip) allocates only for a shape the stream has not seen, which the
# eager calls in front of every capture have shown it.  tree_evaluate_prepare sizes its workspace on the host from (pop, gp_len) alone
# and fills it with launches.  The histogram hook of csrc/sr_tc.hip (evogp_hip_debug_tc_histogram) records a hipMemsetAsync, but it is a
# measurement hook of the debug header and no registered op reaches it.
NOT_CAPTURABLE = {}


def registered_ops():
    return {n.split(".")[0] for n in torch._C._dispatch_get_all_op_names() if n.startswith(("evogp_cuda::", "evogp_hip::"))}
