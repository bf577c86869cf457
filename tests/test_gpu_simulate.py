"""GPU: simulation fitness (csrc/sr_simulate.hip).  1: the states bit for bit against tests/simulate_ref.py's float32 formulas stepping
``Forest.forward`` one (trajectory, step, stage) at a time.  2 (the truth that does not descend from the kernel) is
tests/test_simulate_ref.py.  3: the fused loss against a longdouble sum over the materialised states within (B T + 8) 2^-53 sum(term) --
one rounding per square, at most one per addition; not fitted -- NaN exactly where the definition puts it, the same bits on a second call
and on a side stream.  4: the forest invariants and the binding contract.  5: DynamicalSystem.
Measured on an MI355X: the worst error / bound ratios of test 3 are 0.0027 (map), 0.0051 (rk4) and 0.0061 (narx); DESIGN.md 3.33."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import simulate_ref as SIM  # noqa: E402
import simulate_tables as ST  # noqa: E402
import sr_grad_ref as R  # noqa: E402
from grad_trees import ALL_FUNCS, ARITH, out_word, random_forest, random_tree  # noqa: E402
from helpers import fbits  # noqa: E402
from semantic_cases import X0, plant  # noqa: E402
from test_gpu_linear_scaling import _chain  # noqa: E402

from evogp_amd.problem import DynamicalSystem  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

pytestmark = pytest.mark.gpu
PLAIN = [R.F_IF, R.F_ADD, R.F_SUB, R.F_MUL, R.F_DIV, R.F_MAX, R.F_MIN, R.F_LT, R.F_GT, R.F_LE, R.F_GE, R.F_INV, R.F_NEG, R.F_ABS, R.F_SQRT]
FUNCS = {"arith": ARITH, "plain": PLAIN, "all": ALL_FUNCS}
POP, L = 40, 256


def _dev(*arrs):
    return [torch.from_numpy(np.array(a, order="C")).cuda() for a in arrs]


def _balanced(rng, leaves, funcs, var_len):
    """a balanced tree of binary functions: 2 leaves - 1 nodes, a shallow operand stack"""
    if leaves == 1:
        return [(float(rng.integers(var_len)), R.T_VAR, 1) if rng.random() < 0.6 else (np.float32(rng.uniform(0.5, 1.5)), R.T_CONST, 1)]
    left, right = _balanced(rng, leaves // 2, funcs, var_len), _balanced(rng, leaves - leaves // 2, funcs, var_len)
    return [(float(rng.choice(funcs)), R.T_BFUNC, 2 * leaves - 1)] + left + right


@functools.lru_cache(maxsize=None)
def forest(funcs, var_len, out_len):
    """40 random trees in rows of 256 words; single-output forests also hold trees of 1, 63, 64, 65 and 201 nodes and two deep combs"""
    rng = np.random.default_rng([20261126, var_len, out_len, len(FUNCS[funcs])])
    f = random_forest(rng, POP, L, FUNCS[funcs], var_len, out_len, max_depth=8)
    if out_len == 1:
        binary = [R.F_ADD, R.F_SUB, R.F_MUL] + ([R.F_MAX, R.F_MIN] if funcs != "arith" else [])
        planted = [[(0.0, R.T_VAR, 1)], [(np.float32(0.75), R.T_CONST, 1)], _balanced(rng, 32, binary, var_len),
                   [(float(R.F_NEG), R.T_UFUNC, 64)] + _balanced(rng, 32, binary, var_len), _balanced(rng, 33, binary, var_len),
                   _balanced(rng, 101, binary, var_len), _chain(rng, 20, var_len), _chain(rng, 100, var_len)]
        for t, nodes in enumerate(planted):
            FI._set(*f, t, nodes)
        assert sorted(int(n) for n in f[2][:8, 0]) == [1, 1, 41, 63, 64, 65, 201, 201]
    else:
        for t in (0, 1, 2):   # long trees of binary functions: staged in LDS
            nodes = []
            while not 64 < len(nodes) <= L:
                nodes = random_tree(rng, ARITH[:3], var_len, out_len, 8)
            FI._set(*f, t, nodes)
        deep = _chain(rng, 20, var_len)   # an operand stack 21 high, every third function an output: the deep kernel
        for k in range(0, 20, 3):
            deep[k] = (out_word(int(deep[k][0]), k % out_len), R.T_BFUNC | 0x80, deep[k][2])
        FI._set(*f, 4, deep)
        f[2][3, 0] = 0   # a malformed tree
    n = f[2][:, 0]
    assert (n <= 64).sum() >= 5 and (n > 64).sum() >= 2, "trees in the register pair and trees staged in LDS"
    return f


def _case(scheme, funcs, S, U, B, T):
    out_len = 1 if scheme == "narx" else S
    rng = np.random.default_rng([B, T, S, U])
    x0 = rng.uniform(0.5, 1.5, (B, S)).astype(np.float32)
    u = rng.uniform(0.5, 1.5, (B, T, U)).astype(np.float32)
    return forest(funcs, S + U, out_len), Forest(S + U, out_len, *_dev(*forest(funcs, S + U, out_len))), x0, u


# ---- 1. bits.  (scheme, function set, S, U, B, T): S 1 / 3 / 8; U 0 / 2, S + U = 32; B 1 .. 130; T 1, 2, 17 (both ends of the prefetch); S + U 11, 14: tuples of 12, 16
CASES = [
    ("map", "arith", 1, 0, 1, 1),
    ("euler", "arith", 1, 2, 63, 2),
    ("rk4", "plain", 1, 2, 64, 17),
    ("narx", "plain", 3, 2, 65, 2),
    ("map", "plain", 3, 0, 130, 2),
    ("euler", "all", 3, 2, 65, 17),
    ("rk4", "all", 8, 2, 63, 2),
    ("rk4", "arith", 8, 24, 2, 17),
    ("narx", "all", 8, 0, 64, 17),
    ("euler", "plain", 1, 31, 3, 2),
    ("map", "all", 1, 2, 130, 1),
    ("euler", "arith", 3, 8, 2, 2),
    ("map", "plain", 8, 6, 2, 2),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-{}-S{}-U{}-B{}-T{}".format(*c))
def test_states_equal_stepping_forward_bit_for_bit(case):
    scheme, funcs, S, U, B, T = case
    _, fo, x0, u = _case(*case)   # (every forward call below is one launch of the route that exists)
    step = lambda rows: fo.forward(torch.from_numpy(rows).cuda()).cpu().numpy()  # noqa: E731
    want = SIM.simulate(step, POP, x0, u, scheme, 0.1)
    got = fo.SR_simulate(*_dev(x0, u), scheme=scheme, dt=0.1).cpu().numpy()
    assert got.shape == want.shape == (POP, B, T, S) and got.dtype == np.float32
    same = fbits(got) == fbits(want)
    assert same.all(), (np.argwhere(~same)[:4], got[~same][:4], want[~same][:4])
    assert np.isfinite(want).all((1, 2, 3)).sum() >= 4, "trees that live"


# ---- 3. the fused loss -----------------------------------------------------------------------------------------------------------------------
MALFORMED, DIV0, SQUARE, SWALLOW = 8, 9, 10, 11


@pytest.mark.parametrize("scheme,S,U,B,T", [("map", 1, 0, 65, 8), ("rk4", 3, 2, 130, 5), ("narx", 3, 1, 64, 5)])
def test_loss_equals_the_longdouble_sum_over_the_states(scheme, S, U, B, T):
    f = [np.array(a) for a in forest("plain", S + U, 1 if scheme == "narx" else S)]
    single = scheme != "rk4"
    if single:
        f[2][MALFORMED, 0] = 0
        plant(*f, DIV0, ("div", X0, ("sub", X0, X0)))
        plant(*f, SQUARE, ("mul", X0, X0))
        plant(*f, SWALLOW, ("max", ("div", X0, ("sub", X0, X0)), ("c", np.float32(0.5))))
    rng = np.random.default_rng([3, B, T])
    x0 = rng.uniform(0.5, 1.0, (B, S)).astype(np.float32)   # (below 1: x0 * x0 under map contracts from every start but the first)
    x0[0] = 10.0   # x0 * x0 under map: 1e2, 1e4, 1e8, 1e16, 1e32, inf
    u = rng.uniform(0.5, 1.5, (B, T, U)).astype(np.float32)
    target = rng.uniform(0.5, 1.5, (B, T) if scheme == "narx" else (B, T, S)).astype(np.float32)
    fo = Forest(S + U, 1 if scheme == "narx" else S, *_dev(*f))
    args = _dev(x0, u, target)
    states = fo.SR_simulate(args[0], args[1], scheme=scheme, dt=0.1).cpu().numpy()
    call = lambda: fo.SR_simulation_loss(*args, scheme=scheme, dt=0.1)  # noqa: E731
    loss = call().cpu().numpy()
    SC = loss.shape[1]
    assert loss.shape == (POP, 1 if scheme == "narx" else S) and loss.dtype == np.float64
    want = SIM.loss(states, target, scheme == "narx")
    dead = np.isnan(states).any((1, 2, 3))
    assert np.array_equal(np.isnan(loss), np.repeat(dead[:, None], SC, 1)) and 0 < dead.sum() <= POP - 4
    bound = (B * T + 8) * 2.0 ** -53 * want
    err = np.abs(loss[~dead].astype(np.longdouble) - want[~dead])
    assert (err <= bound[~dead]).all(), (err / bound[~dead]).max()
    print(f"{scheme}: worst error / bound {float((err / np.maximum(bound[~dead], np.longdouble(1e-300))).max()):.3g}")
    if single:
        assert dead[[MALFORMED, DIV0]].all() and not dead[SWALLOW] and np.isnan(states[MALFORMED]).all() and np.isnan(states[DIV0]).all()
        if scheme == "map":   # (eight steps: the square overflows at the sixth)
            assert dead[SQUARE] and np.isfinite(states[SQUARE, 0, :5]).all() and np.isnan(states[SQUARE, 0, 5:]).all() and np.isfinite(states[SQUARE, 1:]).all()
            assert (states[SWALLOW] == 0.5).all()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        side = call()
    stream.synchronize()
    for other in (call(), side):
        assert np.array_equal(FI._bits(other.cpu().numpy()), FI._bits(loss))


# ---- 4. the tables ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op,case", [(op, c) for op in (ST.SIMULATE, ST.LOSS) for c in FI.cases_for(op)])
def test_op_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("op", [ST.SIMULATE, ST.LOSS])
def test_binding_contract(op):
    ST.BC.test_valid_call_and_one_fault_at_a_time(op)


# ---- 5. the problem class --------------------------------------------------------------------------------------------------------------------
def test_dynamical_system_ranks_the_true_oscillator_first():
    rng = np.random.default_rng(9)
    f = [np.array(a) for a in random_forest(rng, POP, 64, ARITH + [R.F_NEG, R.F_MAX], 2, 2, max_depth=4)]
    true = 5   # x0' = -x1, x1' = x0: a root that adds nothing over neg[out 0](x1) and max[out 1](x0, x0)
    FI._set(*f, true, [(float(R.F_ADD), R.T_BFUNC, 6), (out_word(R.F_NEG, 0), R.T_UFUNC | 0x80, 2), (1.0, R.T_VAR, 1),
                       (out_word(R.F_MAX, 1), R.T_BFUNC | 0x80, 3), (0.0, R.T_VAR, 1), (0.0, R.T_VAR, 1)])
    n, dt = 200, 0.1
    angle = rng.uniform(0, 6.28) + dt * np.arange(n)
    series = torch.from_numpy(np.stack([np.cos(angle), np.sin(angle)], 1).astype(np.float32)).cuda()
    problem = DynamicalSystem.from_series(series, None, window=16, stride=2, scheme="rk4", dt=dt)
    fo = Forest(2, 2, *_dev(*f))
    fitness = problem.evaluate(fo)
    loss = fo.SR_simulation_loss(problem.x0, None, problem.target, "rk4", dt)
    want = -(loss / problem.state_scale).sum(1)
    want = torch.where(torch.isnan(want), torch.full_like(want, -np.inf), want).to(torch.float32)
    assert torch.equal(fitness, want) and fitness.shape == (POP,)
    others = torch.cat([fitness[:true], fitness[true + 1:]])
    assert float(fitness[true]) > float(others.max()) and float(fitness[true]) > -1e-8
