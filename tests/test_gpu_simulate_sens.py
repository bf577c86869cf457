"""GPU: constant tuning under simulation fitness (csrc/sr_simulate_sens.hip).  1: states and sensitivities bit for bit against
tests/simulate_sens_ref.py's float32 restatement.  2: the sensitivities against finite differences of the float64 restatement, within a
bound taken from the reference alone (tests/test_simulate_sens_ref.py smooth_case).  3: the fused normal equations against a longdouble
sum over the materialised arrays within (T SC + ntiles + 16) 2^-24 sum|term| -- one rounding per addition of a lane's (t, s) terms, of the
butterfly, of the tiles, and the division; not fitted.  4: the forest invariants and the binding contract.  5: the tuner end to end."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import simulate_sens_ref as SR  # noqa: E402
import simulate_sens_tables as SST  # noqa: E402
import sr_grad_ref as R  # noqa: E402
import test_simulate_sens_ref as CPU  # noqa: E402
from grad_trees import ARITH, out_word, random_forest  # noqa: E402
from test_gpu_linear_scaling import _chain  # noqa: E402
from test_gpu_simulate import PLAIN, _balanced, _dev  # noqa: E402

from evogp_amd.problem import DynamicalSystem  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402
from evogp_amd.tree.forest import SIM_SCHEMES  # noqa: E402

pytestmark = pytest.mark.gpu
FUNCS = {"arith": ARITH, "plain": PLAIN}
POP, L, F = 40, 128, np.float32
MALFORMED, SQUARE = {1: 10, 0: 2}, 20   # the malformed row of single- / multi-output forests; the row test 3 plants x0 * x0 in
normal_eq = torch.ops.evogp_hip.tree_SR_simulation_normal_eq


def _consts(rng, n):
    """x0 * ((c + c) + ...): n constants, the first 8 optimised"""
    e = CPU.const(rng.uniform(0.5, 1.5))
    for _ in range(n - 1):
        e = CPU.node(R.F_ADD, e, CPU.const(rng.uniform(0.5, 1.5)))
    return CPU.node(R.F_MUL, e, CPU.var(0))


@functools.lru_cache(maxsize=None)
def forest(funcs, var_len, out_len):
    """40 random trees in rows of 128 words.  Planted, single output: 1 node, nc = 0 / 1 / 4 / 5 / 8 / 9, 64 / 65 / 101 nodes, a comb 21
    operands high, a malformed row; several outputs: 66 nodes, a deep comb whose OUT nodes sit mid-tree, a malformed row"""
    rng = np.random.default_rng([20261127, var_len, out_len, len(FUNCS[funcs])])
    f = random_forest(rng, POP, L, FUNCS[funcs], var_len, out_len, max_depth=5)
    binary = [R.F_ADD, R.F_SUB, R.F_MUL]
    if out_len == 1:
        planted = [CPU.var(0), CPU.const(0.75)] + [_consts(rng, n) for n in (4, 5, 8, 9)]
        planted += [[(float(R.F_NEG), R.T_UFUNC, 64)] + _balanced(rng, 32, binary, var_len), _balanced(rng, 33, binary, var_len),
                    _balanced(rng, 51, binary, var_len), _chain(rng, 20, var_len)]
    else:
        deep = _chain(rng, 20, var_len)
        for k in range(1, 20, 3):
            deep[k] = (out_word(int(deep[k][0]), k % out_len), R.T_BFUNC | 0x80, deep[k][2])
        planted = [CPU.node(R.F_ADD, _balanced(rng, 33, binary, var_len), CPU.node(R.F_MUL, CPU.var(0), CPU.const(0.5), out=0)), deep]
    for t, nodes in enumerate(planted):
        FI._set(*f, t, nodes)
    f[2][MALFORMED[out_len == 1], 0] = 0
    return f


def _case(scheme, funcs, S, U, B, T, seed=0):
    out_len = 1 if scheme == "narx" else S
    rng = np.random.default_rng([seed, B, T, S, U])
    f = [np.array(a) for a in forest(funcs, S + U, out_len)]
    return f, out_len, rng.uniform(0.5, 1.0, (B, S)).astype(F), rng.uniform(0.5, 1.5, (B, T, U)).astype(F), rng


# ---- 1. bits.  (scheme, function set, S, U, B, T): every scheme; S 1 / 3 / 8; U 0 / 2 / 24; B at tile ends, several waves; T at both ends of the prefetch
CASES = [("map", "arith", 1, 0, 1, 1), ("euler", "plain", 1, 2, 63, 2), ("rk4", "plain", 1, 2, 65, 17), ("narx", "plain", 3, 2, 65, 2),
         ("map", "plain", 3, 0, 130, 2), ("euler", "arith", 3, 2, 63, 17), ("rk4", "arith", 8, 2, 130, 2), ("narx", "arith", 8, 0, 1, 17),
         ("map", "plain", 8, 2, 65, 1), ("rk4", "plain", 3, 0, 2, 2), ("euler", "plain", 8, 24, 2, 2)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-{}-S{}-U{}-B{}-T{}".format(*c))
def test_states_and_sensitivities_equal_the_restatement_bit_for_bit(case):
    scheme, _, S, U, B, T = case
    f, out_len, x0, u, _ = _case(*case)
    fo = Forest(S + U, out_len, *_dev(*f))
    want_x, want_s, _ = SR.simulate(f, S + U, x0, u, scheme, 0.1)
    states, sens, _ = fo.SR_simulation_sensitivities(*_dev(x0, u), scheme=scheme, dt=0.1)
    assert np.array_equal(FI._bits(states.cpu().numpy()), FI._bits(fo.SR_simulate(*_dev(x0, u), scheme=scheme, dt=0.1).cpu().numpy()))
    got_s = sens.cpu().numpy()
    assert got_s.shape == (POP, B, T, S, 8) and got_s.dtype == np.float32 and np.array_equal(states.cpu().numpy(), want_x, equal_nan=True)
    same = (got_s == want_s) | (np.isnan(got_s) & np.isnan(want_s))
    assert same.all(), (np.argwhere(~same)[:4], got_s[~same][:4], want_s[~same][:4])
    assert (np.abs(np.nan_to_num(want_s)) > 0).any((1, 2, 3, 4)).sum() >= 4, "trees that live and have constants"


# ---- 2. truth that does not descend from the rule table (measured on an MI355X: worst error / bound 0.25 on each)
@pytest.mark.parametrize("name", list(CPU.SMOOTH))
def test_sensitivities_equal_finite_differences_of_the_float64_states(name):
    c = CPU.smooth_case(name)
    fo = Forest(c["S"] + c["U"], c["S"], *_dev(*c["forest"]))
    sens = fo.SR_simulation_sensitivities(*_dev(c["x0"], c["u"]), scheme=c["scheme"], dt=c["dt"])[1].cpu().numpy()[0]
    ok = np.isfinite(c["fd"])
    err = np.abs(sens[..., :c["nc"]].astype(np.float64) - c["fd"])[ok].max()
    print(f"{name}: worst error / bound {err / c['bound']:.3g}")
    assert ok.mean() >= 0.9 and err <= c["bound"] and (sens[..., c["nc"]:] == 0).all()


# ---- 3. the fused op (measured: worst error / bound 0.13 map, 0.065 rk4, 0.065 narx)
@pytest.mark.parametrize("scheme,S,U,B,T", [("map", 1, 0, 65, 8), ("rk4", 3, 2, 130, 5), ("narx", 3, 1, 64, 5)])
def test_normal_equations_equal_the_longdouble_sum_over_the_sensitivities(scheme, S, U, B, T):
    f, out_len, x0, u, rng = _case(scheme, "plain", S, U, B, T, seed=3)
    FI._set(*f, SQUARE, CPU.node(R.F_MUL, CPU.var(0), CPU.var(0)))   # under map from 10: 1e2, 1e4, 1e8, 1e16, 1e32, inf
    x0[0] = 10.0
    SC = 1 if scheme == "narx" else S
    target, weight = rng.uniform(0.5, 1.5, (B, T, SC)).astype(F), np.linspace(0.5, 2.0, SC).astype(F)
    fo = Forest(S + U, out_len, *_dev(*f))
    args = _dev(x0, u, target[..., 0] if scheme == "narx" else target)
    states, sens, index = (a.cpu().numpy() for a in fo.SR_simulation_sensitivities(args[0], args[1], scheme=scheme, dt=0.1))
    call = lambda: normal_eq(*fo._tensors(), *args, _dev(weight)[0], SIM_SCHEMES[scheme], 0.1)  # noqa: E731
    loss64, loss32, normal = (a.cpu().numpy() for a in call())
    assert np.array_equal(FI._bits(loss64), FI._bits(fo.SR_simulation_loss(*args, scheme=scheme, dt=0.1).cpu().numpy()))
    dead = np.isnan(states).any((1, 2, 3))
    assert dead[MALFORMED[out_len == 1]] and (dead[SQUARE] or scheme != "map") and dead.sum() <= POP - 4
    assert np.isnan(loss64[dead]).all() and np.isnan(loss32[dead]).all() and (normal[dead] == 0).all()
    want32 = functools.reduce(lambda acc, s: acc + np.float64(weight[s]) * loss64[:, s], range(SC), np.zeros(POP))
    assert np.array_equal(FI._bits(loss32[~dead]), FI._bits(want32.astype(F)[~dead]))
    A, b = (a.cpu().numpy() for a in fo.SR_simulation_normal_equations(*args, scheme=scheme, dt=0.1, state_weight=weight)[1:3])
    eps, worst = (T * SC + (B + 63) // 64 + 16) * 2.0 ** -24, 0.0
    for t in np.flatnonzero(~dead):
        nc = int((index[t] >= 0).sum())
        assert (A[t][nc:] == 0).all() and (A[t][:, nc:] == 0).all() and (b[t][nc:] == 0).all()
        wA, wb, sA, sb = SR.normal_equations(states[t][..., :SC], sens[t][..., :SC, :], target, weight)
        for got, want, scale in ((A[t], wA, sA), (b[t], wb, sb)):
            fin = np.isfinite(got) & np.isfinite(want.astype(np.float64))
            err = np.abs(got.astype(np.longdouble) - want)[fin]
            assert (err <= eps * scale[fin]).all(), (t, got, want)
            worst = max([worst] + list((err / np.maximum(eps * scale[fin], np.longdouble(1e-300))).astype(float)))
    print(f"{scheme}: worst error / bound {worst:.3g}")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        side = call()
    stream.synchronize()
    for other in (call(), side):
        assert all(np.array_equal(FI._bits(x.cpu().numpy()), FI._bits(y)) for x, y in zip(other, (loss64, loss32, normal)))


# ---- 4. the tables
@pytest.mark.parametrize("op,case", [(op, c) for op in (SST.SENS, SST.NORMAL) for c in FI.cases_for(op)])
def test_op_keeps_the_invariants(op, case):
    FI.check(op, FI.TABLE[op], FI.build_case(case), "cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("op", [SST.SENS, SST.NORMAL])
def test_binding_contract(op):
    SST.BC.test_valid_call_and_one_fault_at_a_time(op)


# ---- 5. end to end
@pytest.mark.parametrize("scheme,S", [("euler", 1), ("rk4", 2)])
def test_tuning_never_raises_a_loss_and_moves_only_the_optimised_constants(scheme, S):
    f, _, x0, u, rng = _case(scheme, "plain", S, 1, 65, 6)
    fo = Forest(S + 1, S, *_dev(*f))
    args = _dev(x0, u, rng.uniform(0.5, 1.5, (65, 6, S)).astype(F))
    start = normal_eq(*fo._tensors(), *args, torch.ones(S, device="cuda"), SIM_SCHEMES[scheme], 0.1)[1].cpu().numpy()
    tuned, loss = fo.optimize_simulation_constants(*args, scheme=scheme, dt=0.1, steps=5)
    loss, ok = loss.cpu().numpy(), np.isfinite(start)
    assert np.array_equal(np.isnan(start), np.isnan(loss)) and (loss[ok] <= start[ok]).all() and (loss[ok] < start[ok]).sum() >= 4
    index = fo.SR_simulation_sensitivities(args[0], args[1], scheme=scheme, dt=0.1)[2].cpu().numpy()
    moved = FI._bits(tuned.batch_node_value.cpu().numpy()) != FI._bits(f[0])
    allowed = (np.arange(L)[None, None, :] == index[:, :, None]).any(1)
    assert moved.any() and not (moved & ~allowed).any()


@pytest.mark.parametrize("scheme", ["map", "rk4"])
def test_tuner_identifies_the_planted_system_as_the_restatement_does(scheme):
    """10 LM steps from (0.8, 0.4) on data from (0.9, 0.5): the device's loss ratio within 10 x the ratio the CPU's run of the same rule
    records (tests/test_simulate_sens_ref.py: 0 for map, 1.06e-12 for rk4; measured on an MI355X: 0 and 1.18e-12)"""
    c = CPU.lm_case(scheme)
    tuned, loss = Forest(2, 1, *_dev(*c["forest"])).optimize_simulation_constants(*_dev(c["x0"], c["u"], c["target"]), scheme=scheme, dt=c["dt"], steps=10)
    h = c["history"]
    print(f"{scheme}: device ratio {float(loss[0]) / h[0]:.3g}, CPU ratio {h[-1] / h[0]:.3g}")
    assert float(loss[0]) / h[0] <= 10 * h[-1] / h[0]
    start = c["forest"][0][0][c["forest"][1][0] == R.T_CONST]
    assert np.allclose(tuned.batch_node_value.cpu().numpy()[0][c["forest"][1][0] == R.T_CONST], np.where(start > 0.6, 0.9, 0.5), rtol=1e-4)


def test_dynamical_system_tunes_with_its_state_scale():
    c = CPU.smooth_case("oscillator")
    fo, (x0,) = Forest(2, 2, *_dev(*c["forest"])), _dev(c["x0"])
    target = fo.SR_simulate(x0, None, 17, "euler", c["dt"])[0] * 1.1
    problem = DynamicalSystem(x0, None, target, "euler", c["dt"], const_opt_steps=2)
    tuned, loss = problem.optimize_constants(fo, steps=2)
    want, want_loss = fo.optimize_simulation_constants(x0, None, target, "euler", c["dt"], 2, 1e-3, (1.0 / problem.state_scale).to(torch.float32))
    assert torch.equal(tuned.batch_node_value, want.batch_node_value) and torch.equal(loss, want_loss)
    assert torch.equal(problem.optimize(fo).batch_node_value, want.batch_node_value)
