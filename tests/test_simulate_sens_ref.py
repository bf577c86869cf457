"""CPU: the restated simulation sensitivities (tests/simulate_sens_ref.py) against truths that do not descend from it: its float64 mode
against central differences of its own float64 states on planted smooth systems, its float32 states against tests/simulate_ref.py on the C
oracle, and the LM rule it drives on two planted identification problems.  The planted cases are shared with tests/test_gpu_simulate_sens.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import forest_invariance as FI  # noqa: E402
import simulate_ref as SIM  # noqa: E402
import simulate_sens_ref as SR  # noqa: E402
import simulate_sens_tables  # noqa: E402,F401  (the ops' rows of the invariance and binding tables exist in every collection)
import sr_grad_ref as R  # noqa: E402
from grad_trees import ARITH, out_word, random_forest  # noqa: E402

F = np.float32
var = lambda k: [(float(k), R.T_VAR, 1)]  # noqa: E731
const = lambda v: [(F(v), R.T_CONST, 1)]  # noqa: E731


def node(f, *kids, out=None):
    typ, n = (R.T_UFUNC if f >= R.F_SIN else R.T_BFUNC), 1 + sum(len(k) for k in kids)
    return [(float(f), typ, n) if out is None else (out_word(f, out), typ | 0x80, n)] + [w for k in kids for w in k]


def one_tree(nodes):
    f = np.zeros((1, 32), F), np.zeros((1, 32), np.int16), np.zeros((1, 32), np.int16)
    FI._set(*f, 0, nodes)
    return f


# ---- planted smooth systems, contracting, away from kinks and poles: name -> (nodes, scheme, S, U, dt)
SMOOTH = {
    # x0' = c2 x1, x1' = c0 x0 - c1 x1: a damped oscillator, two OUT nodes under a root that adds nothing
    "oscillator": (node(R.F_ADD, node(R.F_MUL, var(1), const(1.0), out=0),
                        node(R.F_SUB, node(R.F_MUL, const(-0.5), var(0)), node(R.F_MUL, const(0.3), var(1)), out=1)), "euler", 2, 0, 0.1),
    # x+ = (c0 x) (c1 - x): the logistic map at r = 2.5, which contracts to 0.6
    "logistic": (node(R.F_MUL, node(R.F_MUL, const(2.5), var(0)), node(R.F_SUB, const(1.0), var(0))), "map", 1, 0, 1.0),
    # x' = c0 tanh(u) - (c1 x + c2 sin(x) exp(-x))
    "transcendental": (node(R.F_SUB, node(R.F_MUL, const(0.7), node(R.F_TANH, var(1))),
                            node(R.F_ADD, node(R.F_MUL, const(0.8), var(0)),
                                 node(R.F_MUL, node(R.F_MUL, const(0.4), node(R.F_SIN, var(0))), node(R.F_EXP, node(R.F_NEG, var(0)))))),
                       "rk4", 1, 1, 0.1),
}


@functools.lru_cache(maxsize=None)
def smooth_case(name):
    """forest, data, and the CPU's views of the sensitivities: differences of the float64 states (the truth), the float64 and the float32
    restatement; ``bound``: what a float32 evaluation of the rule may miss the truth by, from the reference alone -- 4 x the float32
    restatement's own worst deviation from the float64 one (the 4: few-ulp differences between numpy's and the device's library
    functions) plus the finite-difference error (the float64 restatement against the differences)"""
    nodes, scheme, S, U, dt = SMOOTH[name]
    rng = np.random.default_rng(len(name))
    forest = one_tree(nodes)
    x0, u = rng.uniform(0.2, 0.8, (5, S)).astype(F), rng.uniform(0.5, 1.5, (5, 17, U)).astype(F)
    fd = SR.finite_differences(forest, S + U, x0, u, scheme, dt, 0)
    nc = fd.shape[-1]
    d64, d32 = (SR.simulate(forest, S + U, x0, u, scheme, dt, t)[1][0] for t in (np.float64, F))
    bound = 4 * np.abs(d32[..., :nc].astype(np.float64) - d64[..., :nc]).max() + np.abs(d64[..., :nc] - fd).max()
    return dict(forest=forest, scheme=scheme, S=S, U=U, dt=dt, x0=x0, u=u, nc=nc, fd=fd, d64=d64, bound=bound)


@pytest.mark.parametrize("name", list(SMOOTH))
def test_float64_restatement_equals_finite_differences(name):
    c = smooth_case(name)
    assert np.isfinite(c["fd"]).mean() >= 0.9, "at least 90 % of the entries are compared"
    scale, err = np.abs(c["fd"]).max(), np.abs(c["d64"][..., :c["nc"]] - c["fd"]).max()
    print(f"{name}: |dual64 - fd| {err:.3g} at scale {scale:.3g}; float32 bound {c['bound']:.3g}")
    # central differences at h = 1e-6 on O(1) states: truncation h^2 f''' / 6 ~ 1e-12, cancellation 2^-53 |x| / h ~ 1e-10
    assert scale > 0.1 and err <= 1e-8 * max(scale, 1.0) and (c["d64"][..., c["nc"]:] == 0).all()


@pytest.mark.parametrize("scheme,S", [("map", 1), ("euler", 1), ("rk4", 1), ("narx", 3)])
def test_restated_states_equal_simulate_ref_on_the_oracle(scheme, S):
    from oracle.pyoracle import Oracle

    oracle, rng = Oracle("port"), np.random.default_rng(S)
    f = random_forest(rng, 12, 32, ARITH + [R.F_NEG, R.F_MAX, R.F_ABS], S + 1, 1, max_depth=4)
    x0, u = rng.uniform(0.5, 1.5, (4, S)).astype(F), rng.uniform(0.5, 1.5, (4, 5, 1)).astype(F)
    want = SIM.simulate(lambda rows: oracle.evaluate(*f, rows, 1), 12, x0, u, scheme, 0.1)
    assert np.array_equal(SR.simulate(f, S + 1, x0, u, scheme, 0.1)[0], want, equal_nan=True) and np.isfinite(want).all((1, 2, 3)).sum() >= 4


# ---- planted identification problems: x+ = c0 x + c1 u (map), dx/dt = c1 u - c0 x (rk4); true (0.9, 0.5), started at (0.8, 0.4)
def _linear(c0, c1, ode):
    return node(R.F_SUB if ode else R.F_ADD, *[node(R.F_MUL, const(c), var(v)) for c, v in ([(c1, 1), (c0, 0)] if ode else [(c0, 0), (c1, 1)])])


@functools.lru_cache(maxsize=None)
def lm_case(scheme):
    """the start forest, data from the true system, and the losses of the CPU's run of 10 LM steps"""
    ode = scheme == "rk4"
    rng = np.random.default_rng(5 + ode)
    x0, u, dt = rng.uniform(0.5, 1.5, (8, 1)).astype(F), rng.uniform(-1, 1, (8, 16, 1)).astype(F), (0.1 if ode else 1.0)
    target = SR.simulate(one_tree(_linear(0.9, 0.5, ode)), 2, x0, u, scheme, dt)[0][0]
    start = one_tree(_linear(0.8, 0.4, ode))
    return dict(forest=start, x0=x0, u=u, target=target, dt=dt, history=SR.lm_tune(start, 2, x0, u, target, scheme, dt, 10))


@pytest.mark.parametrize("scheme", ["map", "rk4"])
def test_lm_on_the_restatement_identifies_the_planted_system(scheme):
    h = lm_case(scheme)["history"]
    print(f"{scheme}: loss {h[0]:.3g} -> {h[-1]:.3g}, ratio {h[-1] / h[0]:.3g}")   # recorded: 0 (map), 1.06e-12 (rk4)
    assert all(b <= a for a, b in zip(h, h[1:])) and h[-1] <= 1e-6 * h[0]
