"""CPU: the host logic of LexicaseSelection and Forest.SR_case_errors with the numpy twin registered as a test-only CPU kernel
(tests/cpu_lexicase_ops.py), a composed GeneticProgramming step on a CPU forest, and the argument checks of the three new C entry
points, which return before any launch."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cpu_lexicase_ops  # noqa: E402
import lexicase_ref as R  # noqa: E402

cpu_lexicase_ops.register()

from evogp_amd.algorithm import LexicaseSelection, lexicase_epsilon  # noqa: E402
from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device  # noqa: E402
from evogp_amd.tree import utils as _tree_utils  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _cpu_default_device():
    saved = _tree_utils._DEVICE
    set_default_device("cpu")
    yield
    _tree_utils._DEVICE = saved


def _problem(rng, pop=40, D=24, out_len=1):
    d = GenerateDescriptor(max_tree_len=32, input_len=2, output_len=out_len, using_funcs=["+", "-", "*", "/"], max_layer_cnt=4,
                           const_samples=[-1, 0.5, 1])
    f = Forest.random_generate(pop, d, keys=torch.tensor([3, 4]))
    X = torch.from_numpy(rng.uniform(-1, 1, (D, 2)).astype(np.float32))
    y = torch.from_numpy(rng.uniform(-1, 1, (D, out_len)).astype(np.float32))
    return d, f, X, y


def test_case_errors_are_the_transposed_case_major_tensor(rng):
    for out_len in (1, 3):
        _, f, X, y = _problem(rng, out_len=out_len)
        for mse in (True, False):
            e = f.SR_case_errors(X, y, use_MSE=mse)
            assert e.shape == (40, 24) and e.stride() == (1, 40) and e.dtype == torch.float32
            want = R.case_errors(f.batch_forward(X).numpy(), y.numpy(), mse)
            assert np.array_equal(e.t().numpy().view(np.uint32), want.view(np.uint32))
    with pytest.raises(AssertionError):
        f.SR_case_errors(X[:, :1], y)
    with pytest.raises(AssertionError):
        f.SR_case_errors(X, y[:5])


def test_argument_checks():
    X, y = torch.zeros(4, 2), torch.zeros(4, 1)
    with pytest.raises(AssertionError):
        LexicaseSelection()
    with pytest.raises(AssertionError):
        LexicaseSelection(X)
    with pytest.raises(AssertionError):
        LexicaseSelection(X, y, epsilon="mad")
    with pytest.raises(AssertionError):
        LexicaseSelection(X, y, epsilon=-1.0)
    with pytest.raises(AssertionError):
        LexicaseSelection(X, y, downsample_rate=0.0)
    with pytest.raises(AssertionError):
        LexicaseSelection(X, y, survivor_rate=1.5)
    with pytest.raises(AssertionError):
        LexicaseSelection(case_errors=3)


def test_survivors_elites_and_reproducibility(rng):
    _, f, X, y = _problem(rng)
    fit = torch.from_numpy(rng.normal(size=40).astype(np.float32))
    fit[5] = float("nan")
    torch.manual_seed(7)
    sel = LexicaseSelection(X, y, survivor_rate=0.5, elite_cnt=3)
    elites, surv = sel(f, fit)
    assert elites.dtype == surv.dtype == torch.int32 and surv.shape == (20,)
    assert elites.tolist() == torch.topk(torch.nan_to_num(fit, nan=float("-inf")), 3).indices.tolist()
    # the survivors are the twin's events on absolute errors with the MAD epsilon, generation 0
    errors = f.SR_case_errors(X, y, use_MSE=False)
    want = R.select(errors.t().contiguous().numpy(), R.epsilon(errors.numpy()), 20, sel.seed, 0)
    assert surv.tolist() == want.tolist()
    assert sel.generation == 1
    # same torch seed -> same draws; the next call is another generation
    torch.manual_seed(7)
    sel2 = LexicaseSelection(X, y, survivor_rate=0.5, elite_cnt=3)
    assert sel2.seed == sel.seed and sel2(f, fit)[1].tolist() == surv.tolist()
    nxt = sel(f, fit)[1]
    assert nxt.tolist() == R.select(errors.t().contiguous().numpy(), R.epsilon(errors.numpy()), 20, sel.seed, 1).tolist()
    # counts: survivor_cnt / elite_rate
    e, s = LexicaseSelection(X, y, survivor_cnt=7, elite_rate=0.1)(f, fit)
    assert e.shape == (4,) and s.shape == (7,)
    e, s = LexicaseSelection(X, y)(f, fit)
    assert e.shape == (0,) and s.shape == (40,)


def test_epsilon_forms_and_mse(rng):
    _, f, X, y = _problem(rng)
    fit = torch.zeros(40)
    errors = f.SR_case_errors(X, y, use_MSE=True)
    E = errors.t().contiguous().numpy()
    for epsilon, eps in ((0.0, np.zeros(24, np.float32)), (0.25, np.full(24, 0.25, np.float32)),
                         (torch.linspace(0, 1, 24), np.linspace(0, 1, 24).astype(np.float32))):
        sel = LexicaseSelection(X, y, epsilon=epsilon, use_MSE=True, survivor_cnt=30)
        got = sel(f, fit)[1]
        assert got.tolist() == R.select(E, eps, 30, sel.seed, 0).tolist()
    np.testing.assert_array_equal(lexicase_epsilon(errors).numpy(), R.epsilon(errors.numpy()))


def test_downsampling(rng):
    _, f, X, y = _problem(rng, D=50)
    sel = LexicaseSelection(X, y, downsample_rate=0.1, survivor_cnt=25)
    for gen in range(3):
        rows = R.sample_rows(sel.seed, gen, 50, 0.1)
        assert len(rows) == 5 and sel.rows(50, "cpu").tolist() == rows.tolist()
        errors = f.SR_case_errors(X[rows], y[rows], use_MSE=False)
        got = sel(f, torch.zeros(40))[1]
        assert got.tolist() == R.select(errors.t().contiguous().numpy(), R.epsilon(errors.numpy()), 25, sel.seed, gen).tolist()


def test_case_errors_hook(rng):
    _, f, X, y = _problem(rng)
    miss = torch.from_numpy((rng.random((40, 30)) < 0.3).astype(np.float32))   # 0/1 misclassification
    seen = []

    def hook(forest):
        seen.append(forest)
        return miss

    sel = LexicaseSelection(case_errors=hook, epsilon=0.0, survivor_cnt=40)
    got = sel(f, torch.zeros(40))[1]
    assert seen == [f]
    assert got.tolist() == R.select(miss.t().contiguous().numpy(), np.zeros(30, np.float32), 40, sel.seed, 0).tolist()
    # down-sampling picks columns of the hook's errors
    sel = LexicaseSelection(case_errors=hook, epsilon=0.0, survivor_cnt=40, downsample_rate=0.5)
    rows = R.sample_rows(sel.seed, 0, 30, 0.5)
    got = sel(f, torch.zeros(40))[1]
    assert got.tolist() == R.select(miss[:, rows].t().contiguous().numpy(), np.zeros(15, np.float32), 40, sel.seed, 0).tolist()
    with pytest.raises(AssertionError):
        LexicaseSelection(case_errors=lambda forest: torch.zeros(3, 2))(f, torch.zeros(40))


def test_composed_generation_step_on_a_cpu_forest(rng):
    from evogp_amd.algorithm import DefaultCrossover, DefaultMutation, GeneticProgramming

    d, f, X, y = _problem(rng, pop=60)
    torch.manual_seed(3)
    algo = GeneticProgramming(f, DefaultCrossover(), DefaultMutation(0.2, d), LexicaseSelection(X, y, elite_cnt=2, survivor_rate=0.5))
    for _ in range(2):
        fit = -algo.forest.SR_fitness(X, y)
        best = algo.forest[torch.topk(torch.nan_to_num(fit, nan=float("-inf")), 2).indices]
        nxt = algo.step(fit)
        assert nxt.pop_size == 60
        assert torch.equal(nxt.batch_node_value[:2], best.batch_node_value)


def test_sharded_step_is_refused():
    from evogp_amd.parallel import _Population

    sel = LexicaseSelection(case_errors=lambda forest: torch.zeros(4, 2))
    with pytest.raises(TypeError, match="sharded"):
        sel(_Population(4), torch.zeros(4))


def test_argument_errors_without_gpu():
    from evogp_amd import _lib

    L = _lib.lib
    p = 8  # (never dereferenced: the host checks come first)
    assert L.evogp_hip_sr_case_errors(0, 8, 32, 3, 1, 1, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_case_errors(4, 8, 2000, 3, 1, 1, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_case_errors(4, 8, 32, 3, 0, 1, p, p, p, p, p, p, None) == -1
    assert L.evogp_hip_sr_case_errors(4, 8, 32, 3, 1, 1, p, p, p, p, p, None, None) == -2
    assert L.evogp_hip_sr_case_errors(4, 8, 32, 3, 300, 1, p, p, p, p, p, p, None) == -3
    b = ctypes.c_ulonglong(0)
    assert L.evogp_hip_lexicase_workspace_bytes(0, 10, 3, ctypes.byref(b)) == -1
    assert L.evogp_hip_lexicase_workspace_bytes(3, 0, 3, ctypes.byref(b)) == -1
    assert L.evogp_hip_lexicase_workspace_bytes(3, 10, 3, None) == -2
    assert L.evogp_hip_lexicase_select(0, 10, p, p, 3, 1, 2, p, p, None) == -1
    assert L.evogp_hip_lexicase_select(3, 0, p, p, 3, 1, 2, p, p, None) == -1
    assert L.evogp_hip_lexicase_select(3, 10, p, p, 0, 1, 2, None, None, None) == 0     # no event: nothing to do
    assert L.evogp_hip_lexicase_select(3, 10, p, None, 3, 1, 2, p, p, None) == -2
    assert L.evogp_hip_lexicase_select(3, 10, p, p, 3, 1, 2, p, None, None) == -2


def test_product_registers_no_cpu_lexicase_kernel():
    code = ("import torch, evogp_amd\n"
            "try:\n"
            "    torch.ops.evogp_hip.lexicase_select(torch.zeros(2, 3), torch.zeros(2), 3, 0, 0)\n"
            "except (RuntimeError, NotImplementedError) as e:\n"
            "    print('REJECTED', 'lexicase_select' in str(e))\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert "REJECTED True" in r.stdout, r.stdout + r.stderr
