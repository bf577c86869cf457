"""GPU: every registered op, captured into a HIP graph after eager calls on the stream, replays to the bits of the eager call
(tests/capture_tables.py: CAPTURE has 70 rows, NOT_CAPTURABLE 0; 153 (op, case) pairs; completeness is tests/test_capture_tables_host.py's).  Per (op, case), on one side stream and with a strictly linear capture:

  eager     two calls on input set A give equal bits (want_A); one on input set B, the same shapes with the rows permuted, gives want_B,
            which differs from want_A
  capture   one call, the argument tensors holding A
  replay 1  outputs poisoned, replay: want_A
  replay 2  after eager calls on the same stream of the same op on other shapes (another pop, a gp_len across 64, a larger one so that the
            workspaces regrow and the counter ring advances), of tree_SR_fitness and of tree_SR_gradient; outputs poisoned, replay: want_A
  replay 3  B copied into the captured argument tensors, outputs poisoned, replay: want_B (a decision the host took from the data at
            capture time would show here)

Floats compare as bit patterns with the NaNs collapsed (helpers.fbits), everything else exactly: no tolerance.  An in-place op's outputs
are its arguments: they are restored from pristine clones instead of poisoned, and the pristine bits must differ from want."""
import os
import sys

import numpy as np
import pytest
import torch

import evogp_amd  # noqa: F401  (registers the ops)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import capture_tables as CT  # noqa: E402
import forest_invariance as FI  # noqa: E402

pytestmark = pytest.mark.gpu
POISON = 0xA5


def _host(outs):
    return [o.detach().cpu().numpy() for o in outs]


def _bits(a):
    return a.view(np.uint8) if a.dtype == np.bool_ else FI._bits(a)


def _differ(got, want):
    return any(g.shape != w.shape or not np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _same(op, what, got, want):
    assert len(got) == len(want), f"{op}: {what}: {len(got)} outputs against {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == w.dtype, f"{op}: {what}: output {k} is {g.dtype}{g.shape}, expected {w.dtype}{w.shape}"
        diff = np.argwhere(_bits(g) != _bits(w))
        if len(diff):
            words = ", ".join(f"{tuple(int(i) for i in d)}: {g[tuple(d)]!r} != {w[tuple(d)]!r}" for d in diff[:4])
            raise AssertionError(f"{op}: {what}: output {k} differs from the eager call in {len(diff)} words, first {words}")


def _poisoned(w):
    return np.full(w.nbytes, POISON, np.uint8).view(w.dtype).reshape(w.shape)


CASES = [(op, name) for op in sorted(CT.CAPTURE) for name in CT.CAPTURE[op]["cases"]]


@pytest.mark.parametrize("op,name", CASES)
def test_replay_equals_eager(op, name):
    row, c, dev = CT.CAPTURE[op], CT.case(name), "cuda"
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        args, call, outputs_of, inplace, first = CT.build(op, c, dev)
        want_1 = _host(first)
        if inplace:
            CT.restore(args)
        want_a = _host(outputs_of(call(args)))
        _same(op, "the second eager call", want_a, want_1)
        assert any(w.size for w in want_a), f"{op}: no output to compare"
        want_b = args_b = None
        if row["no_b"] is None:
            args_b, _, _, _, first_b = CT.build(op, c, dev, "B")
            want_b = _host(first_b)
            assert _differ(want_b, want_a), f"{op} on {name}: input sets A and B give the same outputs"
        held = {t.data_ptr() for t in args.tensors if t.numel()}
        if inplace:
            CT.restore(args)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = outputs_of(call(args))

        def replay(k, want, source=None):
            if inplace or source is not None:
                CT.restore(args, source)
            fresh = [o for o in outs if o.numel() and o.data_ptr() not in held]
            for o, w in zip(outs, want):
                if o.numel() and o.data_ptr() not in held:
                    assert not np.array_equal(_bits(_poisoned(w)), _bits(w)), f"{op}: the poison pattern equals the expected output"
                    CT._raw(o).fill_(POISON)
            if inplace:
                was = {t.data_ptr(): q for t, q in zip(args.tensors, _host((source or args).pristine))}
                pairs = [(was[o.data_ptr()], w) for o, w in zip(outs, want) if o.data_ptr() in held]
                assert _differ([a for a, _ in pairs], [b for _, b in pairs]), f"{op}: the in-place call changes nothing"
            else:
                assert fresh, f"{op}: no output was poisoned"
            graph.replay()
            side.synchronize()
            _same(op, f"replay {k} on {name}", _host(outs), want)

        replay(1, want_a)
        for d in CT.DISTURB[name]:
            CT.eager(op, CT.build_case(*d), dev)
        d = CT.build_case(*CT.OTHER[name])
        FI._sr_fitness(d.stale, d.shared, d.per_tree, dev)
        FI.TABLE["evogp_hip::tree_SR_gradient"]["call"](d.stale, d.shared, d.per_tree, dev)
        replay(2, want_a)
        if want_b is not None:
            replay(3, want_b, args_b)
        else:
            replay(3, want_a)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()

