"""The capture tables (tests/capture_tables.py) without a GPU: every registered op is in exactly one of them, every escape carries a
citation that exists, and INTEGRATION.md's "capturable after one eager call" table says what the tables say."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import capture_tables as CT  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_registered_op_is_in_exactly_one_table():
    have, listed = CT.registered_ops(), set(CT.CAPTURE) | set(CT.NOT_CAPTURABLE)
    assert not set(CT.CAPTURE) & set(CT.NOT_CAPTURABLE)
    assert have == listed, (sorted(have - listed), sorted(listed - have))
    assert set(CT.BC.TABLE) <= listed, sorted(set(CT.BC.TABLE) - listed)
    for op, row in CT.CAPTURE.items():
        assert row["cases"] and set(row["cases"]) <= set(CT.CASES), op


def test_every_escape_cites_a_line_that_exists():
    for op, (reason, cite) in CT.NOT_CAPTURABLE.items():
        path, line = cite.rsplit(":", 1)
        with open(os.path.join(ROOT, path)) as fh:
            assert 1 <= int(line) <= len(fh.readlines()), (op, cite)
        assert reason.strip(), op


def test_the_document_says_what_the_tables_say():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        found = dict(re.findall(r"^\| (yes|no) [^|]*\| (.*) \|$", fh.read(), re.M))
    rows = {op: answer for answer, ops in found.items() for op in re.findall(r"`(evogp_(?:hip|cuda)::\w+)`", ops)}
    want = {**{op: "yes" for op in CT.CAPTURE}, **{op: "no" for op in CT.NOT_CAPTURABLE}}
    assert rows == want, (sorted(set(want) - set(rows)), sorted(set(rows) - set(want)), sorted(op for op in rows if want.get(op) != rows[op]))


def test_the_tape_rejects_a_tensor_it_did_not_make():
    """an adapter that makes a tensor with a factory of its own (a fill or a host copy a capture cannot replay) fails in the recording call"""
    with pytest.raises(AssertionError, match="FI._d"):
        with CT.taped(CT.Tape(), "record"):
            torch.arange(3)
    tape = CT.Tape()
    with CT.taped(tape, "record"):
        t = CT.FI._d(np.arange(3), "cpu") + 1
    assert len(tape.tensors) == 1 and t.tolist() == [1, 2, 3]


def test_the_long_multi_output_case():
    c = CT.case(CT.MULTI_LONG)
    n = CT.FI.live_len(c.stale[2])
    assert c.L > 64 and c.out_len >= 2 and c.stale[0].shape == (c.pop, c.L) and (n > 64).sum() >= 3 and (n < 64).any()
