#!/usr/bin/env python3
"""Record tests/golden/reference_calls.json: the results of the REFERENCE's own device code compiled for the host
(oracle/_ref/libevogp_ref.so, built by oracle/build_ref.py from the reference's sources) on every call that
tests/test_oracle_vs_ref.py makes, so that the test compares the oracle with the reference wherever it runs.

Run where the reference's sources exist:
    python tests/golden/make_reference_calls.py
Every test of tests/test_oracle_vs_ref.py that takes the `reference` fixture runs once, with each of its parameter sets, against
the live library; its assertions hold on the way (the oracle agrees with the reference), and every call is recorded as
{operator:digest of its inputs -> digest of the result} (tests/reference_calls.py).
"""
import inspect
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, os.path.dirname(TESTS))
sys.path.insert(0, TESTS)
from oracle import build_ref  # noqa: E402
from oracle.pyoracle import Oracle  # noqa: E402
from reference_calls import RECORD, RecordingReference  # noqa: E402

import test_oracle_vs_ref  # noqa: E402


def parameter_sets(fn):
    """every parameter set pytest runs fn with (the cross product of its parametrize marks)"""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name != "parametrize":
            continue
        names = [n.strip() for n in m.args[0].split(",")] if isinstance(m.args[0], str) else list(m.args[0])
        axes.append([dict(zip(names, (v,) if len(names) == 1 else tuple(v))) for v in m.args[1]])
    for combo in itertools.product(*axes):
        yield {k: v for d in combo for k, v in d.items()}


def main():
    assert build_ref.available(), f"the reference's sources are not at {build_ref.REF} (set EVOGP_REFERENCE)"
    build_ref.build()
    oracle, rec = Oracle("port"), RecordingReference(Oracle("reference"))
    n = 0
    for name, fn in inspect.getmembers(test_oracle_vs_ref, inspect.isfunction):
        if not name.startswith("test_") or "reference" not in inspect.signature(fn).parameters:
            continue
        for params in parameter_sets(fn):
            fn(oracle=oracle, reference=rec, **params)
            n += 1
    with open(RECORD, "w") as f:
        json.dump({"what": "tests/test_oracle_vs_ref.py's calls of the compiled reference: operator:digest of the inputs -> digest "
                           "of the result (tests/reference_calls.py); written by tests/golden/make_reference_calls.py",
                   "calls": dict(sorted(rec.calls.items()))}, f, indent=0)
        f.write("\n")
    print(f"{n} test cases, {len(rec.calls)} calls -> {RECORD}")


if __name__ == "__main__":
    main()
