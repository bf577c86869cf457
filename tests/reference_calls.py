"""The reference's own device code compiled for the host (oracle/_ref), replayed from a record of the calls the tests make.

tests/golden/reference_calls.json maps every call of tests/test_oracle_vs_ref.py -- the operator and a digest of exactly the inputs
the library receives -- to a digest of what the compiled reference returned for it (tests/golden/make_reference_calls.py writes it
where the reference's sources exist).  The comparison is the one the tests made against the live library: the live prefix
[0, len) of every (value, type, size) row bit for bit (the reference leaves the tail uninitialised), float results bit for bit
with every NaN mapped to one pattern (helpers.fbits).  A call whose inputs were never recorded is an error, never a pass.
"""
import hashlib
import json
import os

import numpy as np

from helpers import bits, fbits
from oracle.pyoracle import live_mask

RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_calls.json")

# the argument dtypes of oracle/pyoracle.py's wrappers: what the C functions receive (None: a scalar passed as an int / a C int)
_F32, _I16, _I32, _U32 = np.float32, np.int16, np.int32, np.uint32
_FOREST = (_F32, _I16, _I16)
SIGNATURES = {
    "generate": (None, None, None, None, _F32, _F32, _U32, _F32, _F32, _F32),
    "evaluate": _FOREST + (_F32, None),
    "sr_fitness": _FOREST + (_F32, _F32, None),
    "crossover": _FOREST + (_I32, _I32, _I32, _I32),
    "mutate": _FOREST + (_I32, _F32, _I16, _I16),
}
FOREST_RESULTS = ("generate", "crossover", "mutate")


def call_key(op, args):
    """op + a digest of the arguments as the library sees them"""
    sig = SIGNATURES[op]
    assert len(args) == len(sig), f"{op}: {len(args)} arguments, the record knows {len(sig)}"
    h = hashlib.sha256(op.encode())
    for a, dt in zip(args, sig):
        if dt is None:
            h.update(b"i" + repr(int(a)).encode())
        else:
            x = np.ascontiguousarray(a, dtype=dt)
            h.update(f"a{x.dtype.str}{x.shape}".encode())
            h.update(x.tobytes())
    return f"{op}:{h.hexdigest()[:32]}"


def result_digest(op, out):
    """digest of the part of a result the comparison looks at"""
    h = hashlib.sha256()
    if op in FOREST_RESULTS:
        value, type_, size = out
        m = live_mask(size)
        for x in (np.asarray(size)[:, 0], bits(value)[m], np.asarray(type_)[m], np.asarray(size)[m]):
            x = np.ascontiguousarray(x)
            h.update(f"{x.dtype.str}{x.shape}".encode())
            h.update(x.tobytes())
    else:
        x = fbits(out)
        h.update(f"{x.shape}".encode())
        h.update(x.tobytes())
    return h.hexdigest()[:32]


class RecordedReference:
    """Oracle("reference")'s operators; each returns the digest of the reference's result for these inputs"""

    def __init__(self, path=RECORD):
        with open(path) as f:
            self.calls = json.load(f)["calls"]

    def _replay(self, op, args):
        key = call_key(op, args)
        if key not in self.calls:
            raise AssertionError(f"{op}: no recorded reference result for these inputs ({key}); "
                                 "tests/golden/make_reference_calls.py records them")
        return self.calls[key]

    def generate(self, *args):
        return self._replay("generate", args)

    def evaluate(self, *args):
        return self._replay("evaluate", args)

    def sr_fitness(self, *args):
        return self._replay("sr_fitness", args)

    def crossover(self, *args):
        return self._replay("crossover", args)

    def mutate(self, *args):
        return self._replay("mutate", args)


class RecordingReference(RecordedReference):
    """The live library (Oracle("reference")): returns the same digests and keeps every call for the record"""

    def __init__(self, live):
        self.live = live
        self.calls = {}

    def _replay(self, op, args):
        d = result_digest(op, getattr(self.live, op)(*args))
        self.calls[call_key(op, args)] = d
        return d
