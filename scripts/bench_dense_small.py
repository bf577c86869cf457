"""Small launches of tree_SR_fitness with the dense and with the packed arithmetic compiler ("One function node per
lane"; profiles/r12_dense_small.jsonl): the sweep behind the dense kernel's default.

    python scripts/bench_dense_small.py [label]          from the root of the tree to measure (its evogp_amd is imported)

Forests: the first 100 k trees of the headline forest -- bench.sr_inputs(0, 100_000): exactly BASELINE configs[1]'s forest on one GPU --
and its first 125 k / 250 k / 500 k trees.  Per forest: 40 untimed calls, then 7 rounds of 20 calls between two events; one JSON line with
the rounds' ms per call, their minimum and median.  Where the engine has the switch (evogp_hip_debug_tc_dense) every forest runs with the
dense kernel forced on, off, on, off; an engine without it (the parent commit, label it "parent") runs once."""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from evogp_amd import _lib  # noqa: E402
from evogp_amd.tree import Forest  # noqa: E402

dev = torch.device("cuda", 0)
torch.cuda.set_device(0)
label = sys.argv[1] if len(sys.argv) > 1 else "tree"
try:
    switch = _lib.lib.evogp_hip_debug_tc_dense
except AttributeError:
    switch = None
big, Xd, yd, _, _ = bench.sr_inputs(0, 500_000, dev)


def head(n):
    return Forest(big.input_len, big.output_len, big.batch_node_value[:n].contiguous(), big.batch_node_type[:n].contiguous(),
                  big.batch_subtree_size[:n].contiguous(), func_mask=big.func_mask)


cases = [("configs1_100k", head(100_000)), ("head125k", head(125_000)), ("head250k", head(250_000)), ("head500k", big)]


def measure(f):
    for _ in range(40):
        f.SR_fitness(Xd, yd, True, "auto")
    torch.cuda.synchronize()
    out = []
    for _ in range(7):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(20):
            f.SR_fitness(Xd, yd, True, "auto")
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / 20)
    return out


try:
    for name, f in cases:
        nan = int(torch.isnan(f.SR_fitness(Xd, yd, True, "auto")).sum())
        for mode in ((1, 0, 1, 0) if switch else (None,)):
            if mode is not None:
                assert switch(mode) == 0
            ms = measure(f)
            print(json.dumps({"side": label, "case": name, "trees": f.pop_size, "nan_fitness": nan, "dense": mode, "ms_per_call_min": round(min(ms), 5),
                              "ms_per_call_median": round(float(np.median(ms)), 5), "ms_per_call": [round(x, 5) for x in ms]}), flush=True)
finally:
    if switch:
        switch(-1)
