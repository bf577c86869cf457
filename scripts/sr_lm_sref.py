"""The CPU side of the head-to-head test of tests/test_gpu_sr_lm.py: on its 4 096-tree + - * / forest and 256 rows, run 5 steps of
the descent and 5 steps of Levenberg-Marquardt with the float64 references registered as CPU kernels (tests/cpu_grad_ops.py,
tests/cpu_lm_ops.py) and print the share s_ref of finite trees whose LM loss is <= their descent loss, and the two median losses.
Needs no GPU (about a minute); the numbers are quoted in DESIGN.md section 3.11 and beside the test's assertion."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import cpu_grad_ops
    import cpu_lm_ops
    import cpu_ops
    from helpers import c2_dataset

    cpu_ops.register()
    cpu_grad_ops.register()
    cpu_lm_ops.register()
    from evogp_amd.tree import Forest, GenerateDescriptor, set_default_device

    set_default_device("cpu")
    desc = GenerateDescriptor(max_tree_len=64, input_len=10, output_len=1, using_funcs=["+", "-", "*", "/"], max_layer_cnt=6,
                              const_samples=[-1, 0, 1])
    f0 = Forest.random_generate(4096, desc, keys=torch.tensor([42, 0]))
    X, y = (torch.from_numpy(a) for a in c2_dataset(D=256))
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    with np.errstate(all="ignore"):
        before = f0.optimize_constants(X, y, steps=0)[1].numpy()
        descent = f0.optimize_constants(X, y, steps=steps)[1].numpy()
        lm = f0.optimize_constants(X, y, steps=steps, method="lm")[1].numpy()
    fin = np.isfinite(descent) & np.isfinite(lm)
    print(json.dumps({"pop": 4096, "rows": 256, "steps": steps, "finite": int(fin.sum()),
                      "s_ref": float((lm[fin] <= descent[fin]).mean()), "lm_strictly_better": float((lm[fin] < descent[fin]).mean()),
                      "descent_strictly_better": float((descent[fin] < lm[fin]).mean()),
                      "median_before": float(np.median(before[fin])), "median_descent": float(np.median(descent[fin])),
                      "median_lm": float(np.median(lm[fin]))}))


if __name__ == "__main__":
    main()
