"""Generate G18(i) under tests/golden/ by RUNNING THE REFERENCE's InfoNCE (util/utils.py:61-76).

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py and importing the
reference the same way:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g18.py

g18_infonce.npz  per case: the fp32 inputs (seeded), then the reference's loss and both input gradients (autograd), computed
                 in float64 on those inputs.  Cases cover several N and d, tau in {0.05, 0.2, 1}, both b_cos, a zero row (the
                 normalize clamp) and duplicated rows.  Regenerates byte for byte.
"""
import os
import sys
import types

os.environ.setdefault("OMP_NUM_THREADS", "1")
os.environ.setdefault("MKL_NUM_THREADS", "1")

import numpy as np
import torch

torch.set_num_threads(1)

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, REF)
_m = types.ModuleType("model")
_m.__path__ = [os.path.join(REF, "model")]
sys.modules["model"] = _m

from util.utils import InfoNCE  # noqa: E402  (reference)

# name: (N, d, tau, b_cos, special)
CASES = {
    "n1": (1, 8, 0.2, True, ""),
    "zero": (7, 4, 0.05, True, "zero"),
    "dup50": (33, 50, 0.2, True, "dup"),
    "raw64": (64, 64, 1.0, False, ""),
    "zerodup": (130, 64, 0.05, True, "zero,dup"),
    "rawdup": (200, 16, 0.2, False, "dup"),
    "cos128": (97, 128, 1.0, True, ""),
    "rawzero": (40, 8, 0.05, False, "zero"),
}


def case_inputs(rng, n, d, special):
    v1 = (rng.standard_normal((n, d)) * 0.3).astype(np.float32)
    v2 = (v1 + rng.standard_normal((n, d)) * 0.2).astype(np.float32)     # correlated views, like two perturbations
    if "zero" in special:
        v1[n // 2] = 0.0
        v2[n - 1] = 0.0
    if "dup" in special:
        v1[1] = v1[0]
        v2[n - 2] = v2[n - 3]
        v1[n - 1] = v1[2]
        v2[n - 1] = v2[2]
    return v1, v2


def main():
    rng = np.random.RandomState(18)
    res = {"cases": np.array(sorted(CASES))}
    for name in sorted(CASES):
        n, d, tau, b_cos, special = CASES[name]
        v1, v2 = case_inputs(rng, n, d, special)
        a = torch.from_numpy(v1).double().requires_grad_()
        b = torch.from_numpy(v2).double().requires_grad_()
        loss = InfoNCE(a, b, tau, b_cos)
        loss.backward()
        res.update({f"{name}_v1": v1, f"{name}_v2": v2, f"{name}_tau": np.float64(tau), f"{name}_bcos": np.int64(b_cos),
                    f"{name}_loss": np.float64(loss.item()), f"{name}_g1": a.grad.numpy(), f"{name}_g2": b.grad.numpy()})
    np.savez_compressed(os.path.join(HERE, "g18_infonce.npz"), **res)


if __name__ == "__main__":
    main()
