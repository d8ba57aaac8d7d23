"""The output bits of the five fused losses that take a plan's inverse index (ops.ccfcrec, ops.gar, ops.mtpr, ops.vbpr,
ops.duif) at the kernel tests' cases: every CASES entry, both cold modes, VBPR with and without h_adv.  Prints one JSON object, a
sha256 per output tensor.  Two libraries with the same ABI compute the same bits exactly when two runs print the same:

    python tools/loss_bits.py > a.json;  CRH_LIB=/path/to/other/libcoldrec_hip.so python tools/loss_bits.py > b.json
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402
from tests import duif_restate, mtpr_restate, test_ccfcrec_gpu, test_gar_gpu, vbpr_restate  # noqa: E402  (the cases and their inputs)

DEV = torch.device("cuda:0")


def digest(t) -> str:
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def record(out: dict, tag: str, names, tensors) -> None:
    torch.cuda.synchronize()
    for n, t in zip(names, tensors):
        if t is not None:
            out[f"{tag}/{n}"] = digest(t)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("loss_bits: needs the GPU; there is no CPU path")
    dev, out = DEV, {}
    for case in test_ccfcrec_gpu.CASES:
        inp = test_ccfcrec_gpu._inputs(case)
        nu, ni, tau, lam = case[5:]
        plan = ops.ccfcrec_plan(*(t.to(dev) for t in inp[3:]), nu, ni)
        got = ops.ccfcrec(*(t.to(dev) for t in inp[:3]), plan, tau, lam)
        record(out, "ccfcrec/" + test_ccfcrec_gpu.IDS(case), ("loss", "grad_user", "grad_item", "grad_q"), got)
    for case in test_gar_gpu.CASES:
        U, V, users, pos, neg, G = (t.to(dev) for t in test_gar_gpu._inputs(case))
        plan = ops.gar_plan(users, pos, neg)
        for cold_user in (False, True):
            got = ops.gar(U, V, G, plan, *test_gar_gpu.COEF, cold_user=cold_user)
            record(out, f"gar/{test_gar_gpu.IDS(case)}/{'user' if cold_user else 'item'}",
                   ("loss", "grad_user", "grad_item", "grad_gen"), got)
    for case in mtpr_restate.CASES:
        for cold_user in (False, True):
            P, Q, h, weu, wei, users, pos, neg = (t.to(dev) for t in mtpr_restate.inputs(case, cold_user,
                                                                                          ops.mtpr_chunk_rows()))
            got = ops.mtpr(P, Q, h, weu, wei, ops.mtpr_plan(users, pos, neg), mtpr_restate.WD1, cold_user=cold_user)
            record(out, f"mtpr/{mtpr_restate.CASE_IDS(case)}/{'user' if cold_user else 'item'}",
                   ("loss", "grad_user", "grad_item", "grad_h", "grad_weu", "grad_wei"), got)
    for case in vbpr_restate.CASES:
        for variant in vbpr_restate.VARIANTS:
            cold_user, adv = variant
            inp = vbpr_restate.inputs(case, cold_user, adv, ops.vbpr_chunk_rows())
            P, Q, A, h, h_adv, users, pos, neg = (None if t is None else t.to(dev) for t in inp)
            got = ops.vbpr(P, Q, A, h, ops.vbpr_plan(users, pos, neg), vbpr_restate.WD1, h_adv=h_adv,
                           lmd=vbpr_restate.CASE_LMD, cold_user=cold_user, want_hsum=True)
            record(out, f"vbpr/{vbpr_restate.CASE_IDS(case)}/{vbpr_restate.VARIANT_IDS(variant)}",
                   ("loss", "grad_user", "grad_item", "grad_aux", "grad_h", "grad_h_adv", "grad_hsum"), got)
    for case in duif_restate.CASES:
        for cold_user in duif_restate.MODES:
            T, C, W, users, pos, neg = (t.to(dev) for t in duif_restate.inputs(case, cold_user, ops.duif_chunk_rows()))
            got = ops.duif(T, C, W, ops.duif_plan(users, pos, neg, cold_user), duif_restate.CASE_REG, cold_user=cold_user, want_h=True)
            record(out, f"duif/{duif_restate.CASE_IDS(case)}/{duif_restate.MODE_IDS(cold_user)}",
                   ("loss", "grad_table", "grad_w", "h"), got)
    print(json.dumps(out, indent=0, sort_keys=True))


if __name__ == "__main__":
    main()
