"""A/B on one device: one fused CLCRec loss call (forward + backward, csrc/clcrec.hip through ops.clcrec, the index plan
included and excluded) against the torch formula of the reference (model/CLCRec.py:125-148) under autograd.

    python tools/clcrec_ab.py [--batch 4096] [--num_neg 128] [--d 64] [--users 6040] [--items 3706] [--rounds 20]

The arms are interleaved round by round and timed with device events after a warm-up of every shape; prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402


def torch_formula(U, V, feat_rows, users, items, rand_index, temp, lam, reg):
    B, G1 = items.shape
    flat = items.reshape(-1)
    u = U[users].repeat_interleave(G1, 0)
    pos = V[items[:, 0]].repeat_interleave(G1, 0)
    allv = V[flat]
    x = allv.clone()
    x[rand_index] = feat_rows[rand_index].clone()
    nf, ne = torch.nn.functional.normalize(feat_rows, dim=1), torch.nn.functional.normalize(pos, dim=1)

    def cl(a, b):
        s = torch.exp((a * b).sum(1) / temp).view(B, G1)
        return (-torch.log(s[:, 0] / s.sum(1))).mean()

    r = (torch.sqrt((u ** 2).sum(1)).mean() + torch.sqrt((allv ** 2).sum(1)).mean()) / 2
    return cl(ne, nf) * lam + cl(u, x) * (1 - lam) + reg * r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--num_neg", type=int, default=128)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clcrec_ab: needs the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    U = (torch.randn(a.users, a.d, generator=g) * 0.1).to(dev).requires_grad_()
    V = (torch.randn(a.items, a.d, generator=g) * 0.1).to(dev).requires_grad_()
    users = torch.randint(a.users, (a.batch,), generator=g).to(dev)
    items = torch.randint(a.items, (a.batch, 1 + a.num_neg), generator=g).to(dev)
    M = items.numel()
    rand_index = torch.randint(M, (M // 2,), generator=g)
    counts = torch.bincount(rand_index, minlength=M).to(torch.int32).to(dev)
    rand_index = rand_index.to(dev)
    plan = ops.clcrec_plan(users, items, a.users, a.items)
    E = (torch.randn(plan["n_slots"], a.d, generator=g) * 0.1).to(dev).requires_grad_()
    ws = ops.clcrec_workspace(a.batch, a.num_neg, a.d, plan["n_slots"], dev)
    bufs = [torch.zeros_like(U), torch.zeros_like(V), torch.empty_like(E)]
    loss = torch.empty(4, device=dev)

    def fused(p=plan):
        bufs[0].zero_()
        bufs[1].zero_()
        ops.clcrec(U.detach(), V.detach(), E.detach(), p, counts, 2.0, 0.5, 1e-4, grad_user=bufs[0], grad_item=bufs[1],
                   grad_feat=bufs[2], loss=loss, workspace=ws)

    def fused_with_plan():
        fused(ops.clcrec_plan(users, items))

    def formula():
        total = torch_formula(U, V, E[plan["slot"].long()], users, items, rand_index, 2.0, 0.5, 1e-4)
        return torch.autograd.grad(total, (U, V, E))

    arms = dict(fused=fused, fused_with_plan=fused_with_plan, torch_formula=formula)
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, f in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            f()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1))
    med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
    ref = formula()
    fused()
    err = [float((b - r).abs().max() / r.abs().max()) for b, r in zip(bufs, ref)]
    print(json.dumps(dict(shape=vars(a), n_slots=plan["n_slots"], n_chunks=plan["n_chunks"],
                          ms_median=med, ms_min={k: min(v) for k, v in times.items()},
                          ratio_formula_over_fused=med["torch_formula"] / med["fused"],
                          ratio_formula_over_fused_with_plan=med["torch_formula"] / med["fused_with_plan"],
                          grad_err_over_max=err)))


if __name__ == "__main__":
    main()
