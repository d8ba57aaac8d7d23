"""A/B on one device: one fused CCFCRec loss call (forward + backward, csrc/ccfcrec.hip through ops.ccfcrec, the index
plan included and excluded) against the torch formula of the reference (model/CCFCRec.py:53-87) under autograd.

    python tools/ccfcrec_ab.py [--batch 4096] [--pos 5] [--neg 40] [--self_neg 40] [--d 64] [--users 6040] [--items 3706]
                               [--rounds 20]

The arms are interleaved round by round and timed with device events after a warm-up of every shape; prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402


def torch_formula(U, V, Q, users, items, neg_users, pos, neg, sneg, tau, lam):
    """The reference's op sequence: gathered (B, P, d), (B, P, N, d) and (B, S, d) rows, norms, products, exponentials,
    -log(pos / (pos + sum neg)), then the two logsigmoid rank terms."""

    def score(q, v):
        return torch.exp((q * v).sum(-1) / (tau * q.norm(dim=-1) * v.norm(dim=-1)))

    q1 = Q.unsqueeze(1)
    e_pos, e_neg = score(q1, V[pos]), score(q1.unsqueeze(1), V[neg]).sum(2)
    contrast = (-torch.log(e_pos / (e_pos + e_neg))).sum() / pos.shape[1]
    e_self, e_sneg = score(Q, V[items]), score(q1, V[sneg]).sum(1)
    self_contrast = (-torch.log(e_self / (e_self + e_sneg))).sum()
    uu, uk, vi = U[users], U[neg_users], V[items]
    ls = torch.nn.functional.logsigmoid
    rank = -ls((vi * uu).sum(1) - (vi * uk).sum(1)).sum() - ls((Q * uu).sum(1) - (Q * uk).sum(1)).sum()
    return lam * (contrast + self_contrast) + (1 - lam) * rank


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--pos", type=int, default=5)
    ap.add_argument("--neg", type=int, default=40)
    ap.add_argument("--self_neg", type=int, default=40)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ccfcrec_ab: needs the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    B, P, N, S = a.batch, a.pos, a.neg, a.self_neg
    U = (torch.randn(a.users, a.d, generator=g) * 0.1).to(dev).requires_grad_()
    V = (torch.randn(a.items, a.d, generator=g) * 0.1).to(dev).requires_grad_()
    Q = (torch.randn(B, a.d, generator=g) * 0.1).to(dev).requires_grad_()
    ru = lambda *shape: torch.randint(a.users, shape, generator=g).to(dev)
    ri = lambda *shape: torch.randint(a.items, shape, generator=g).to(dev)
    ids = (ru(B), ri(B), ru(B), ri(B, P), ri(B, P, N), ri(B, S))
    plan = ops.ccfcrec_plan(*ids, a.users, a.items)
    ws = ops.ccfcrec_workspace(B, P, N, S, a.d, plan["n_items"], plan["n_users"], dev)
    bufs = [torch.zeros_like(U), torch.zeros_like(V), torch.empty_like(Q)]
    loss = torch.empty(5, device=dev)

    def fused(p=plan):
        bufs[0].zero_()
        bufs[1].zero_()
        ops.ccfcrec(U.detach(), V.detach(), Q.detach(), p, 0.1, 0.6, grad_user=bufs[0], grad_item=bufs[1], grad_q=bufs[2],
                    loss=loss, workspace=ws)

    def fused_with_plan():
        fused(ops.ccfcrec_plan(*ids))

    def formula():
        return torch.autograd.grad(torch_formula(U, V, Q, *ids, 0.1, 0.6), (U, V, Q))

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
    print(json.dumps(dict(shape=vars(a), rows=ops.ccfcrec_rows(P, N, S), n_items=plan["n_items"],
                          n_item_chunks=plan["n_item_chunks"], n_users=plan["n_users"],
                          n_user_chunks=plan["n_user_chunks"], ms_median=med,
                          ms_min={k: min(v) for k, v in times.items()},
                          ratio_formula_over_fused=med["torch_formula"] / med["fused"],
                          ratio_formula_over_fused_with_plan=med["torch_formula"] / med["fused_with_plan"],
                          grad_err_over_max=err)))


if __name__ == "__main__":
    main()
