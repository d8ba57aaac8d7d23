"""A/B on one device: one whole training step of VBPR and of AMR (cold items) -- content[ids] @ W, the loss, R_w, backward,
Adagrad over P, Q, PQ2, Adam over W, AMR's two noise additions -- with the trainers' fused operator (csrc/vbpr.hip
through ops.vbpr) and ``ops.adagrad_rows``, against the same step written as the torch formula of the reference
(model/VBPR.py, model/AMR.py in the running-sum form of the noise, as tests/vbpr_restate.py states them) under autograd
with ``torch.optim.Adagrad``, in float32 on the same tables.

    python tools/vbpr_step_ab.py [--batch 2048] [--d 64] [--content 16] [--reps 60]

Two table shapes: the toy one (300 x 500) and a MovieLens-sized one (6040 x 3706, the shape of fixture g12).  After a
warm-up every step is timed on its own between two synchronisations; prints the median and the 10th / 90th percentiles
of each arm and the ratio of the medians.
"""
import argparse
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from coldrec_amd.model.AMR import AMR_Learner  # noqa: E402
from coldrec_amd.model.VBPR import VBPR_Learner  # noqa: E402
from tests import vbpr_restate as R  # noqa: E402  (the torch formula)

DEV = torch.device("cuda:0")
LR, WD1, WD2, EPS, LMD = 0.05, 0.01, 0.01, 0.1, 1.0


def median_ms(step, batches, warm, reps):
    for k in range(warm):
        step(batches[k % len(batches)])
    torch.cuda.synchronize()
    ts = []
    for k in range(reps):
        b = batches[k % len(batches)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step(b)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), float(np.percentile(ts, 10)), float(np.percentile(ts, 90))


def arms(which, a, nu, ni, g):
    """(fused step, torch step) on equal tables."""
    B, D, C = a.batch, a.d, a.content
    amr = which == "AMR"
    content = torch.randn(ni, C, generator=g)
    P, Q, A = (torch.randn(n, D, generator=g) * 0.1 for n in (nu, ni, nu))
    W = torch.randn(C, D, generator=g) * 0.1
    data = types.SimpleNamespace(user_num=nu, item_num=ni, mapped_item_content=content.numpy(), item_content_dim=C)
    args = argparse.Namespace(dataset="ab", cold_object="item", p_emb=[LR, WD1], p_ctx=[LR, WD2], eps=EPS, lmd=LMD)
    if amr:
        os.makedirs("emb", exist_ok=True)
        for t, f in zip((P, Q, A, content @ W, W), R.FILES):
            torch.save(t, f"./emb/ab_cold_item_VBPR_{f}.pt")
        model = AMR_Learner(args, data, D, DEV).to(DEV)
    else:
        model = VBPR_Learner(args, data, D, DEV, tensors=(P, Q, A, W)).to(DEV)
    opt = torch.optim.Adam([model.W], lr=LR)

    def fused(b):
        loss = model.loss(*b) + model.weight_regs()
        opt.zero_grad()
        loss.backward()
        model.step_tables()
        opt.step()

    tp, tq, ta, tw = (torch.nn.Parameter(t.clone().to(DEV)) for t in (P, Q, A, W))
    c = content.to(DEV)
    noise = torch.zeros_like(c)
    opts = [torch.optim.Adagrad([tp, ta, tq], lr=LR), torch.optim.Adam([tw], lr=LR)]

    def plain(b):
        u, p, n = (t.long() for t in b[:3])
        ids = torch.cat([p, n])
        h = c[ids] @ tw
        h_adv = None
        if amr:
            first = R.loss_terms(tp, tq, ta, h, u, p, n, WD1, False)[0]
            dh, = torch.autograd.grad(first, h, retain_graph=True)
            noise.index_add_(0, ids, dh @ tw.detach().T)
            h_adv = (c[ids] + EPS * F.normalize(noise[ids])) @ tw
            h.retain_grad()
            h_adv.retain_grad()
        loss = R.loss_terms(tp, tq, ta, h, u, p, n, WD1, False, h_adv, LMD)[3] + WD2 * (tw ** 2).sum()
        for o in opts:
            o.zero_grad()
        loss.backward()
        if amr:
            noise.index_add_(0, ids, (h.grad + h_adv.grad) @ tw.detach().T)
        for o in opts:
            o.step()

    return fused, plain


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--content", type=int, default=16)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=60)
    a = ap.parse_args()
    for label, nu, ni in (("toy", 300, 500), ("movielens-sized", 6040, 3706)):
        g = torch.Generator().manual_seed(1)
        batches = []
        for _ in range(16):
            u, p, n = (torch.randint(k, (a.batch,), generator=g).to(DEV) for k in (nu, ni, ni))
            batches.append((u, p, n, ((0, nu - 1), (0, ni - 1))))
        for which in ("VBPR", "AMR"):
            fused, plain = arms(which, a, nu, ni, g)
            f, t = median_ms(fused, batches, a.warm, a.reps), median_ms(plain, batches, a.warm, a.reps)
            print(f"{which} {label} ({nu} x {ni}, B = {a.batch}, d = {a.d}, content {a.content}): fused {f[0]:.3f} ms (p10 {f[1]:.3f}, "
                  f"p90 {f[2]:.3f}), torch {t[0]:.3f} ms (p10 {t[1]:.3f}, p90 {t[2]:.3f}), ratio {t[0] / f[0]:.2f}", flush=True)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:      # (AMR's learner loads VBPR's files from ./emb)
        os.chdir(tmp)
        try:
            main()
        finally:
            os.chdir(ROOT)
