"""A/B on one device: one whole training step of MetaEmbedding and of DeepMusic (cold items) -- the generator on the batch's
content rows, the loss, backward, Adam over the generator -- with the trainers' fused operators (csrc/metaemb.hip through
ops.metaemb, csrc/deepmusic.hip through ops.deepmusic), against the same step written the reference's way in float32
torch autograd on the same device (tests/metaemb_restate.py and tests/deepmusic_restate.py's ``loss_terms``: the gathers,
both forward passes, ``autograd.grad`` in the middle, ``binary_cross_entropy_with_logits``; ``F.mse_loss`` and
``torch.norm``).  There is no earlier trainer of either model in this package to compare with.

    python tools/metaemb_step_ab.py [--batch 2048] [--d 64] [--content 16] [--reps 60]

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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from coldrec_amd.model.DeepMusic import DeepMusic_Encoder  # noqa: E402
from coldrec_amd.model.MetaEmbedding import MetaEmbedding_Learner  # noqa: E402
from tests import deepmusic_restate as DR  # noqa: E402  (the torch formulas)
from tests import metaemb_restate as MR  # noqa: E402

DEV = torch.device("cuda:0")
LR, ALPHA, REG = 1e-3, 0.5, 1e-4


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
    """(fused step, torch step) on equal tables and equal generators."""
    D, C = a.d, a.content
    content = torch.randn(ni, C, generator=g)
    U, V = (torch.randn(n, D, generator=g) * 0.1 for n in (nu, ni))
    data = types.SimpleNamespace(user_num=nu, item_num=ni, mapped_item_content=content.numpy(), item_content_dim=C)
    args = argparse.Namespace(dataset="ab", cold_object="item", backbone="MF", alpha=ALPHA)
    os.makedirs("emb", exist_ok=True)
    torch.save(U, "./emb/ab_cold_item_MF_user_emb.pt")
    torch.save(V, "./emb/ab_cold_item_MF_item_emb.pt")
    meta = which == "MetaEmbedding"
    if meta:
        model = MetaEmbedding_Learner(args, data, D, DEV, LR / 10.).to(DEV)
        theirs = MR.generator(C, D)
        theirs.load_state_dict(model.emb_pred_Dense.state_dict())
    else:
        model = DeepMusic_Encoder(args, data, D, DEV, REG).to(DEV)
        theirs = DR.generator(C, D)
        theirs.load_state_dict(model.transformation.state_dict())
    theirs = theirs.to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    opt_t = torch.optim.Adam(theirs.parameters(), lr=LR)
    c, tu, tv = content.to(DEV), U.to(DEV), V.to(DEV)

    def fused(b):
        loss = model.loss(*b)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def plain(b):
        u, p, n = (t.long() for t in b[:3])
        if meta:
            uu, ii = torch.cat([u, u]), torch.cat([p, n])
            loss = MR.loss_terms(tu[uu], theirs(c[ii]) / 5., u.shape[0], ALPHA, LR / 10.)[2]
        else:
            loss = DR.loss_terms(tv[p], theirs(c[p]), REG)[2]
        opt_t.zero_grad()
        loss.backward()
        opt_t.step()

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
        for which in ("MetaEmbedding", "DeepMusic"):
            fused, plain = arms(which, a, nu, ni, g)
            f, t = median_ms(fused, batches, a.warm, a.reps), median_ms(plain, batches, a.warm, a.reps)
            print(f"{which} {label} ({nu} x {ni}, B = {a.batch}, d = {a.d}, content {a.content}): fused {f[0]:.3f} ms (p10 {f[1]:.3f}, "
                  f"p90 {f[2]:.3f}), torch {t[0]:.3f} ms (p10 {t[1]:.3f}, p90 {t[2]:.3f}), ratio {t[0] / f[0]:.2f}", flush=True)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as tmp:      # (the learners load the backbone's files from ./emb)
        os.chdir(tmp)
        try:
            main()
        finally:
            os.chdir(ROOT)
