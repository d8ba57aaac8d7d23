"""Three arms on one device: one whole DUIF training step in float32, Adam included, for cold items and cold users --
    (a) this trainer's step: ``DUIF_Encoder.loss`` (the plan, csrc/duif.hip through ops.duif), backward, torch.optim.Adam;
    (b) the reference's formulation (model/DUIF.py:19-27): project the WHOLE content table, gather, autograd, Adam;
    (c) the torch formulation that gathers the batch's content rows first and projects only those (tests/duif_restate.py).

    python tools/duif_step_ab.py [--batch 2048] [--d 64] [--warm 10] [--reps 60]

Four shapes: the toy one (300 x 500, content width 16), a MovieLens-sized one (6040 x 3706, 206), a CiteULike-sized one
(5551 x 16980, 300) and one catalogue of 10^6 content rows at width 128 (the free side 6040 rows).  After a warm-up of
every arm the arms run interleaved, one step of each in turn, every step timed on its own between two synchronisations;
prints the median and the 10th / 90th percentiles of each arm.  Run it twice.
"""
import argparse
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from coldrec_amd.model.DUIF import DUIF_Encoder  # noqa: E402
from tests import duif_restate as R  # noqa: E402  (the torch formula)

DEV = torch.device("cuda:0")
LR, REG = 1e-3, 1e-4
SHAPES = (("toy", 300, 500, 16), ("movielens-sized", 6040, 3706, 206), ("citeulike-sized", 5551, 16980, 300),
          ("10^6 content rows", None, None, 128))


def interleaved_ms(steps, batches, warm, reps):
    """Per arm (median, p10, p90) ms of individually timed steps, the arms taking turns."""
    for step in steps:
        for k in range(warm):
            step(batches[k % len(batches)])
    torch.cuda.synchronize()
    ts = [[] for _ in steps]
    for k in range(reps):
        b = batches[k % len(batches)]
        for arm, step in enumerate(steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step(b)
            torch.cuda.synchronize()
            ts[arm].append((time.perf_counter() - t0) * 1e3)
    return [(float(np.median(t)), float(np.percentile(t, 10)), float(np.percentile(t, 90))) for t in ts]


def arms(a, nu, ni, cdim, cold_user, g):
    """(fused step, whole-table torch step, gather-first torch step) on equal tensors."""
    d = a.d
    n_content = nu if cold_user else ni
    content = torch.randn(n_content, cdim, generator=g)
    data = types.SimpleNamespace(user_num=nu, item_num=ni, user_content_dim=cdim, item_content_dim=cdim,
                                 mapped_user_content=content.numpy(), mapped_item_content=content.numpy())
    args = argparse.Namespace(cold_object="user" if cold_user else "item", reg=REG)
    model = DUIF_Encoder(args, data, d, DEV).to(DEV)
    opt = torch.optim.Adam(model.parameters(), lr=LR)

    def fused(b):
        loss = model.loss(*b)
        opt.zero_grad()
        loss.backward()
        opt.step()

    c = model.content
    out = [fused]
    for whole in (True, False):
        T = torch.nn.Parameter(model.table.detach().clone())
        W = torch.nn.Parameter(model.projector.weight.detach().clone())
        o = torch.optim.Adam([T, W], lr=LR)

        def plain(b, T=T, W=W, o=o, whole=whole):
            u, p, n = (t.long() for t in b[:3])
            if whole:                                   # model(): the whole table projected, then gathered
                H = c @ W.T
                U, P, N = (H[u], T[p], T[n]) if cold_user else (T[u], H[p], H[n])
                loss = R.bpr((U * P).sum(1) - (U * N).sum(1)).mean() + REG * sum(torch.norm(t, p=2) / t.shape[0] for t in (U, P, N))
            else:
                loss = R.loss_terms(T, c, W, u, p, n, REG, cold_user)[2]
            o.zero_grad()
            loss.backward()
            o.step()

        out.append(plain)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--reps", type=int, default=60)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("duif_step_ab: needs the GPU; there is no CPU path")
    for label, nu, ni, cdim in SHAPES:
        for cold_user in (False, True):
            if nu is None:
                su, si = (1_000_000, 3706) if cold_user else (6040, 1_000_000)
            else:
                su, si = nu, ni
            g = torch.Generator().manual_seed(1)
            batches = []
            for _ in range(16):
                u, p, n = (torch.randint(k, (a.batch,), generator=g).to(DEV) for k in (su, si, si))
                batches.append((u, p, n, ((0, su - 1), (0, si - 1))))
            f, w, s = interleaved_ms(arms(a, su, si, cdim, cold_user, g), batches, a.warm, a.reps)
            print(f"{label} ({su} x {si}, c = {cdim}, {'user' if cold_user else 'item'} mode, B = {a.batch}, d = {a.d}): "
                  f"(a) fused {f[0]:.3f} ms (p10 {f[1]:.3f}, p90 {f[2]:.3f}); (b) whole table {w[0]:.3f} ms (p10 {w[1]:.3f}, p90 "
                  f"{w[2]:.3f}); (c) gather first {s[0]:.3f} ms (p10 {s[1]:.3f}, p90 {s[2]:.3f}); b / a {w[0] / f[0]:.2f}, "
                  f"c / a {s[0] / f[0]:.2f}", flush=True)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
