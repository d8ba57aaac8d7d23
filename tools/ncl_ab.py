#!/usr/bin/env python3
"""Interleaved same-process A/B of NCL's structure contrast on the MI355X, timed with HIP events.

One side of ssl_layer_loss (model/NCL.py:68-94) forward + backward: the library's crh_table_nce_f32 (one call: the loss, the
batch rows' gradient and the dense table gradient) against the reference's torch formula under autograd (normalize the
whole table, B x N matmul, exp, sum, log, and autograd back through all of it) on the same inputs, at shapes where torch
still fits.  A and B alternate in rounds; each round times `--reps` back-to-back calls between two events and the median
round is reported, with the torch arm's peak memory above the inputs.  FLOP model: 8 B N d per call (S and P.T in the row
pass, S again and P^T.X in the column pass), against the 157.3 TF fp32 MFMA peak.

    python tools/ncl_ab.py [--rounds 7] [--reps 10] [--shape 2048x262144x64 512x300x64] [--out profiles/ncl_ab.json]

``--step``: one whole warm-up TRAINING STEP of the built-in engine (train.NCLEngine) against the same step written with this
package's hooks under autograd -- HipSparseAdj through torch.sparse.mm, bpr_loss and l2_reg_loss of coldrec_amd.util.utils,
the torch formula above for both sides, torch.optim.Adam.  Sizes: the CiteULike shape (5 551 x 16 980, d = 128, L = 3,
B = 4 096) and the toy shape (d = 64, L = 3, B = 512).  Steps are launched eagerly on both sides.

    python tools/ncl_ab.py --step [--rounds 7] [--reps 20] [--out profiles/ncl_ab_step.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from coldrec_amd import ops  # noqa: E402
from tools.cl_ab import _step_setup  # noqa: E402

PEAK_TF = 157.3


def torch_formula(ctx, table, idx, tau):
    x1, x2, t = F.normalize(ctx[idx]), F.normalize(table[idx]), F.normalize(table)
    pos = torch.exp((x1 * x2).sum(1) / tau)
    ttl = torch.exp(x1 @ t.T / tau).sum(1)
    return -torch.log(pos / ttl).sum()


def _rounds(sides, rounds, reps):
    """Median and spread of `reps` back-to-back calls per round, the sides alternating (microseconds per call)."""
    times = {k: [] for k in sides}
    for _ in range(rounds):
        for name, f in sides.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / reps)
    return times


def _autograd_step(su, L, h, tau, ssl_reg, alpha, reg, lr, dev):
    import scipy.sparse as sp
    from coldrec_amd.graph import HipSparseAdj
    from coldrec_amd.util.utils import bpr_loss, l2_reg_loss
    n = su["U"] + su["I"]
    adj = HipSparseAdj.from_scipy(sp.csr_matrix((su["val"], su["col"], su["rowptr"]), shape=(n, n))).to(dev)
    E = torch.nn.Parameter(torch.cat([su["U0"], su["V0"]], 0).to(dev))
    opt = torch.optim.Adam([E], lr=lr)
    U, u, i, j = su["U"], su["u"].long(), su["i"].long(), su["j"].long()

    def step():
        embs = [E]
        for _ in range(L):
            embs.append(torch.sparse.mm(adj, embs[-1]))
        rec, ctx = torch.stack(embs, 1).mean(1), embs[2 * h]
        ue, pe, ne = rec[u], rec[i + U], rec[j + U]
        loss = bpr_loss(ue, pe, ne) + l2_reg_loss(reg, ue, pe, ne) + ssl_reg * (
            torch_formula(ctx[:U], E[:U], u, tau) + alpha * torch_formula(ctx[U:], E[U:], i, tau))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def _engine_step(su, L, h, tau, ssl_reg, alpha, reg, lr, dev):
    from coldrec_amd.train import NCLEngine
    eng = NCLEngine(su["U0"], su["V0"], su["rowptr"], su["col"], su["val"], L, lr, reg, dev, tau=tau, ssl_reg=ssl_reg,
                    alpha=alpha, hyper_layers=h, batch_size=int(su["u"].shape[0]))
    plan = ops.build_plans_device(su["u"], su["i"], su["j"], su["u"].shape[0])[0]
    return lambda: eng.step(su["u"], su["i"], su["j"], plan)


def step_main(args):
    dev = torch.device("cuda:0")
    hyper = dict(tau=0.2, ssl_reg=1e-6, alpha=1.0, reg=1e-4, lr=1e-3)
    sizes = {"citeulike": (128, 3, 4096), "toy": (64, 3, 512)}
    rows = []
    for shape in ([args.step_shape] if args.step_shape else ["citeulike", "toy"]):
        d, L, B = sizes[shape]
        su = _step_setup(shape, d, B, dev)
        sides = {"engine": _engine_step(su, L, 1, dev=dev, **hyper), "autograd": _autograd_step(su, L, 1, dev=dev, **hyper)}
        for f in sides.values():
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        times = _rounds(sides, args.rounds, args.reps)
        row = {"shape": shape, "d": d, "layers": L, "hyper_layers": 1, "batch": int(su["u"].shape[0]),
               "users": su["U"], "items": su["I"], "edges": int(su["rowptr"][-1])}
        for name, t in times.items():
            row[name + "_step_us"] = round(statistics.median(t), 1)
            row[name + "_step_us_spread"] = [round(min(t), 1), round(max(t), 1)]
        row["speedup"] = round(row["autograd_step_us"] / row["engine_step_us"], 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
    return {"tool": "tools/ncl_ab.py --step", "hyper": hyper, "steps": rows}


def kernel_main(args):
    dev = torch.device("cuda:0")
    rows = []
    for shape in args.shape:
        b, n, d = (int(x) for x in shape.lower().split("x"))
        g = torch.Generator(device=dev).manual_seed(b + n + d)
        table = torch.randn(n, d, device=dev, generator=g) * 0.3
        ctx = table * 0.5 + torch.randn(n, d, device=dev, generator=g) * 0.2
        idx = torch.randint(0, n, (b,), device=dev, generator=g, dtype=torch.int32)
        il = idx.long()
        g_ctx, g_table, loss = torch.zeros_like(ctx), torch.empty_like(table), torch.empty(1, device=dev)
        ws = ops.table_nce_workspace(b, n, d, dev)
        a1, a2 = ctx.clone().requires_grad_(), table.clone().requires_grad_()

        def lib_call():
            ops.table_nce(ctx, table, idx, args.tau, grad_ctx=g_ctx, grad_table=g_table, loss=loss, workspace=ws)

        def torch_call():
            a1.grad = a2.grad = None
            torch_formula(a1, a2, il, args.tau).backward()

        for f in (lib_call, torch_call):           # warm-up: code objects, the BLAS library's algorithm choice
            for _ in range(3):
                f()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        torch_call()
        torch.cuda.synchronize()
        torch_peak = torch.cuda.max_memory_allocated(dev) - base
        times = _rounds({"lib": lib_call, "torch": torch_call}, args.rounds, args.reps)
        torch_loss = torch_formula(ctx, table, il, args.tau).item()    # the two sides compute the same loss (fp32 vs fp32)
        lib_call()
        torch.cuda.synchronize()
        lib_us, torch_us = statistics.median(times["lib"]), statistics.median(times["torch"])
        flop = 8.0 * b * n * d
        rows.append({"batch": b, "rows": n, "d": d, "lib_us": round(lib_us, 1), "torch_us": round(torch_us, 1),
                     "speedup": round(torch_us / lib_us, 2), "lib_tflops": round(flop / lib_us / 1e6, 1),
                     "lib_frac_of_fp32_peak": round(flop / lib_us / 1e6 / PEAK_TF, 3),
                     "lib_us_spread": [round(min(times["lib"]), 1), round(max(times["lib"]), 1)],
                     "torch_us_spread": [round(min(times["torch"]), 1), round(max(times["torch"]), 1)],
                     "lib_workspace_mib": round(ws.numel() / 2 ** 20, 1), "torch_peak_mib": round(torch_peak / 2 ** 20, 1),
                     "loss_rel_diff": abs(loss.item() - torch_loss) / abs(torch_loss)})
        print(json.dumps(rows[-1]), flush=True)
        del ws
    return {"tool": "tools/ncl_ab.py", "tau": args.tau, "table_nce": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="time one training step of the built-in engine (see the docstring)")
    ap.add_argument("--step-shape", choices=["citeulike", "toy"], default=None, help="--step: one shape only")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shape", nargs="*", default=["2048x262144x64", "512x300x64"], help="BxNxd of the kernel A/B")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ncl_ab.py measures on the GPU; no GPU is visible")
    rec = step_main(args) if args.step else kernel_main(args)
    rec.update(rounds=args.rounds, reps=args.reps, device=torch.cuda.get_device_name(0))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
