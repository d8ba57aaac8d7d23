#!/usr/bin/env python3
"""Interleaved same-process A/B of the contrastive loss on the MI355X, timed with HIP events.

InfoNCE forward + backward (util/utils.py:61-76 with b_cos): the library's crh_infonce_f32 (one call: loss and both
gradients) against the reference's torch formula (normalize, N x N matmul, log_softmax, diag, mean, autograd back through
all of it) on the same inputs, at N in {1024, 2048, 4096, 16384} and d in {64, 128}.  A and B alternate in rounds; each
round times `--reps` back-to-back calls between two events and the median round is reported.  FLOP model: 8 N^2 d per
call (S and P.Z2 in the row pass, S again and P^T.Z1 in the column pass), against the 157.3 TF fp32 MFMA peak.

    python tools/cl_ab.py [--rounds 7] [--reps 20] [--n 4096] [--d 64] [--out profiles/cl_ab.json]
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

PEAK_TF = 157.3


def torch_formula(v1, v2, tau):
    a, b = F.normalize(v1, dim=1), F.normalize(v2, dim=1)
    return -torch.diag(F.log_softmax((a @ b.T) / tau, dim=1)).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, nargs="*", default=[1024, 2048, 4096, 16384])
    ap.add_argument("--d", type=int, nargs="*", default=[64, 128])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cl_ab.py measures on the GPU; no GPU is visible")
    dev = torch.device("cuda:0")
    rows = []
    for n in args.n:
        for d in args.d:
            g = torch.Generator(device=dev).manual_seed(n + d)
            v1 = torch.randn(n, d, device=dev, generator=g) * 0.3
            v2 = v1 + torch.randn(n, d, device=dev, generator=g) * 0.2
            g1, g2, loss = torch.empty_like(v1), torch.empty_like(v2), torch.empty(1, device=dev)
            ws = ops.infonce_workspace(n, d, dev)
            a1, a2 = v1.clone().requires_grad_(), v2.clone().requires_grad_()

            def lib_call():
                ops.infonce(v1, v2, args.tau, True, grad1=g1, grad2=g2, loss=loss, workspace=ws)

            def torch_call():
                a1.grad = a2.grad = None
                torch_formula(a1, a2, args.tau).backward()

            for f in (lib_call, torch_call):       # warm-up: code objects, rocBLAS algorithm choice
                for _ in range(3):
                    f()
            torch.cuda.synchronize()
            times = {"lib": [], "torch": []}
            for _ in range(args.rounds):
                for name, f in (("lib", lib_call), ("torch", torch_call)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        f()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
            # the two sides compute the same loss (fp32 vs fp32)
            torch_loss = torch_formula(v1, v2, args.tau).item()
            lib_call()
            torch.cuda.synchronize()
            lib_us, torch_us = statistics.median(times["lib"]), statistics.median(times["torch"])
            flop = 8.0 * n * n * d
            rows.append({"n": n, "d": d, "lib_us": round(lib_us, 2), "torch_us": round(torch_us, 2),
                         "speedup": round(torch_us / lib_us, 2), "lib_tflops": round(flop / lib_us / 1e6, 1),
                         "lib_frac_of_fp32_peak": round(flop / lib_us / 1e6 / PEAK_TF, 3),
                         "lib_us_spread": [round(min(times["lib"]), 2), round(max(times["lib"]), 2)],
                         "loss_rel_diff": abs(loss.item() - torch_loss) / abs(torch_loss)})
            print(json.dumps(rows[-1]), flush=True)
            del ws
    rec = {"tool": "tools/cl_ab.py", "tau": args.tau, "rounds": args.rounds, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "infonce": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
