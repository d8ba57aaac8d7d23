#!/usr/bin/env python3
"""Interleaved same-process A/B of the contrastive loss on the MI355X, timed with HIP events.

InfoNCE forward + backward (util/utils.py:61-76 with b_cos): the library's crh_infonce_f32 (one call: loss and both
gradients) against the reference's torch formula (normalize, N x N matmul, log_softmax, diag, mean, autograd back through
all of it) on the same inputs, at N in {1024, 2048, 4096, 16384} and d in {64, 128}.  A and B alternate in rounds; each
round times `--reps` back-to-back calls between two events and the median round is reported.  FLOP model: 8 N^2 d per
call (S and P.Z2 in the row pass, S again and P^T.Z1 in the column pass), against the 157.3 TF fp32 MFMA peak.

    python tools/cl_ab.py [--rounds 7] [--reps 20] [--n 4096] [--d 64] [--out profiles/cl_ab.json]

``--step``: one whole TRAINING STEP of the built-in SimGCL / XSimGCL engines (train.CLEngine, device noise) against the
same step written with this package's hooks under autograd -- HipSparseAdj through torch.sparse.mm, bpr_loss, l2_reg_loss
and InfoNCE of coldrec_amd.util.utils, torch.optim.Adam -- i.e. the module-swap path an unmodified model file takes.  Sizes:
the CiteULike shape (5 551 x 16 980, d = 128, L = 3, B = 4 096) and the toy shape (d = 64, L = 3, B = 512).  Steps are
launched eagerly on both sides; rounds alternate, the median round and the spread are reported.

    python tools/cl_ab.py --step [--rounds 7] [--reps 20] [--out profiles/cl_ab_step.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/cl_ab.py --step --engine-only simgcl --shape citeulike
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


def _step_setup(shape, d, B, dev):
    """Graph, tables and one batch of triples at a dataset shape (synthetic interactions, raw ids = internal ids)."""
    import numpy as np
    from coldrec_amd.data.synth import make_dataset
    from coldrec_amd.util.databuilder import bipartite_norm_adj_csr
    split = make_dataset(shape, "item", seed=1, with_content=False)
    tr = np.asarray(split.warm_train)[:, :2].astype(np.int64)
    U, I = split.user_num, split.item_num
    rowptr, col, val = bipartite_norm_adj_csr(tr[:, 0], tr[:, 1], U, I)
    rng = np.random.default_rng(5)
    pick = rng.choice(tr.shape[0], size=min(B, tr.shape[0]), replace=False)
    u, i = tr[pick, 0].astype(np.int32), tr[pick, 1].astype(np.int32)
    j = rng.integers(0, I, size=u.shape[0]).astype(np.int32)
    g = torch.Generator().manual_seed(3)
    bound = (6.0 / (U + d)) ** 0.5
    U0 = (torch.rand((U, d), generator=g) * 2 - 1) * bound
    V0 = (torch.rand((I, d), generator=g) * 2 - 1) * (6.0 / (I + d)) ** 0.5
    return dict(U=U, I=I, rowptr=rowptr, col=col, val=val, U0=U0, V0=V0,
                u=torch.from_numpy(u).to(dev), i=torch.from_numpy(i).to(dev), j=torch.from_numpy(j).to(dev))


def _autograd_step(su, mode, L, l_cl, eps, tau, cl_rate, reg, lr, dev):
    """The step as a model file writes it, on the package's hooks (every product, loss and Adam under autograd / torch)."""
    import scipy.sparse as sp
    from coldrec_amd.graph import HipSparseAdj
    from coldrec_amd.util.utils import InfoNCE, bpr_loss, l2_reg_loss
    n = su["U"] + su["I"]
    adj = HipSparseAdj.from_scipy(sp.csr_matrix((su["val"], su["col"], su["rowptr"]), shape=(n, n))).to(dev)
    E = torch.nn.Parameter(torch.cat([su["U0"], su["V0"]], 0).to(dev))
    opt = torch.optim.Adam([E], lr=lr)
    U, u, i, j = su["U"], su["u"].long(), su["i"].long(), su["j"].long()

    def encode(perturbed):
        x, layers = E, []
        for _ in range(L):
            x = torch.sparse.mm(adj, x)
            if perturbed:
                x = x + torch.sign(x) * F.normalize(torch.rand_like(x), dim=-1) * eps
            layers.append(x)
        return torch.stack(layers, 1).mean(1), layers

    def step():
        uu, ii = torch.unique(u), torch.unique(i) + U
        if mode == "simgcl":
            rec, v1, v2 = encode(False)[0], encode(True)[0], encode(True)[0]
        else:
            rec, layers = encode(True)
            v1, v2 = rec, layers[l_cl - 1]
        ue, pe, ne = rec[u], rec[i + U], rec[j + U]
        loss = bpr_loss(ue, pe, ne) + l2_reg_loss(reg, ue, pe) + \
            cl_rate * (InfoNCE(v1[uu], v2[uu], tau) + InfoNCE(v1[ii], v2[ii], tau))
        opt.zero_grad()
        loss.backward()
        opt.step()
    return step


def _engine_step(su, mode, L, l_cl, eps, tau, cl_rate, reg, lr, dev):
    from coldrec_amd.train import CLEngine
    eng = CLEngine(su["U0"], su["V0"], su["rowptr"], su["col"], su["val"], L, lr, reg, dev, mode=mode, eps=eps, tau=tau,
                   cl_rate=cl_rate, l_cl=l_cl, noise="device", seed=1)
    plan = ops.build_plans_device(su["u"], su["i"], su["j"], su["u"].shape[0])[0]
    return lambda: eng.step(su["u"], su["i"], su["j"], plan)


def step_main(args):
    dev = torch.device("cuda:0")
    hyper = dict(eps=0.1, tau=0.2, cl_rate=0.5, reg=1e-4, lr=1e-3)
    sizes = {"citeulike": (128, 3, 4096), "toy": (64, 3, 512)}
    rows = []
    for shape in ([args.shape] if args.shape else ["citeulike", "toy"]):
        d, L, B = sizes[shape]
        su = _step_setup(shape, d, B, dev)
        for mode in ([args.engine_only] if args.engine_only else ["simgcl", "xsimgcl"]):
            sides = {"engine": _engine_step(su, mode, L, 2, dev=dev, **hyper)}
            if not args.engine_only:
                sides["autograd"] = _autograd_step(su, mode, L, 2, dev=dev, **hyper)
            for f in sides.values():
                for _ in range(5):
                    f()
            torch.cuda.synchronize()
            times = {k: [] for k in sides}
            for _ in range(args.rounds):
                for name, f in sides.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        f()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.reps)
            row = {"shape": shape, "mode": mode, "d": d, "layers": L, "batch": int(su["u"].shape[0]),
                   "rows": su["U"] + su["I"], "edges": int(su["rowptr"][-1])}
            for name, t in times.items():
                row[name + "_step_us"] = round(statistics.median(t), 1)
                row[name + "_step_us_spread"] = [round(min(t), 1), round(max(t), 1)]
            if "autograd" in times:
                row["speedup"] = round(row["autograd_step_us"] / row["engine_step_us"], 2)
            rows.append(row)
            print(json.dumps(row), flush=True)
    rec = {"tool": "tools/cl_ab.py --step", "rounds": args.rounds, "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "hyper": hyper, "steps": rows}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="time one training step of the built-in engines (see the docstring)")
    ap.add_argument("--shape", choices=["citeulike", "toy"], default=None, help="--step: one shape only")
    ap.add_argument("--engine-only", choices=["simgcl", "xsimgcl"], default=None,
                    help="--step: run the engine of one mode alone (for a kernel trace)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--tau", type=float, default=0.2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, nargs="*", default=[1024, 2048, 4096, 16384])
    ap.add_argument("--d", type=int, nargs="*", default=[64, 128])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cl_ab.py measures on the GPU; no GPU is visible")
    if args.step:
        return step_main(args)
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
