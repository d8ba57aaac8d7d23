"""A/B on one device.  Default: one fused NGCF layer, forward + backward (csrc/ngcf.hip through ops.ngcf_layer_fwd /
ops.ngcf_layer_bwd), against the torch formula of the reference (model/NGCF.py:94-99) under autograd, on the same x, s,
weights and incoming gradient; both arms produce x_k, d s, the gradient that flows to x directly, and the weight and bias
gradients.  The fused forward is also timed alone (x_k only: two tables read, one written) and its achieved bytes/s
printed against the 6.3 TB/s a streaming copy reaches on the MI355X.
With --step: a whole ``train.NGCFEngine.step`` against the step of the G17 plug-in (tests/test_g17_ngcf_plugin_gpu.py): the
same SpMM kernel behind ``torch.sparse.mm``, the same fused BPR / L2 kernels, stock torch under autograd in between, and one
torch.optim.Adam over everything -- on a random bipartite graph of --rows rows and about --degree edges per row.

    python tools/ngcf_ab.py [--rows 1000000] [--d 64] [--rounds 20]
    python tools/ngcf_ab.py --step [--rows 1000000] [--d 64] [--layers 2] [--batch 4096] [--degree 32]

The arms are interleaved round by round after a warm-up; every sample is ``--calls`` calls between two device events.
Prints one JSON line with the medians, the extremes of every arm (the run-to-run spread) and the largest differences.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy on the MI355X


def summary(times):
    return dict(ms_median={k: sorted(v)[len(v) // 2] for k, v in times.items()},
                ms_min={k: min(v) for k, v in times.items()}, ms_max={k: max(v) for k, v in times.items()})


def measure(arms, rounds, calls):
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, f in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(calls):
                f()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / calls)
    return summary(times)


def layer_ab(a, dev):
    n, d, c = a.rows, a.d, 1.0 / 3.0
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, generator=g, device=dev)
    x, s, gk, dout = r(n, d) * 0.5, r(n, d) * 0.5, r(n, d) * 0.1, r(n, d) * 0.1
    w, b = r(2 * d, d) * (0.7 / d ** 0.5), r(2, d) * 0.1
    y, ds, local = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    dw, db = torch.empty_like(w), torch.empty(d, device=dev)
    ws = ops.ngcf_workspace(n, d, dev)
    leaves = [t.clone().requires_grad_() for t in (x, s, w[:d], w[d:], b[0], b[1])]

    def fused_fwd():
        ops.ngcf_layer_fwd(x, s, w, b, y=y)

    def fused():
        ops.ngcf_layer_fwd(x, s, w, b, y=y)
        ops.ngcf_layer_bwd(x, s, y, gk, dout, c, w, ds=ds, local=local, dw=dw, db=db, workspace=ws)

    def formula_fwd():
        with torch.no_grad():
            return F.leaky_relu(F.linear(s, w[:d], b[0]) + F.linear(x * s, w[d:], b[1]))

    def formula():
        lx, ls, wgc, wbi, bgc, bbi = leaves
        xk = F.leaky_relu(F.linear(ls, wgc, bgc) + F.linear(lx * ls, wbi, bbi))
        gx, gs, gwgc, gwbi, gbgc, _ = torch.autograd.grad(xk, leaves, gk)
        return xk.detach(), gs, c * dout + gx, torch.cat([gwgc, gwbi]), gbgc

    out = measure(dict(fused=fused, torch_formula=formula, fused_forward=fused_fwd, torch_forward=formula_fwd), a.rounds,
                  a.calls)
    fused()

    def formula_with_the_kernels_signs():
        # an element with z within rounding of 0 can come out on the other side in the two arms, and its slope then
        # differs by 0.99: the gradients are compared with the slope taken where the fused x_k is positive
        lx, ls, wgc, wbi, bgc, bbi = leaves
        z = F.linear(ls, wgc, bgc) + F.linear(lx * ls, wbi, bbi)
        xk = torch.where(y > 0, z, 0.01 * z)
        gx, gs, gwgc, gwbi, gbgc, _ = torch.autograd.grad(xk, leaves, gk)
        return xk.detach(), gs, c * dout + gx, torch.cat([gwgc, gwbi]), gbgc

    ref = formula_with_the_kernels_signs()
    torch.cuda.synchronize()
    err = [float((p - q).abs().max() / q.abs().max()) for p, q in zip((y, ds, local, dw, db), ref)]
    m = out["ms_median"]
    fwd_bytes = 3 * n * d * 4
    out.update(what="layer", shape=dict(rows=n, d=d), calls_per_sample=a.calls,
               ratio_formula_over_fused=m["torch_formula"] / m["fused"],
               ratio_forward_formula_over_fused=m["torch_forward"] / m["fused_forward"],
               arms_separated=out["ms_max"]["fused"] < out["ms_min"]["torch_formula"],
               forward_bytes=fwd_bytes, forward_bytes_per_s=fwd_bytes / (m["fused_forward"] * 1e-3),
               forward_share_of_hbm_copy_rate=fwd_bytes / (m["fused_forward"] * 1e-3) / HBM_COPY_BYTES_PER_S,
               err_over_max=dict(zip(("x_k", "ds", "local", "dw", "db"), err)))
    return out


def random_graph(n_users, n_items, degree, seed=0):
    """Symmetric normalised adjacency D^-1/2 A D^-1/2 of a random bipartite graph as scipy CSR, about ``degree`` edges per
    row on average (users x items drawn uniformly, duplicates merged)."""
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    m = (n_users + n_items) * degree // 2
    u, i = rng.integers(0, n_users, m), rng.integers(0, n_items, m)
    r = sp.csr_matrix((np.ones(m, np.float32), (u, i)), shape=(n_users, n_items))
    r.data[:] = 1.0
    adj = sp.bmat([[None, r], [r.T, None]], format="csr", dtype=np.float32)
    deg = np.asarray(adj.sum(1)).ravel()
    dinv = np.where(deg > 0, 1.0 / np.sqrt(np.maximum(deg, 1e-12)), 0.0).astype(np.float32)
    adj = sp.diags(dinv) @ adj @ sp.diags(dinv)
    adj = adj.tocsr().astype(np.float32)
    adj.sort_indices()
    return adj


def step_ab(a, dev):
    from coldrec_amd.graph import HipSparseAdj
    from coldrec_amd.train import NGCFEngine
    from coldrec_amd.util.utils import bpr_loss, l2_reg_loss
    n_users = a.rows * 6 // 10
    n_items = a.rows - n_users
    d, L, B = a.d, a.layers, a.batch
    adj = random_graph(n_users, n_items, a.degree)
    g = torch.Generator().manual_seed(0)
    u0, v0 = torch.randn(n_users, d, generator=g) * 0.1, torch.randn(n_items, d, generator=g) * 0.1
    weights = [tuple(torch.randn(sh, generator=g) * sc for sh, sc in (((d, d), 0.1), ((d,), 0.05), ((d, d), 0.1), ((d,), 0.05)))
               for _ in range(L)]
    users, pos, neg = (torch.randint(k, (B,), generator=g, dtype=torch.int32).to(dev) for k in (n_users, n_items, n_items))
    plan = ops.build_plans_device(users, pos, neg, B)[0]
    eng = NGCFEngine(u0, v0, adj.indptr.astype(np.int64), adj.indices.astype(np.int32), adj.data, L, 1e-3, 1e-4, dev, weights)
    eng.keep_grad = True

    # the plug-in's step: parameters under autograd, the SpMM behind torch.sparse.mm
    A = HipSparseAdj.from_scipy(adj).to(dev)
    E = torch.nn.Parameter(torch.cat([u0, v0]).to(dev))
    P = [tuple(torch.nn.Parameter(t.clone().to(dev)) for t in w) for w in weights]
    opt = torch.optim.Adam([E] + [p for w in P for p in w], lr=1e-3)
    ul, pl, nl = users.long(), pos.long(), neg.long()

    def plugin():
        ego, outs = E, [E]
        for wgc, bgc, wbi, bbi in P:
            side = torch.sparse.mm(A, ego)
            ego = F.leaky_relu(F.linear(side, wgc, bgc) + F.linear(ego * side, wbi, bbi))
            outs.append(ego)
        out = torch.mean(torch.stack(outs, dim=1), dim=1)
        ue, pe, ne = out[:n_users][ul], out[n_users:][pl], out[n_users:][nl]
        loss = bpr_loss(ue, pe, ne) + l2_reg_loss(1e-4, ue, pe, ne)
        opt.zero_grad()
        loss.backward()
        opt.step()

    def fused():
        eng.step(users, pos, neg, plan)

    # the first step of both arms, from the same state: the table gradients
    fused()
    plugin()
    torch.cuda.synchronize()
    diff = float((eng.G - E.grad).abs().max() / E.grad.abs().max())
    out = measure(dict(fused=fused, plugin=plugin), a.rounds, a.calls)
    m = out["ms_median"]
    out.update(what="step", shape=dict(rows=a.rows, users=n_users, items=n_items, d=d, layers=L, batch=B, nnz=int(adj.nnz)),
               calls_per_sample=a.calls, ratio_plugin_over_fused=m["plugin"] / m["fused"],
               arms_separated=out["ms_max"]["fused"] < out["ms_min"]["plugin"], first_step_table_grad_diff_over_max=diff)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--degree", type=int, default=32, help="--step: mean edges per row of the random graph")
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=5, help="calls per timed sample")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ngcf_ab: needs the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    print(json.dumps(step_ab(a, dev) if a.step else layer_ab(a, dev)))


if __name__ == "__main__":
    main()
