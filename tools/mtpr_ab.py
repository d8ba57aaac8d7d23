"""A/B on one device.  Default: one fused MTPR loss call (forward + backward, csrc/mtpr.hip through ops.mtpr) against the
torch formula of the reference (model/MTPR.py:140-202, as tests/mtpr_restate.py states it) under autograd, on the same
tables, projections and content rows; both arms produce the two dense table gradients and the gradients of the content
rows, weu and wei.  The fused arm is timed twice: the call alone on a prepared plan (its two gradient tables zeroed
first, which a trainer does not pay: the Adagrad kernel clears what it consumes), and with ``ops.mtpr_plan`` -- the
grouping of the step's ids, which a trainer pays once per step -- in front of it.
With --step: a whole training step -- content[ids] @ W, the loss, R_w, backward, Adam over [W, weu] and [wei], Adagrad
over the tables -- with the trainer's fused operator and ``ops.adagrad_rows`` against the same step with the torch
formula and ``torch.optim.Adagrad``.

    python tools/mtpr_ab.py [--cold_object item|user] [--batch 4096] [--d 64] [--users 6040] [--items 3706] [--rounds 30]
    python tools/mtpr_ab.py --step [...]

The arms are interleaved round by round after a warm-up; every sample is ``--calls`` calls between two device events.
Prints one JSON line with the medians, the extremes of every arm (the run-to-run spread) and the largest difference of the
gradients (or, with --step, of the five trained tensors after three steps).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402
from tests.mtpr_restate import P_CTX, P_EMB, P_PROJ, loss_terms  # noqa: E402  (the torch formula)


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


def _problem(a, dev):
    """Tables and projections xavier-sized, ids uniform with repeats."""
    g = torch.Generator().manual_seed(0)
    cold_user, d = a.cold_object == "user", a.d
    wp, wq = (d, 2 * d) if cold_user else (2 * d, d)
    r = lambda rows, cols: ((torch.rand(rows, cols, generator=g) * 2 - 1) * (6.0 / (rows + cols)) ** 0.5).to(dev)
    P, Q, W, weu, wei = r(a.users, wp), r(a.items, wq), r(a.content_dim, d), r(2 * d, d), r(2 * d, d)
    content = torch.randn(a.users if cold_user else a.items, a.content_dim, generator=g).to(dev)
    users, pos, neg = (torch.randint(n, (a.batch,), generator=g).to(dev) for n in (a.users, a.items, a.items))
    return cold_user, P, Q, W, weu, wei, content, users, pos, neg


def loss_ab(a, dev):
    cold_user, P, Q, W, weu, wei, content, users, pos, neg = _problem(a, dev)
    h = (content[users if cold_user else torch.cat([pos, neg])] @ W).contiguous()
    wd1 = 0.01
    rng = ((0, a.users - 1), (0, a.items - 1))
    plan = ops.mtpr_plan(users, pos, neg, id_range=rng)
    ws = ops.mtpr_workspace(a.batch, a.d, cold_user, plan["n_items"], plan["n_users"], dev)
    bufs = [torch.zeros_like(P), torch.zeros_like(Q), torch.empty_like(h), torch.empty_like(weu), torch.empty_like(wei)]
    loss = torch.empty(6, device=dev)
    leaves = [t.clone().requires_grad_() for t in (P, Q, h, weu, wei)]

    def fused(p=plan):
        bufs[0].zero_()
        bufs[1].zero_()
        ops.mtpr(P, Q, h, weu, wei, p, wd1, cold_user=cold_user, grad_user=bufs[0], grad_item=bufs[1], grad_h=bufs[2],
                 grad_weu=bufs[3], grad_wei=bufs[4], loss=loss, workspace=ws)

    def fused_with_plan():
        fused(ops.mtpr_plan(users, pos, neg, id_range=rng))

    def formula():
        return torch.autograd.grad(loss_terms(*leaves, users, pos, neg, wd1, cold_user)[5], leaves)

    out = measure(dict(fused=fused, fused_with_plan=fused_with_plan, torch_formula=formula), a.rounds, a.calls)
    ref = formula()
    fused()
    err = [float((b - r).abs().max() / r.abs().max()) for b, r in zip(bufs, ref)]
    m = out["ms_median"]
    out.update(what="loss", cold_object=a.cold_object,
               shape=dict(batch=a.batch, d=a.d, users=a.users, items=a.items), calls_per_sample=a.calls,
               ratio_formula_over_fused=m["torch_formula"] / m["fused"],
               ratio_formula_over_fused_with_plan=m["torch_formula"] / m["fused_with_plan"],
               arms_separated=out["ms_max"]["fused_with_plan"] < out["ms_min"]["torch_formula"], grad_err_over_max=err)
    return out


def step_ab(a, dev):
    from coldrec_amd.model.MTPR import _FusedLoss
    cold_user, P0, Q0, W0, weu0, wei0, content, users, pos, neg = _problem(a, dev)
    (lr1, wd1), (lr2, wd2), (lr3, wd3) = P_EMB, P_CTX, P_PROJ
    src = users if cold_user else torch.cat([pos, neg])
    rng = ((0, a.users - 1), (0, a.items - 1))
    arms, state = {}, {}
    for name in ("fused", "torch_formula"):
        fused = name == "fused"
        P, Q = (torch.nn.Parameter(t.clone(), requires_grad=not fused) for t in (P0, Q0))
        W, weu, wei = (torch.nn.Parameter(t.clone()) for t in (W0, weu0, wei0))
        opts = [torch.optim.Adam([W, weu], lr=lr2), torch.optim.Adam([wei], lr=lr3)]
        if fused:
            bufs = [torch.zeros_like(P), torch.zeros_like(Q), torch.zeros_like(P), torch.zeros_like(Q)]
            ws = ops.mtpr_workspace(a.batch, a.d, cold_user, 2 * a.batch, a.batch, dev)
        else:
            opts.append(torch.optim.Adagrad([P, Q], lr=lr1))
        state[name] = (P, Q, W, weu, wei)

        def step(fused=fused, P=P, Q=Q, W=W, weu=weu, wei=wei, opts=opts, bufs=bufs if fused else None,
                 ws=ws if fused else None):
            h = content[src] @ W
            if fused:
                plan = ops.mtpr_plan(users, pos, neg, id_range=rng)
                total, _ = _FusedLoss.apply(h, weu, wei, P, Q, plan, wd1, cold_user, bufs[0], bufs[1], ws)
            else:
                total = loss_terms(P, Q, h, weu, wei, users, pos, neg, wd1, cold_user)[5]
            total = total + wd2 * ((W * W).sum() + (weu * weu).sum()) + wd3 * (wei * wei).sum()
            for o in opts:
                o.zero_grad()
            total.backward()
            if fused:
                ops.adagrad_rows(P.data, bufs[0], bufs[2], plan["user_ids"], lr1)
                ops.adagrad_rows(Q.data, bufs[1], bufs[3], plan["item_ids"], lr1)
            for o in opts:
                o.step()

        arms[name] = step
    # the arms are compared after three steps each: the timed loop repeats one batch hundreds of times, until the terms
    # saturate and Adam turns the rounding noise of vanishing gradients into steps of its full size.  (Even so the tables
    # differ by 1e-4 .. 1e-3 of their maximum, as float32 and float64 torch do on this problem: Adagrad's first step of an
    # element is lr g / (|g| + eps), which carries the RELATIVE error of a gradient element that happens to lie near zero.)
    for f in arms.values():
        for _ in range(3):
            f()
    diff = [float((x.detach() - y.detach()).abs().max() / y.detach().abs().max())
            for x, y in zip(state["fused"], state["torch_formula"])]
    out = measure(arms, a.rounds, a.calls)
    m = out["ms_median"]
    out.update(what="step", cold_object=a.cold_object,
               shape=dict(batch=a.batch, d=a.d, users=a.users, items=a.items, content_dim=a.content_dim),
               calls_per_sample=a.calls, ratio_formula_over_fused=m["torch_formula"] / m["fused"],
               arms_separated=out["ms_max"]["fused"] < out["ms_min"]["torch_formula"], trained_diff_over_max_after_3_steps=diff)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cold_object", choices=["item", "user"], default="item")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--content_dim", type=int, default=206, help="width of the content rows (206: the synthetic movielens)")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mtpr_ab: needs the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    print(json.dumps(step_ab(a, dev) if a.step else loss_ab(a, dev)))


if __name__ == "__main__":
    main()
