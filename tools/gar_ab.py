"""A/B on one device.  Default: one fused GAR loss call (forward + backward, csrc/gar.hip through ops.gar) against the torch
formula of the reference (model/GAR.py:24-31, as tests/gar_restate.py states it) under autograd, on the same tables and
generator output; both arms produce the two dense table gradients and the generator output's.  The fused arm is timed
twice: the call alone on a prepared plan (its two gradient tables zeroed first, as a caller must), and with
``ops.gar_plan`` -- the grouping of the step's ids, which a trainer pays once per step -- in front of it.
With --step: a whole training step of the trainer's learner (generator forward, loss, backward, one Adam step over the
generator and both tables) with the fused operator against the same step with the torch formula.

    python tools/gar_ab.py [--cold_object item|user] [--batch 4096] [--d 64] [--users 6040] [--items 3706] [--rounds 30]
    python tools/gar_ab.py --step [...]

The arms are interleaved round by round after a warm-up; every sample is ``--calls`` calls between two device events.
Prints one JSON line with the medians, the extremes of every arm (the run-to-run spread) and the largest difference of the
gradients.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402
from tests.gar_restate import generator, loss_terms  # noqa: E402  (the torch formula)

COEF = (0.05, 0.1, 1e-4)


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
    g = torch.Generator().manual_seed(0)
    U, V = (torch.randn(a.users, a.d, generator=g) * 0.1).to(dev), (torch.randn(a.items, a.d, generator=g) * 0.1).to(dev)
    users, pos, neg = (torch.randint(n, (a.batch,), generator=g).to(dev) for n in (a.users, a.items, a.items))
    return g, U, V, users, pos, neg


def loss_ab(a, dev):
    g, U, V, users, pos, neg = _problem(a, dev)
    cold_user = a.cold_object == "user"
    G = torch.tanh(torch.randn(a.batch, a.d, generator=g) * 0.3).to(dev)
    rng = ((0, a.users - 1), (0, a.items - 1))
    plan = ops.gar_plan(users, pos, neg, id_range=rng)
    ws = ops.gar_workspace(a.batch, a.d, plan["n_items"], plan["n_users"], dev)
    bufs, loss = [torch.zeros_like(U), torch.zeros_like(V), torch.empty_like(G)], torch.empty(4, device=dev)
    leaves = [t.clone().requires_grad_() for t in (U, V, G)]

    def fused(p=plan):
        bufs[0].zero_()
        bufs[1].zero_()
        ops.gar(U, V, G, p, *COEF, cold_user=cold_user, grad_user=bufs[0], grad_item=bufs[1], grad_gen=bufs[2], loss=loss,
                workspace=ws)

    def fused_with_plan():
        fused(ops.gar_plan(users, pos, neg, id_range=rng))

    def formula():
        return torch.autograd.grad(loss_terms(leaves[0], leaves[1], users, pos, neg, leaves[2], *COEF, cold_user)[3], leaves)

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
    from coldrec_amd.model.GAR import _FusedLoss
    g, U, V, users, pos, neg = _problem(a, dev)
    cold_user = a.cold_object == "user"
    content = torch.randn(a.users if cold_user else a.items, a.content_dim, generator=g).to(dev)
    src = users if cold_user else pos
    rng = ((0, a.users - 1), (0, a.items - 1))
    torch.manual_seed(0)
    first = generator(a.content_dim, a.d)
    arms, state = {}, {}
    for name in ("fused", "torch_formula"):
        gen = generator(a.content_dim, a.d)
        gen.load_state_dict(first.state_dict())
        gen = gen.to(dev)
        Up, Vp = torch.nn.Parameter(U.clone()), torch.nn.Parameter(V.clone())
        opt = torch.optim.Adam(list(gen.parameters()) + [Up, Vp], lr=1e-3)
        state[name] = (Up, Vp)

        def step(name=name, gen=gen, Up=Up, Vp=Vp, opt=opt):
            out = gen(content[src])
            if name == "fused":
                total, _ = _FusedLoss.apply(out, Up, Vp, ops.gar_plan(users, pos, neg, id_range=rng), COEF, cold_user)
            else:
                total = loss_terms(Up, Vp, users, pos, neg, out, *COEF, cold_user)[3]
            opt.zero_grad()
            total.backward()
            opt.step()

        arms[name] = step
    out = measure(arms, a.rounds, a.calls)
    diff = [float((x - y).abs().max() / y.abs().max()) for x, y in zip(state["fused"], state["torch_formula"])]
    m = out["ms_median"]
    out.update(what="step", cold_object=a.cold_object,
               shape=dict(batch=a.batch, d=a.d, users=a.users, items=a.items, content_dim=a.content_dim),
               calls_per_sample=a.calls, ratio_formula_over_fused=m["torch_formula"] / m["fused"],
               arms_separated=out["ms_max"]["fused"] < out["ms_min"]["torch_formula"], table_diff_over_max=diff)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cold_object", choices=["item", "user"], default="item")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--content_dim", type=int, default=128, help="width of the content rows of --step's generator")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed sample")
    ap.add_argument("--step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gar_ab: needs the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    print(json.dumps(step_ab(a, dev) if a.step else loss_ab(a, dev)))


if __name__ == "__main__":
    main()
