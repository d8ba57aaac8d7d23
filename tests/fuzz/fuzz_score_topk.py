#!/usr/bin/env python3
"""Randomised parity fuzzing of the scoring kernels against the canonical oracle (tests-style tool: it imports
oracle/).  Draws shapes, widths, k, mask densities, split counts, layouts and dtypes for --minutes, checks
bit-exact scores + indices (fp32, and fp16 on exact-arithmetic tables) and prints a summary line.  A few cases (all of them
with --shards) rank the catalogue as the ranks of the sharded evaluation do: 2 .. 8 shards (``shard_bounds`` or random cuts off
the tile grid), one launch per shard with item_base = lo, merged, against the one-launch ranking bitwise and every shard against
the oracle on sampled users.  A shard case is drawn from its own generator, seeded (seed, case): its failure line names it and
``tools/fuzz_case_replay.py --score-shard SEED CASE`` replays it alone.

    python tests/fuzz/fuzz_score_topk.py --minutes 5 [--seed 0] [--shards]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from coldrec_amd import ops  # noqa: E402
from oracle import oracle_np as orc  # noqa: E402

SWITCHES = ("CRH_SCORE_WG", "CRH_SCORE_DMA", "CRH_SCORE_SEED")


def shard_case(seed, case, dev, verbose=False):
    """One sharded case drawn from default_rng([seed, case]).  Returns (ok, description)."""
    from coldrec_amd.eval import ShardedTopK, shard_bounds
    rng = np.random.default_rng([seed, case])
    world = int(rng.integers(2, 9))
    half = rng.random() < 0.35
    d = int(rng.choice([16, 32, 64, 128, 256] if half else [8, 16, 32, 64, 128, 256, 24, 100]))
    k = int(rng.choice([1, 5, 20, 20, 33, 64, 128]))
    kind = rng.choice(["small", "big", "seeded"], p=[0.55, 0.3, 0.15])
    if kind == "big":                                  # workgroup / DMA kernels (with CRH_SCORE_WG=2)
        n_users, n_items = int(rng.integers(32768, 34000)), int(rng.integers(world * 40, 24000))
        if d not in (64, 128, 256):
            d = int(rng.choice([64, 128, 256] if half else [64, 128]))
    elif kind == "seeded":                             # every shard >= 65 536 items, few users
        n_users, n_items = int(rng.integers(1, 500)), world * int(rng.integers(65536, 70000))
        d = 16 if half else int(rng.choice([8, 16]))
    else:
        n_users, n_items = int(rng.integers(1, 700)), int(rng.integers(world, 40000))
    if rng.random() < 0.5:
        cuts = [shard_bounds(n_items, world, r)[0] for r in range(world)] + [n_items]
    else:                                              # random cuts, a third of them pushed off the grid by 1 or 31
        inner = rng.choice(np.arange(1, n_items), world - 1, replace=False)
        inner = np.where(rng.random(world - 1) < 0.33, (inner // 32) * 32 + rng.choice([1, 31], world - 1), inner)
        cuts = [0] + sorted(set(int(c) for c in np.clip(inner, 1, n_items - 1))) + [n_items]
    if any(hi <= lo for lo, hi in zip(cuts[:-1], cuts[1:])):
        cuts = [shard_bounds(n_items, world, r)[0] for r in range(world)] + [n_items]
    world = len(cuts) - 1
    quant = half or rng.random() < 0.5
    if quant:
        q = int(rng.choice([2, 4, 8]))
        U = (rng.integers(-q, q + 1, (n_users, d)) / q).astype(np.float32)
        V = (rng.integers(-q, q + 1, (n_items, d)) / q).astype(np.float32)
    else:
        U = (rng.standard_normal((n_users, d)) * 0.3).astype(np.float32)
        V = (rng.standard_normal((n_items, d)) * 0.3).astype(np.float32)
    mean_r = int(rng.choice([0, 3, 30]))
    lens = rng.poisson(mean_r, n_users) if mean_r else np.zeros(n_users, np.int64)
    rated = [np.unique(x) for x in np.split(rng.integers(0, n_items, int(lens.sum())), np.cumsum(lens)[:-1])]
    for c in cuts[1:-1]:                               # some users rated at the boundaries
        u = int(rng.integers(0, n_users))
        rated[u] = np.union1d(rated[u], [c - 1, c])
    frac = float(rng.choice([0.0, 0.05, 0.2, 0.9]))
    bm_ids = np.where(rng.random(n_items) < frac)[0] if frac else np.zeros(0, np.int64)
    bm_ids = np.union1d(bm_ids, np.clip(np.array([c + o for c in cuts[1:-1] for o in (-1, 0, 31, 32)], np.int64), 0, n_items - 1))
    use_idx = rng.random() < 0.4 and kind != "big"
    users = rng.permutation(n_users)[: max(1, n_users // 2)].astype(np.int64) if use_idx else None
    splits = int(rng.choice([0, 0, 1, 3]))
    env = {}
    if kind == "big" and rng.random() < 0.7:
        env["CRH_SCORE_WG"] = "2"
    env["CRH_SCORE_DMA"] = str(rng.choice(["1", "0", "2", "3"]))
    env["CRH_SCORE_SEED"] = str(rng.choice(["1", "0", "2"]))
    for v in SWITCHES:
        os.environ.pop(v, None)
    os.environ.update(env)
    nq = n_users if users is None else len(users)
    q_rated = rated if users is None else [rated[u] for u in users]
    rp_u = np.concatenate([[0], np.cumsum([len(r) for r in q_rated])]).astype(np.int64)
    col_u = np.concatenate(q_rated).astype(np.int64) if rp_u[-1] else np.zeros(0, np.int64)
    tdt = torch.float16 if half else torch.float32
    tU, tV = torch.from_numpy(U).to(dev).to(tdt), torch.from_numpy(V).to(dev).to(tdt)
    rp_t = torch.from_numpy(rp_u).to(dev) if rp_u[-1] else None
    rc_t = torch.from_numpy(col_u.astype(np.int32)).to(dev) if rp_u[-1] else None
    bm_t = ops.make_bitmap(n_items, bm_ids, dev)
    tu = None if users is None else torch.from_numpy(users.astype(np.int32)).to(dev)
    S, I, routes = [], [], []
    for r in range(world):
        lo, hi = cuts[r], cuts[r + 1]
        x = ops.score_topk_route(nq, hi - lo, d, k, half=half, has_bitmap=bm_t is not None, n_splits=splits)
        routes.append("%s%s%s" % (x["route"], "+seeded" if x["seeded"] else "", "/" + x["dma_form"] if x["dma_form"] else ""))
        if verbose:
            print("shard %d [%d, %d) base %% 32 = %d: %s" % (r, lo, hi, lo % 32, routes[r]))
        s, i = ShardedTopK(tV[lo:hi], lo, n_items, k).topk(tU, tu, rp_t, rc_t, bm_t, n_splits=splits)
        S.append(s)
        I.append(i)
    ms, mi = ops.merge_topk(torch.stack(S), torch.stack(I), k)
    us, ui = ops.score_topk(tU, tu, tV, k, rp_t, rc_t, bm_t)
    torch.cuda.synchronize()
    desc = dict(seed=seed, case=case, world=world, cuts=cuts, routes=routes, half=half, d=d, k=k, n_users=n_users,
                n_items=n_items, quant=quant, mean_r=mean_r, frac=frac, use_idx=use_idx, splits=splits, env=env)
    what = []
    if not (torch.equal(mi, ui) and torch.equal(ms.view(torch.int32), us.view(torch.int32))):
        bad = ((mi != ui).any(1) | (ms.view(torch.int32) != us.view(torch.int32)).any(1)).nonzero().flatten()[:8].tolist()
        what.append("merged != unsharded for users %s" % bad)
    if quant or not half:                              # every shard against the oracle, exact arithmetic
        pick = np.arange(nq) if nq <= 48 else np.unique(np.concatenate([[0, 63, 64, 127, 128, nq - 1], rng.choice(nq, 24)]))
        pick = pick[pick < nq]
        q_users = pick if users is None else users[pick]
        prp = np.concatenate([[0], np.cumsum([len(rated[u]) for u in q_users])]).astype(np.int64)
        pcol = np.concatenate([rated[u] for u in q_users]).astype(np.int64) if prp[-1] else None
        bm_o = orc.make_bitmap(n_items, bm_ids) if len(bm_ids) else None
        for r in range(world):
            lo, hi = cuts[r], cuts[r + 1]
            ws, wi = orc.score_topk(U, q_users, V[lo:hi], k, prp if prp[-1] else None, pcol, bm_o, item_base=lo)
            gs, gi = S[r].cpu().numpy()[pick], I[r].cpu().numpy()[pick]
            if not (np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))):
                rows = np.where((gi != wi).any(1) | (gs.view(np.uint32) != ws.view(np.uint32)).any(1))[0]
                what.append("shard %d [%d, %d) (%s) != oracle for users %s" % (r, lo, hi, routes[r], pick[rows][:8].tolist()))
    for v in SWITCHES:
        os.environ.pop(v, None)
    return not what, dict(desc, failures=what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--minutes", type=float, default=5.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--shards", action="store_true", help="every case is a sharded case")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(args.seed)
    t_end = time.time() + args.minutes * 60
    n_cases = n_big = n_seeded = n_many = n_shard = 0
    pick_shard = np.random.default_rng([args.seed, 1 << 30])      # its own stream: the other cases draw as they always did
    next_report = time.time() + 60
    while time.time() < t_end:
        if time.time() > next_report:                              # a long run reports once a minute
            print(f"... {n_cases} cases ({n_shard} sharded)", flush=True)
            next_report += 60
        if args.shards or pick_shard.random() < 0.03:
            ok, desc = shard_case(args.seed, n_cases, dev)
            if not ok:
                print("MISMATCH shard", desc, flush=True)
                sys.exit(1)
            n_cases += 1
            n_shard += 1
            continue
        half = rng.random() < 0.35
        d = int(rng.choice([16, 32, 64, 128, 256] if half else [8, 16, 32, 64, 128, 256, 24, 100]))
        k = int(rng.choice([1, 5, 10, 20, 20, 20, 33, 64, 100, 128]))
        big = rng.random() < 0.15                       # workgroup-kernel territory
        n_users = int(rng.integers(32768, 34000)) if big else int(rng.integers(1, 700))
        n_items = int(rng.integers(1, 3000)) if big else int(rng.integers(1, 40000))
        # seeded-route territory (catalogues of >= 65 536 items: score_topk_any ranks a prefix by the dense route and seeds the
        # fused selection with it): few users (the item range is cut; prefix = 1/16 of the catalogue) or, fp32, users that fill
        # the chip on their own (no cuts; 4 096-item prefix)
        seeded = (not big) and rng.random() < 0.05
        many = seeded and rng.random() < 0.4
        if seeded:
            n_items = int(rng.integers(65536, 80000))
            if many:
                half, n_users = False, 131072 + int(rng.integers(0, 200))
            d = 16 if half else int(rng.choice([8, 16]))
        quant = half or rng.random() < 0.5              # exact arithmetic / heavy ties
        if quant:
            q = int(rng.choice([2, 4, 8]))
            U = (rng.integers(-q, q + 1, (n_users, d)) / q).astype(np.float32)
            V = (rng.integers(-q, q + 1, (n_items, d)) / q).astype(np.float32)
        else:
            U = (rng.standard_normal((n_users, d)) * 0.3).astype(np.float32)
            V = (rng.standard_normal((n_items, d)) * 0.3).astype(np.float32)
        base = int(rng.choice([0, 0, 31, 4096, 100003]))
        n_glob = base + n_items + int(rng.integers(0, 100))
        mean_r = int(rng.choice([0, 3, 30, 200]))
        if many:
            mean_r = min(mean_r, 3)
        rated = [np.unique(rng.integers(base, base + n_items, rng.poisson(mean_r))) if mean_r else np.zeros(0, np.int64)
                 for _ in range(n_users)]
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rated])]).astype(np.int64)
        col = np.concatenate(rated).astype(np.int64) if rowptr[-1] else np.zeros(0, np.int64)
        frac = float(rng.choice([0.0, 0.05, 0.2, 0.9, 1.0]))
        bm_ids = np.where(rng.random(n_glob) < frac)[0] if frac else None
        use_idx = rng.random() < 0.5 and not big and not many
        users = rng.permutation(n_users)[: max(1, n_users // 2)].astype(np.int64) if use_idx else None
        splits = int(rng.choice([0, 0, 1, 2, 7]))
        if seeded:
            splits = 0                                   # a caller that names a split count gets the plain fused selection
        # fp32 launches take the workgroup kernel from 2 M items only; CRH_SCORE_WG=2 (read per call) forces it here
        if big and rng.random() < 0.6:
            os.environ["CRH_SCORE_WG"] = "2"
        else:
            os.environ.pop("CRH_SCORE_WG", None)
        pack = bool(rng.random() < 0.7)
        sel = slice(None) if users is None else users
        nq = n_users if users is None else len(users)
        if users is not None:
            rp_u = np.concatenate([[0], np.cumsum([len(rated[u]) for u in users])]).astype(np.int64)
            col_u = np.concatenate([rated[u] for u in users]).astype(np.int64) if rp_u[-1] else np.zeros(0, np.int64)
        else:
            rp_u, col_u = rowptr, col
        tdt = torch.float16 if half else torch.float32
        tU, tV = torch.from_numpy(U).to(dev).to(tdt), torch.from_numpy(V).to(dev).to(tdt)
        if not half and d in (24, 100):
            pass                                         # ops pads the width (exact)
        srp, src = orc.sort_rated(rp_u, col_u)
        rp_t = torch.from_numpy(srp).to(dev) if rp_u[-1] else None
        rc_t = torch.from_numpy(src).to(dev) if rp_u[-1] else None
        bm_t = ops.make_bitmap(n_glob, bm_ids, dev)
        tu = None if users is None else torch.from_numpy(users.astype(np.int32)).to(dev)
        s, i = ops.score_topk(tU, tu, tV, k, rp_t, rc_t, bm_t, item_base=base, n_splits=splits, pack=pack)
        torch.cuda.synchronize()
        # oracle on a sample of the queried users (all of them when small)
        pick = np.arange(nq) if nq <= 96 else np.sort(rng.choice(nq, 64, replace=False))
        q_users = pick if users is None else users[pick]
        prp = np.concatenate([[0], np.cumsum([len(rated[u]) for u in q_users])]).astype(np.int64)
        pcol = np.concatenate([rated[u] for u in q_users]).astype(np.int64) if prp[-1] else np.zeros(0, np.int64)
        bm_o = orc.make_bitmap(n_glob, bm_ids) if bm_ids is not None and len(bm_ids) else None
        ws, wi = orc.score_topk(U, q_users.astype(np.int64), V, k, prp if prp[-1] else None, pcol if prp[-1] else None,
                                bm_o, item_base=base)
        gs, gi = s.cpu().numpy()[pick], i.cpu().numpy()[pick]
        ok = np.array_equal(gi, wi) and np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
        if not ok:
            print("MISMATCH", dict(half=half, d=d, k=k, n_users=n_users, n_items=n_items, quant=quant, base=base, seeded=seeded,
                                   mean_r=mean_r, frac=frac, use_idx=use_idx, splits=splits, pack=pack, seed=args.seed,
                                   case=n_cases), flush=True)
            sys.exit(1)
        n_cases += 1
        n_big += big
        n_seeded += seeded
        n_many += many
    print(f"fuzz ok: {n_cases} random cases ({n_big} in workgroup-kernel territory, {n_seeded} in seeded-route territory of which "
          f"{n_many} with users that fill the chip, {n_shard} sharded) bit-exact vs the oracle, seed {args.seed}")


if __name__ == "__main__":
    main()
