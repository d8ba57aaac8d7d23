"""Time ops.score_topk at the headline shape (131 072 users x 10 M items, d=128, k=20, fp32, rated CSR + a candidate bitmap over a
share of the items) with the item rows scaled by a lognormal factor -- trained tables have norms that vary; the bench's
xavier-uniform rows do not (coefficient of variation 4 %).  One process per setting of CRH_SCORE_SCREEN_ORDER
(tools/screen_order_ab.sh runs 1 and 0 in the same build); prints one JSON line.

    python tools/screen_order_ab.py [--norm-sigma 0.3] [--masked 0.2] [--steps 4] [--warmup 1] [--users 131072] [--items 10000000]"""
import argparse
import json
import os
import sys
import zlib

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from coldrec_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--norm-sigma", type=float, default=0.3, help="sigma of the lognormal row scale of the item table (0: none)")
    ap.add_argument("--masked", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--users", type=int, default=131072)
    ap.add_argument("--items", type=int, default=10_000_000)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    d, k = 128, 20
    g = torch.Generator(device=dev).manual_seed(10)
    U = (torch.rand((a.users, d), device=dev, generator=g) * 2 - 1) * (6.0 / (a.users + d)) ** 0.5
    V = (torch.rand((a.items, d), device=dev, generator=g) * 2 - 1) * (6.0 / (a.items + d)) ** 0.5
    if a.norm_sigma > 0:
        V *= torch.exp(torch.randn((a.items, 1), device=dev, generator=g) * a.norm_sigma)
    lens = torch.randint(0, 40, (a.users,), device=dev, generator=g)
    owner = torch.repeat_interleave(torch.arange(a.users, device=dev), lens)
    key = torch.unique(owner * a.items + torch.randint(0, a.items, owner.shape, device=dev, generator=g))
    rowptr = torch.zeros(a.users + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(key // a.items, minlength=a.users), 0)
    col = (key % a.items).to(torch.int32)
    masked = torch.nonzero(torch.rand(a.items, device=dev, generator=g) < a.masked).flatten().cpu().numpy()
    bm = ops.make_bitmap(a.items, masked, dev)
    route = ops.score_topk_route(a.users, a.items, d, k, has_bitmap=bm is not None)
    ordered = ops.score_topk_screen_ordered(a.users, a.items, d, k, has_bitmap=bm is not None)
    out = None
    ms = []
    for step in range(a.warmup + a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = ops.score_topk(U, None, V, k, rowptr, col, bm, out=out)
        e1.record()
        torch.cuda.synchronize()
        if step >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    crc = zlib.crc32(out[1].cpu().numpy().tobytes(), zlib.crc32(out[0].cpu().numpy().tobytes()))
    print(json.dumps({"norm_sigma": a.norm_sigma, "masked": a.masked, "order_env": os.environ.get("CRH_SCORE_SCREEN_ORDER", "1"),
                      "screened": route["screened"], "ordered": ordered, "ms_per_step": sum(ms) / len(ms), "ms_min": min(ms),
                      "ms_max": max(ms), "uncertified": ops.score_topk_uncertified() if route["screened"] else None,
                      "result_crc32": crc}))


if __name__ == "__main__":
    main()
