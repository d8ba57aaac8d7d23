#!/usr/bin/env python3
"""Price a lane-private top-m screen before building it.

In the fp16 DMA kernel a lane (i, h) holds rows (r & 3) + 8 (r >> 2) + 4 h of every 32-row tile for its users, i.e. the items
with ((item >> 2) & 1) == h.  If each lane kept only its own m best (score, id) pairs, the threshold T_L of a lane (its m-th best
once full) would bound every item it dropped, so the certificate e_k > max(T_L, ...) + B_u fails whenever one half holds m or more
of a user's top k.  This prints that probability exactly (the top k's halves are independent fair coins when item ids carry no
score order) and measured on tables drawn like the bench's (xavier-uniform, d = 128).

    python tools/screen_lane_sim.py [--users 2048 --items 1000000]
"""
import argparse
from math import comb

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=2048)
    ap.add_argument("--items", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--headline-users", type=int, default=131072)
    args = ap.parse_args()
    k, nu, ni, d = args.k, args.users, args.items, 128
    print("m  P(uncertified)  users of %d" % args.headline_users)
    for m in range(k // 2 + 4, k + 2):
        p = sum(comb(k, j) for j in range(k + 1) if max(j, k - j) >= m) / 2 ** k
        print("%-2d %.5f         %.0f" % (m, p, p * args.headline_users))
    rng = np.random.default_rng(0)
    U = ((rng.random((nu, d), dtype=np.float32) * 2 - 1) * np.sqrt(6 / (1_000_000 + d))).astype(np.float32)
    V = ((rng.random((ni, d), dtype=np.float32) * 2 - 1) * np.sqrt(6 / (10_000_000 + d))).astype(np.float32)
    half = (np.arange(ni) >> 2) & 1
    in_h1 = np.empty(nu, np.int64)
    for u0 in range(0, nu, 256):
        S = U[u0:u0 + 256] @ V.T
        top = np.argpartition(-S, k, axis=1)[:, :k]
        in_h1[u0:u0 + 256] = half[top].sum(1)
    worst = np.maximum(in_h1, k - in_h1)
    for m in (16, 18, 20):
        print("tables like the bench's (%d x %d): m = %d leaves %.4f of the users uncertified" % (nu, ni, m, np.mean(worst >= m)))


if __name__ == "__main__":
    main()
