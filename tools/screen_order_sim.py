#!/usr/bin/env python3
"""CPU model of the bookkeeping of the screened route's fp16 pass, to price the order its rows are streamed in.

One workgroup: 512 users in 4 waves of 128, K' = 28 candidates per user, lists seeded exactly from the first 8 192 ids, then the
live rows of the main range in tiles of 32.  A wave has an event in a tile when any of its users has a row above the user's
current K'-th score; the workgroup waits at the tile's barrier whenever any of its four waves has one.  The model counts, for the
ascending order and for the order by descending norm key (the high 16 bits of the fp32 sum of squares, ascending id inside a key):
events per wave, tiles in which any wave has an event, and the sum over tiles of the busiest wave's candidates.  Tables are drawn
like the bench's (uniform, xavier bound); --norm-sigma scales the item rows by a lognormal factor.

Every count is printed with the MARGIN rule off and on: with it, once a list is full, a row is a candidate only above
max(K'-th score, k-th score - M), M = 2 (1 + 2^-10) max B_u from the error bound of oracle/screen_model.py (k = 20).

With rated lists drawn like the bench's (bench_legs.common.rated_lists over the live items) the model also counts, per wave and for
the order by norm with the rule on, what stage 1's rated lookups see: the entering candidates that HIT their user's 192-bit
membership filter (each such hit is a trip to memory: list bounds, then the search), and the candidates that lie in a tile some
user of the wave rated -- the only ones that need the filter at all (the rated-tile flags).  filter_fill and
flagged_tiles give the two rates behind those counts for any lists: the mean fraction of filter bits a user's list sets, and the
fraction of a stream's tiles in which a wave's 128 users rated a row.

    python tools/screen_order_sim.py [--items 8000000] [--users 512] [--norm-sigma 0.0]
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import screen_model as sm  # noqa: E402

KP, SEED, TILE, WAVE, K = 28, 8192, 32, 128, 20


def margin(U, V, chunk=65536):
    """M of the call in the scores' own units: the item maxima chunk by chunk, B_u of every user, 2 (1 + 2^-10) times the largest."""
    e_i, e_u = sm.scale_exp(V), sm.scale_exp(U)
    R = N = Nh = 0.0
    for c0 in range(0, len(V), chunk):
        v = V[c0:c0 + chunk]
        vn, vhn, vdn = sm.row_norms(v, sm.f16_copy(v, e_i))
        R, N, Nh = max(R, float(vdn.max())), max(N, float(vn.max())), max(Nh, float(vhn.max()))
    un, uhn, udn = sm.row_norms(U, sm.f16_copy(U, e_u))
    B, _ = sm.bound(un, uhn, udn, R, N, Nh)
    return np.float32(2.0 * (1.0 + 2.0 ** -10) * B.max()), float(B.max())


def norm_keys(V):
    ss = np.einsum("ij,ij->i", V, V, dtype=np.float32)
    return (ss.view(np.uint32) >> 16).astype(np.int64)


FILTER_BITS = 192


def hash192(ids):
    """rated_hash192 of score_topk_dma.hip: the filter bit of each id."""
    h = (np.asarray(ids, np.int64) * 2654435761) & 0xFFFFFFFF
    return ((h >> 16) * FILTER_BITS) >> 16


def filter_fill(rowptr, col, users, lo, hi):
    """Fraction of its 192 filter bits that each of `users` sets with its rated ids in [lo, hi): the rate at which an UNRATED
    candidate of that user hits the filter."""
    out = np.empty(len(users))
    for n, u in enumerate(users):
        ids = col[rowptr[u]:rowptr[u + 1]]
        ids = ids[(ids >= lo) & (ids < hi)]
        out[n] = len(np.unique(hash192(ids))) / FILTER_BITS
    return out


def flagged_tiles(rowptr, col, row_of, n_rows, n_waves, group=WAVE):
    """Per group of `group` consecutive users (a wave: 128; a workgroup: 512) the fraction of the stream's 32-row tiles that hold a
    row one of them rated.  row_of[id] = the id's row in the stream, -1 for an id that is not streamed (prefix, cold)."""
    n_tiles = (n_rows + TILE - 1) // TILE
    out = np.empty(n_waves)
    for w in range(n_waves):
        ids = col[rowptr[w * group]:rowptr[(w + 1) * group]]
        rows = row_of[ids]
        out[w] = len(np.unique(rows[rows >= 0] // TILE)) / n_tiles
    return out


def stream(U, V, order, chunk=8192, M=None, rated=None):
    """Events of streaming V[order] behind the seed prefix; returns (events per wave, busy tiles, sum of busiest-wave candidates).
    M: the margin rule's M (None: the thresholds are the K'-th scores).  rated = (rowptr, col) over the ids of V: the result gains
    (entering candidates, those that hit their user's filter, those in a tile their wave rated), each a mean per wave."""
    nu = U.shape[0]
    n_waves = nu // WAVE
    lists = -np.sort(-(U @ V[:SEED].T), axis=1)[:, :KP].copy()      # descending; column KP-1 is the threshold
    n_tiles = (len(order) + TILE - 1) // TILE
    cand = np.zeros((n_tiles, n_waves), np.int32)
    if rated is not None:
        rowptr, col = rated
        filt = np.zeros((nu, FILTER_BITS), bool)
        flag = np.zeros((n_tiles, n_waves), bool)
        row_of = np.full(len(V), -1, np.int64)
        row_of[order] = np.arange(len(order))
        for u in range(nu):
            ids = col[rowptr[u]:rowptr[u + 1]]
            ids = ids[ids >= SEED]
            filt[u, hash192(ids)] = True
            flag[row_of[ids] // TILE, u // WAVE] = True
        n_cand, n_hit, n_flag = np.zeros(n_waves), np.zeros(n_waves), np.zeros(n_waves)
    for c0 in range(0, len(order), chunk):
        S = U @ V[order[c0:c0 + chunk]].T
        thr = lists[:, KP - 1:KP] if M is None else np.maximum(lists[:, KP - 1:KP], lists[:, K - 1:K] - M)
        us, ps = np.nonzero(S > thr)                                 # a superset: thresholds only rise inside the chunk
        for j in np.argsort(ps, kind="stable"):
            u, p = us[j], ps[j]
            s = S[u, p]
            if s > (lists[u, KP - 1] if M is None else max(lists[u, KP - 1], lists[u, K - 1] - M)):
                row = lists[u]
                q = np.searchsorted(-row, -s)
                row[q + 1:] = row[q:-1]
                row[q] = s
                cand[(c0 + p) // TILE, u // WAVE] += 1
                if rated is not None:
                    n_cand[u // WAVE] += 1
                    n_hit[u // WAVE] += filt[u, hash192(order[c0 + p])]
                    n_flag[u // WAVE] += flag[(c0 + p) // TILE, u // WAVE]
    per_wave = (cand > 0).sum(0).mean()
    res = per_wave, int((cand > 0).any(1).sum()), int(cand.max(1).sum())
    return res if rated is None else res + (n_cand.mean(), n_hit.mean(), n_flag.mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=8_000_000, help="live items (the bench: 10 M less 20 % cold)")
    ap.add_argument("--users", type=int, default=512)
    ap.add_argument("--norm-sigma", type=float, default=0.0)
    a = ap.parse_args()
    d = 128
    rng = np.random.default_rng(0)
    U = ((rng.random((a.users, d), dtype=np.float32) * 2 - 1) * np.sqrt(6 / (1_000_000 + d))).astype(np.float32)
    V = ((rng.random((a.items, d), dtype=np.float32) * 2 - 1) * np.sqrt(6 / (10_000_000 + d))).astype(np.float32)
    if a.norm_sigma > 0:
        V *= np.exp(rng.normal(0.0, a.norm_sigma, (a.items, 1))).astype(np.float32)
    main_ids = np.arange(SEED, a.items)
    keys = norm_keys(V[SEED:])
    by_norm = main_ids[np.argsort(-keys, kind="stable")]
    print("distinct keys in the main range: %d" % len(np.unique(keys)))
    M, Bmax = margin(U, V)
    sd = float((U[:64] @ V[:65536].T).std())
    print("largest B_u %.3g = %.4f sigma of the scores; M = %.3g" % (Bmax, Bmax / sd, M))
    r_id = stream(U, V, main_ids)
    r_nm = stream(U, V, by_norm)
    m_id = stream(U, V, main_ids, M=M)
    from bench_legs.common import rated_lists
    m_nm = stream(U, V, by_norm, M=M, rated=rated_lists(a.users, a.items, 50, seed=4))
    n_cand, n_hit, n_flag = m_nm[3:]
    m_nm = m_nm[:3]
    names = ("events per wave", "tiles where any of the %d waves has an event" % (a.users // WAVE),
             "sum over tiles of the busiest wave's candidates")
    print("| | id order | main range by descending norm key | change |")
    print("|---|---|---|---|")
    for n, x, y in zip(names, r_id, r_nm):
        print("| %s | %.0f | %.0f | %+.1f %% |" % (n, x, y, 100.0 * (y - x) / x))
    print("| with the margin rule | id order | main range by descending norm key | change against the rule off (id order / norm order) |")
    print("|---|---|---|---|")
    for n, x, y, x0, y0 in zip(names, m_id, m_nm, r_id, r_nm):
        print("| %s | %.0f | %.0f | %+.1f %% / %+.1f %% |" % (n, x, y, 100.0 * (x - x0) / x0, 100.0 * (y - y0) / y0))
    print("rated lookups per wave (norm order, rule on, lists like the bench's): %.0f entering candidates, %.0f hit their user's filter "
          "(%.1f %%), %.0f lie in a tile the wave rated (%.1f %%)" % (n_cand, n_hit, 100.0 * n_hit / n_cand, n_flag, 100.0 * n_flag / n_cand))


if __name__ == "__main__":
    main()
