"""Item-sharded ranking on every scoring route at shard bases off the 32-item tile grid (run with -m gpu on an MI355X).

Rank r of the sharded evaluation ranks item rows [lo, hi) with global ids (``ShardedTopK``, ``item_base = lo``); the lists are
gathered and merged by ``crh_merge_topk``.  ``shard_bounds`` puts most bases at 16 mod 32, and the tile-bit, pack, filter-window
and rated-hash code of the kernels works in global ids, so a slip there only shows off the grid.  Every case here ranks a
catalogue the way the ranks do -- one world-1 launch per shard on a view of the table, then the merge -- and asserts
  (a) merged == the one-launch ranking of the whole table, bit for bit, for every user;
  (b) each shard's list == the C oracle with ``item_base = lo`` on sampled users (fp32 and exact-arithmetic fp16);
  (c) each shard launch took the route the case is for (``ops.score_topk_route``), so that a retuned threshold fails here
      instead of quietly moving the case to another kernel.
Every catalogue carries the boundary edges: bitmap bits at lo-1, lo, lo+31, lo+32, hi-1, hi; users rated only just outside a
shard or exactly at lo / hi-1; rows shared across each boundary (exact ties between shards) that the edge users rank first."""
import os
import subprocess
import sys
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from coldrec_amd import ops
from coldrec_amd.eval import ShardedTopK, shard_bounds
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

PAD = 0x7FFFFFFF
N_WG = 32768 + 77                 # the fewest users that reach the workgroup and DMA kernels (512 groups of 64)
SWITCHES = ("CRH_SCORE_WG", "CRH_SCORE_DMA", "CRH_SCORE_SEED")
HOT_LO, HOT_HI = 12, 40           # rows [B - 12, B + 40) around every inner boundary B share one row


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _off_grid_cuts(n_items, world, residues=(1, 16, 31), tiny_after=None):
    """``world`` shards of ~n_items / world items whose inner bases run through ``residues`` mod 32; ``tiny_after`` = r inserts
    a 7-item shard right after cut r (a shard with fewer items than k)."""
    step = n_items // world
    cuts = [0] + [r * step - (r * step) % 32 + residues[(r - 1) % len(residues)] for r in range(1, world)] + [n_items]
    if tiny_after is not None:
        cuts.insert(tiny_after + 1, cuts[tiny_after] + 7)
    return cuts


def _csr(lists):
    rowptr = np.zeros(len(lists) + 1, np.int64)
    rowptr[1:] = np.cumsum([len(x) for x in lists])
    col = np.concatenate(lists).astype(np.int64) if rowptr[-1] else np.zeros(0, np.int64)
    return rowptr, col


class Catalogue:
    """Tables on the GPU, rated lists and bitmap on both sides, and the edge users of every inner boundary."""

    def __init__(self, seed, n_q, n_items, d, cuts, half=False, quant=False, use_users=False, mean_rated=6,
                 masked_shard=None, thin_user=False, frac=0.1):
        dev = _dev()
        rng = np.random.default_rng(seed)
        g = torch.Generator(device=dev).manual_seed(seed)
        self.n_q, self.n_items, self.d, self.cuts, self.half = n_q, n_items, d, cuts, half
        self.exact = (not half) or quant
        n_rows = n_q + 29 if use_users else n_q
        self.users = rng.permutation(n_rows)[:n_q].astype(np.int64) if use_users else None
        if quant:
            U = torch.randint(-4, 5, (n_rows, d), generator=g, device=dev).float() / 4
            V = torch.randint(-4, 5, (n_items, d), generator=g, device=dev).float() / 4
        else:
            U = torch.randn((n_rows, d), generator=g, device=dev) * 0.3
            V = torch.randn((n_items, d), generator=g, device=dev) * 0.3
        row = (lambda s: s) if self.users is None else (lambda s: int(self.users[s]))
        # every inner boundary B: one shared row over [B-12, B+40) and three users that rank it first -- a plain one (ties across
        # the boundary, canonical order through the merge), one rated at B-3 .. B+2 (only just outside each of the two shards), one
        # rated exactly at B-1 = hi-1 and B = lo and at B+31
        bounds = cuts[1:-1]
        slots = rng.permutation(n_q)[: 3 * len(bounds)] if n_q >= 3 * len(bounds) else np.arange(3 * len(bounds)) % n_q
        self.edge = {}                      # boundary -> its three user slots
        extra = {}
        for j, B in enumerate(bounds):
            h = torch.from_numpy(rng.choice([-1.0, 1.0], d).astype(np.float32) if quant else
                                 (rng.standard_normal(d) * 0.3).astype(np.float32)).to(dev)
            V[max(0, B - HOT_LO):min(n_items, B + HOT_HI)] = h
            trio = [int(x) for x in slots[3 * j:3 * j + 3]]
            self.edge[B] = trio
            for s in trio:
                U[row(s)] = h
            extra.setdefault(trio[1], []).extend([B - 3, B - 2, B - 1, B, B + 1, B + 2])
            extra.setdefault(trio[2], []).extend([B - 1, B, B + 31])
        dt = torch.float16 if half else torch.float32
        self.tU, self.tV = U.to(dt), V.to(dt)
        self.U_host = self.tU.float().cpu().numpy()           # the values the kernels see (fp16: exact on quantised tables)
        lens = rng.poisson(mean_rated, n_q)
        rated = np.split(rng.integers(0, n_items, int(lens.sum())), np.cumsum(lens)[:-1])
        for s, ids in extra.items():
            rated[s] = np.concatenate([rated[s], ids])
        if thin_user:                       # one user whose unmasked catalogue is smaller than k: all but 5 items rated
            self.thin = int(rng.integers(0, n_q))
            rated[self.thin] = np.setdiff1d(np.arange(n_items), rng.choice(n_items, 5, replace=False))
        rated = [np.unique(np.clip(r, 0, n_items - 1)) for r in rated]
        self.rowptr, self.col = _csr(rated)
        self.rated = rated
        cold = [np.where(rng.random(n_items) < frac)[0]]
        for j, B in enumerate([0] + bounds):             # bitmap edges: lo-1, lo, lo+31, lo+32 (and hi-1, hi of the shard before)
            if j % 2 == 0:                                # on every other boundary; the rated edge users sit on all of them
                cold.append(np.array([B - 1, B, B + 31, B + 32]))
        cold.append(np.array([n_items - 1]))
        self.masked_shard = masked_shard
        if masked_shard is not None:
            cold.append(np.arange(cuts[masked_shard], cuts[masked_shard + 1]))
        self.cold = np.unique(np.clip(np.concatenate(cold), 0, n_items - 1))
        self.bm = ops.make_bitmap(n_items, self.cold, dev)
        self.bm_host = orc.make_bitmap(n_items, self.cold)
        self.rp = torch.from_numpy(self.rowptr).to(dev)
        self.rc = torch.from_numpy(self.col.astype(np.int32)).to(dev)
        self.tu = None if self.users is None else torch.from_numpy(self.users.astype(np.int32)).to(dev)

    def sample(self, rng, edge_users=3):
        """Oracle users: first / last and the 64- / 128-user group edges, the edge users of every boundary, two random ones."""
        n = self.n_q
        pick = [u for u in (0, 63, 64, 127, 128, 32767, 32768, n - 1) if u < n]
        for trio in self.edge.values():
            pick += trio[:edge_users]
        pick += list(rng.integers(0, n, 2))
        return np.unique(np.array(pick, np.int64))

    def oracle(self, pick, lo, hi):
        sub_rp, sub_col = _csr([self.rated[s] for s in pick])
        q = pick if self.users is None else self.users[pick]
        Vs = self.tV[lo:hi].float().cpu().numpy()
        return orc.score_topk(self.U_host, q, Vs, self.k_oracle, sub_rp if sub_rp[-1] else None,
                              sub_col if sub_rp[-1] else None, self.bm_host, item_base=lo)


def _route(cat, lo, hi, k, n_splits):
    r = ops.score_topk_route(cat.n_q, hi - lo, cat.d, k, half=cat.half, has_bitmap=True, n_splits=n_splits)
    return (r["route"], r["seeded"], r["dma_form"]), r


def rank_sharded(name, cat, k, n_splits=0, expect=None, expect_small=None, oracle=True, seed=0, edge_users=3):
    """Rank ``cat`` shard by shard as the ranks do, merge, and assert (a), (b), (c).  ``expect``: (route, seeded, dma_form) of
    every shard of >= 1 024 items; ``expect_small``: that of the smaller ones."""
    cuts = cat.cuts
    world = len(cuts) - 1
    S, I, routes = [], [], []
    for r in range(world):
        lo, hi = cuts[r], cuts[r + 1]
        key, info = _route(cat, lo, hi, k, n_splits)
        routes.append(key)
        print(f"[{name}] shard {r}: [{lo}, {hi}) base % 32 = {lo % 32}: {info['route']} seeded={info['seeded']} "
              f"form={info['dma_form']} prefix={info['prefix_items']} cuts={info['n_splits']} ({info['kernel']})")
        want = expect if hi - lo >= 1024 else expect_small
        if want is not None:
            assert key == tuple(want), f"{name}: shard {r} [{lo}, {hi}) took {key}, the case is for {want}"
        s, i = ShardedTopK(cat.tV[lo:hi], lo, cat.n_items, k).topk(cat.tU, cat.tu, cat.rp, cat.rc, cat.bm, n_splits=n_splits)
        S.append(s)
        I.append(i)
    ms, mi = ops.merge_topk(torch.stack(S), torch.stack(I), k)
    us, ui = ops.score_topk(cat.tU, cat.tu, cat.tV, k, cat.rp, cat.rc, cat.bm)
    torch.cuda.synchronize()
    # (a) merged == unsharded, every user
    bad = (mi != ui).any(dim=1) | (ms.view(torch.int32) != us.view(torch.int32)).any(dim=1)
    assert not bool(bad.any()), f"{name}: merged != unsharded for users {torch.nonzero(bad).flatten()[:8].tolist()}"
    mi_h, ms_h = mi.cpu().numpy(), ms.cpu().numpy()
    # the catalogue does what it is built for: the shared rows rank first for the edge users, across each boundary
    crossing = sum(int(((mi_h[s] < B) & (mi_h[s] >= B - HOT_LO)).any() and ((mi_h[s] >= B) & (mi_h[s] < B + HOT_HI)).any())
                   for B, trio in cat.edge.items() for s in trio[:1])
    assert crossing >= len(cat.edge) // 2, f"{name}: only {crossing} edge users rank across their boundary"
    if cat.masked_shard is not None:                      # an all-masked shard lists -1e9 only, and they lose the merge
        r = cat.masked_shard
        assert (S[r].cpu().numpy() == np.float32(-1e9)).all()
        assert not ((mi_h >= cuts[r]) & (mi_h < cuts[r + 1])).any()
    for r in range(world):
        if cuts[r + 1] - cuts[r] < k:                     # a shard of fewer than k items ends in padding
            assert (I[r].cpu().numpy()[:, cuts[r + 1] - cuts[r]:] == PAD).all()
    if oracle and cat.exact:
        # (b) every shard against the oracle with item_base = lo; and the oracle's merge of the oracle lists == merged
        cat.k_oracle = k
        pick = cat.sample(np.random.default_rng(seed), edge_users)
        with ThreadPoolExecutor(max_workers=8) as ex:
            want = list(ex.map(lambda r: cat.oracle(pick, cuts[r], cuts[r + 1]), range(world)))
        for r in range(world):
            gs, gi = S[r].cpu().numpy()[pick], I[r].cpu().numpy()[pick]
            ws, wi = want[r]
            rows = np.where((gi != wi).any(1) | (gs.view(np.uint32) != ws.view(np.uint32)).any(1))[0]
            assert len(rows) == 0, f"{name}: shard {r} [{cuts[r]}, {cuts[r + 1]}) != oracle for users {pick[rows][:8]}"
        os_, oi = orc.merge_topk(np.stack([w[0] for w in want]), np.stack([w[1] for w in want]), k)
        assert np.array_equal(mi_h[pick], oi) and np.array_equal(ms_h[pick].view(np.uint32), os_.view(np.uint32))
    return routes, (ms, mi)


def _env(monkeypatch, env):
    for v in SWITCHES:
        monkeypatch.delenv(v, raising=False)
    for a, b in env.items():
        monkeypatch.setenv(a, b)


# ================================================================================ workgroup, DMA and per-wave kernels
WG2 = {"CRH_SCORE_WG": "2"}
FLAGS = {"CRH_SCORE_WG": "2", "CRH_SCORE_DMA": "2"}
BARRIER = {"CRH_SCORE_WG": "2", "CRH_SCORE_DMA": "3"}
RING = {"CRH_SCORE_WG": "2", "CRH_SCORE_DMA": "0"}
# name: dtype, d, k, users, env, n_splits, users indirection, quantised, expected route, extras
FUSED = {
    "dma-flags-seeded":    ("f32", 128, 20, N_WG, FLAGS, 0, False, False, ("fused-dma", True, "flags"), {"masked_shard": 5}),
    "dma-flags-1":         ("f32", 128, 20, N_WG, FLAGS, 1, True, True, ("fused-dma", False, "flags"), {"tiny_after": 3}),
    "dma-flags-3":         ("f32", 128, 20, N_WG, FLAGS, 3, False, False, ("fused-dma", False, "flags"), {}),
    "dma-barrier-seeded":  ("f32", 128, 20, N_WG, BARRIER, 0, True, False, ("fused-dma", True, "barrier"), {}),
    "dma-barrier-1":       ("f32", 128, 20, N_WG, BARRIER, 1, False, True, ("fused-dma", False, "barrier"), {"masked_shard": 2}),
    "dma-barrier-3":       ("f32", 128, 20, N_WG, BARRIER, 3, True, False, ("fused-dma", False, "barrier"), {"tiny_after": 6}),
    "dma-d64-k20-seeded":  ("f32", 64, 20, N_WG, WG2, 0, False, False, ("fused-dma", True, "barrier"), {}),
    "dma-d64-k28-1":       ("f32", 64, 28, N_WG, WG2, 1, True, True, ("fused-dma", False, "barrier"), {}),
    "dma-d64-k20-3":       ("f32", 64, 20, N_WG, WG2, 3, True, False, ("fused-dma", False, "barrier"), {}),
    "dma-d64-k28-seeded":  ("f32", 64, 28, N_WG, WG2, 0, True, True, ("fused-dma", True, "barrier"), {}),
    "dma-f16-exact-seeded": ("f16", 256, 20, N_WG, {}, 0, True, True, ("fused-dma", True, "barrier"), {}),
    "dma-f16-exact-1":     ("f16", 256, 20, N_WG, {}, 1, False, True, ("fused-dma", False, "barrier"), {"masked_shard": 4}),
    "dma-f16-cont-3":      ("f16", 256, 20, N_WG, {}, 3, True, False, ("fused-dma", False, "barrier"), {}),
    "dma-f16-cont-seeded": ("f16", 256, 20, N_WG, {}, 0, False, False, ("fused-dma", True, "barrier"), {}),
    "ring-f32-seeded":     ("f32", 128, 20, N_WG, RING, 0, False, False, ("fused-wg", True, None), {}),
    "ring-f32-1":          ("f32", 128, 20, N_WG, RING, 1, True, True, ("fused-wg", False, None), {"masked_shard": 1}),
    "ring-f32-3":          ("f32", 128, 20, N_WG, RING, 3, False, True, ("fused-wg", False, None), {}),
    "ring-f16-d64-seeded": ("f16", 64, 20, N_WG, {}, 0, True, True, ("fused-wg", True, None), {}),
    "ring-f16-d128-1":     ("f16", 128, 20, N_WG, {}, 1, False, True, ("fused-wg", False, None), {}),
    "ring-f16-d64-3":      ("f16", 64, 20, N_WG, {}, 3, False, False, ("fused-wg", False, None), {}),
    "ring-f16-d128-seeded": ("f16", 128, 20, N_WG, {}, 0, True, False, ("fused-wg", True, None), {}),
    "wave-d64-k50-1":      ("f32", 64, 50, 333, {}, 1, True, False, ("fused-wave", False, None), {"tiny_after": 2}),
    "wave-d128-k128-3":    ("f32", 128, 128, 333, {}, 3, False, True, ("fused-wave", False, None), {}),
    "wave-d64-k128-3":     ("f32", 64, 128, 333, {}, 3, True, True, ("fused-wave", False, None), {"masked_shard": 3}),
    "wave-d128-k50-1":     ("f32", 128, 50, 333, {}, 1, False, False, ("fused-wave", False, None), {}),
    "seeded-f32-d64":      ("f32", 64, 20, 333, {}, 0, True, False, ("fused-wave", True, None), {"thin_user": True}),
    "seeded-f32-d128-k50": ("f32", 128, 50, 333, {"CRH_SCORE_SEED": "2"}, 0, False, True, ("fused-wave", True, None), {}),
    "seeded-f16-d128":     ("f16", 128, 20, 333, {}, 0, True, True, ("fused-wave", True, None), {"masked_shard": 6}),
}


@pytest.mark.parametrize("name", list(FUSED))
def test_fused_routes_sharded_off_grid(name, monkeypatch):
    """8 shards of ~150 000 items (bases 1, 16, 31 mod 32; some cases add a 7-item shard or mask a whole shard) through one
    fused route each: the DMA kernel in both forms at 512- and 256-byte rows and fp16 d=256, the register-staged ring kernel,
    the per-wave kernel, and the seeded route on the per-wave and workgroup kernels; item-range cuts 0 (seeded: the library's
    own cuts), 1 and 3 inside each shard; with and without the ``users`` indirection."""
    dtype, d, k, n_q, env, n_splits, use_users, quant, expect, extra = FUSED[name]
    _env(monkeypatch, env)
    n_items = 8 * 150_000 + 77
    cuts = _off_grid_cuts(n_items, 8, tiny_after=extra.get("tiny_after"))
    cat = Catalogue(zlib.crc32(name.encode()) % 10_000, n_q, n_items, d, cuts, half=dtype == "f16", quant=quant, use_users=use_users,
                    masked_shard=extra.get("masked_shard") if "tiny_after" not in extra else None,
                    thin_user=extra.get("thin_user", False))
    small = None
    if "tiny_after" in extra:           # the 7-item shard: the block route when nothing names a split count
        small = expect if n_splits else ("dense", False, None)
    rank_sharded(name, cat, k, n_splits, expect, small)


# ================================================================================ the dense route (validation shape)
@pytest.mark.parametrize("ways", [2, 3, 8])
def test_dense_route_validation_shape_sharded(ways, monkeypatch):
    """6 040 users x 3 706 items (the reference's ML-1M split), fp32 d=64: every shard takes the dense route (score block +
    wave-per-user ranking, bitmap and rated lists by global id).  2 and 3 ways by ``shard_bounds``; 8 ways on off-grid cuts
    with a 7-item shard, a fully masked shard and a user whose unmasked catalogue is smaller than k."""
    _env(monkeypatch, {})
    n_items = 3706
    if ways == 8:
        cuts = _off_grid_cuts(n_items, 7, residues=(1, 16, 31, 17), tiny_after=4)
        masked = 2
    else:
        cuts = [shard_bounds(n_items, ways, r)[0] for r in range(ways)] + [n_items]
        masked = None
    cat = Catalogue(60 + ways, 6040, n_items, 64, cuts, masked_shard=masked, thin_user=ways == 8)
    _, (ms, mi) = rank_sharded(f"dense-{ways}", cat, 20, 0, ("dense", False, None), ("dense", False, None))
    if ways == 8:                                                 # the thin user's list is mostly masked entries
        assert int((ms[cat.thin] == -1e9).sum()) >= 15 and int((mi[cat.thin] == PAD).sum()) == 0


# ================================================================================ the real shard shape
def test_real_shard_shape_default_dispatcher_8_ranks():
    """131 072 users x 10 M items fp32 d=128 (the S-EVAL table, 5 GB), 8 ranks by ``shard_bounds`` (bases 16 mod 32 on odd
    ranks), no switches: every 1.25 M-item shard must take the seeded flag-form DMA kernel (a dense 4 096-item prefix, then the
    kernel at item_base = lo + 4 096), and the merge must equal the one-launch ranking of the whole table for every user;
    every shard against the oracle on sampled users."""
    for v in SWITCHES:
        assert v not in os.environ
    dev = _dev()
    n_q, n_items, d, k, world = 131072, 10_000_000, 128, 20, 8
    cuts = [shard_bounds(n_items, world, r)[0] for r in range(world)] + [n_items]
    assert [c % 32 for c in cuts[1:-1]] == [16, 0, 16, 0, 16, 0, 16]
    cat = Catalogue(808, n_q, n_items, d, cuts, mean_rated=5)
    assert cat.tV.numel() * 4 > 5e9
    for r in range(world):
        key, info = _route(cat, cuts[r], cuts[r + 1], k, 0)
        assert key == ("fused-dma", True, "flags") and info["prefix_items"] == 4096, info
    rank_sharded("real-shape", cat, k, 0, ("fused-dma", True, "flags"), seed=808, edge_users=1)


# ================================================================================ merge edges
def _lists(n_lists, n_users, k_in, seed, dev):
    """Canonical (score desc, id asc) lists: real entries on a coarse grid (ties between lists), then -1e9 masked entries,
    then (-inf, INT32_MAX) padding; ids distinct within a user.  Some lists are all padding, some users all masked."""
    g = torch.Generator(device=dev).manual_seed(seed)
    shp = (n_lists, n_users, k_in)
    s = torch.randint(-6, 7, shp, generator=g, device=dev).float() / 4
    t = torch.arange(k_in, device=dev).view(1, 1, -1)
    ids = (torch.arange(n_lists, device=dev).view(-1, 1, 1) * 256 + t +
           (torch.arange(n_users, device=dev).view(1, -1, 1) % 1000) * 16384).to(torch.int32)
    n_real = torch.randint(0, k_in + 1, shp[:2], generator=g, device=dev)
    n_mask = (torch.rand(shp[:2], generator=g, device=dev) * (k_in - n_real + 1).float()).long()
    u = torch.arange(n_users, device=dev).view(1, -1)
    l = torch.arange(n_lists, device=dev).view(-1, 1)
    n_real = torch.where(u % 97 == 0, torch.zeros_like(n_real), n_real)                         # users with masked entries only
    empty = (u % 5 == 0) & (l % 7 == 3)                                                          # lists of padding only
    n_real, n_mask = torch.where(empty, 0, n_real), torch.where(empty, 0, n_mask)
    n_real, n_mask = n_real.unsqueeze(-1), n_mask.unsqueeze(-1)
    s = torch.where(t < n_real, s, torch.where(t < n_real + n_mask, torch.tensor(-1e9, device=dev), torch.tensor(float("-inf"), device=dev)))
    ids = torch.where(t < n_real + n_mask, ids, torch.tensor(PAD, dtype=torch.int32, device=dev))
    o = torch.argsort(ids, dim=-1, stable=True)
    s, ids = torch.gather(s, -1, o), torch.gather(ids, -1, o)
    o = torch.argsort(s, dim=-1, descending=True, stable=True)
    return torch.gather(s, -1, o).contiguous(), torch.gather(ids, -1, o).contiguous()


@pytest.mark.parametrize("n_lists,k_in,n_users,k_outs", [
    (64, 128, 16384 + 77, (128, 20, 1)),     # the LDS limit: 64 KiB per user, two waves per block; 8 192 blocks cover 16 384 users
    (8, 20, 32768 + 4 * 99, (20, 7, 1)),     # four waves per block: past 32 768 users the grid-stride loop runs
    (33, 50, 1000, (50, 1)),
])
def test_merge_topk_edges_against_oracle(n_lists, k_in, n_users, k_outs):
    """``crh_merge_topk`` at its limit of 64 lists x k = 128 and beyond the 8 192-block grid cap, k_out < k_in and k_out = 1,
    on padded lists and -1e9 entries in several lists (ids distinct), against the oracle's merge bit for bit."""
    dev = _dev()
    s, i = _lists(n_lists, n_users, k_in, n_lists * 1000 + k_in, dev)
    sel = np.unique(np.concatenate([np.arange(0, 300), np.arange(n_users - 300, n_users),
                                    np.random.default_rng(1).integers(0, n_users, 300)]))
    hs, hi = s[:, sel].cpu().numpy(), i[:, sel].cpu().numpy()
    for k_out in k_outs:
        ms, mi = ops.merge_topk(s, i, k_out)
        torch.cuda.synchronize()
        ws, wi = orc.merge_topk(hs, hi, k_out)
        gs, gi = ms.cpu().numpy()[sel], mi.cpu().numpy()[sel]
        assert np.array_equal(gi, wi), (n_lists, k_in, k_out, sel[np.where((gi != wi).any(1))[0][:8]])
        assert np.array_equal(gs.view(np.uint32), ws.view(np.uint32))
        # every user was written (the grid-stride loop reached the last users too): a user's first entry is its best real one
        best = torch.where(i == PAD, torch.tensor(float("-inf"), device=dev), s).amax(dim=(0, 2))
        assert torch.equal(ms[:, 0], best)


@pytest.mark.parametrize("n_lists,k_in,k_out,what", [(65, 20, 20, "n_lists=65"), (2, 129, 20, "k_in=129"),
                                                      (2, 20, 129, "k_out=129")])
def test_merge_topk_refuses_beyond_its_limits(n_lists, k_in, k_out, what):
    """65 lists or k = 129: a named error from crh_merge_topk, no launch."""
    dev = _dev()
    s = torch.zeros((n_lists, 4, k_in), device=dev)
    i = torch.zeros((n_lists, 4, k_in), dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError, match="crh_merge_topk") as e:
        ops.merge_topk(s, i, k_out)
    assert what in str(e.value)
    torch.cuda.synchronize()


# ================================================================================ the shard fuzzer, in the suite
def test_shard_fuzzer_short_run():
    """Half a minute of tests/fuzz/fuzz_score_topk.py --shards: random worlds of 2 .. 8 ranks, ``shard_bounds`` or random
    off-grid cuts, random widths / k / masks / route switches; merged == unsharded bitwise and every shard against the oracle."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "fuzz", "fuzz_score_topk.py"), "--shards", "--minutes", "0.5",
                          "--seed", "31"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fuzz ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
