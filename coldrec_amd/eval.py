"""Full-catalogue evaluation over a row-sharded item table.

GPU g owns item rows [g*I/G, (g+1)*I/G); the user table, the rated CSR and the candidate bitmap
are replicated.  Each rank runs the fused scoring/top-k kernel over its shard (global ids via
``item_base``), then ONE all-gather of the packed per-shard top-k (k scores + k ids per user,
8*k bytes) and the canonical merge -- so the result is independent of G.  With G == 1 there is
no collective at all.
"""
from __future__ import annotations

import os
from typing import Tuple

import torch

from . import ops


def shard_bounds(n_items: int, world: int, rank: int) -> Tuple[int, int]:
    """Contiguous row range of ``rank`` (same rule everywhere: bench, trainer, tests)."""
    return rank * n_items // world, (rank + 1) * n_items // world


class _PreparedShard:
    """The engines' lazily built ``ops.PreparedItems`` of their item table (see ``ShardedTopK`` for the contract)."""

    def _prepared(self, n_users: int, cand_bitmap, item_base: int, n_splits: int = 0):
        items = self.items
        if not items.is_cuda or items.dtype != torch.float32 or items.dim() != 2 or items.shape[1] != 128 or not items.is_contiguous():
            return None
        if cand_bitmap is not None and not cand_bitmap.is_contiguous():
            return None
        if not ops.score_topk_route(n_users, items.shape[0], 128, self.k, has_bitmap=cand_bitmap is not None,
                                    n_splits=n_splits)["screened"]:
            return None
        prep = getattr(self, "_prep", None)
        if prep is None or not prep.fits(items, cand_bitmap, item_base):
            self._prep = prep = None          # (frees the old buffer before the new one is allocated)
            try:
                self._prep = prep = ops.prepare_items(items, cand_bitmap, item_base)
            except torch.cuda.OutOfMemoryError:
                return None                   # no room for the copy: every call builds its own, as without the state
        return prep

    def refresh(self) -> None:
        """Drop the prepared item state: the next screened ``topk`` call builds a new one.  Needed after the table or the bitmap
        was written through raw pointers (the library's optimiser kernels), which no ``_version`` counter sees."""
        self._prep = None


class UserShardedTopK(_PreparedShard):
    """The zero-exchange alternative of SURVEY.md 8(e): the item table is REPLICATED (5.1 GB at S-EVAL) and the
    user block is cut across the ranks; every rank ranks its users against the whole catalogue and one
    all-gather puts the (k scores, k ids) rows back in user order.  No merge, no dependence on G by construction;
    used as the validation mode of the item-sharded path and when the catalogue fits every GPU.

    Calls that take the screened route share one prepared item state, under the contract ``ShardedTopK`` states."""

    def __init__(self, items: torch.Tensor, k: int, world: int = 1, rank: int = 0, group=None):
        self.items, self.k = items, int(k)
        self.world, self.rank, self.group = world, rank, group

    def topk(self, user_emb, users, rated_rowptr=None, rated_col=None, cand_bitmap=None):
        """``users`` must be given (int32 rows of user_emb for the whole block, identical on every rank)."""
        n = users.shape[0]
        lo, hi = self.rank * n // self.world, (self.rank + 1) * n // self.world
        rp = rc = None
        if rated_rowptr is not None:
            rp = (rated_rowptr[lo:hi + 1] - rated_rowptr[lo]).contiguous()
            rc = rated_col[int(rated_rowptr[lo]):int(rated_rowptr[hi])].contiguous()
        prep = self._prepared(hi - lo, cand_bitmap, 0)
        s, i = ops.score_topk(user_emb, users[lo:hi].contiguous(), self.items, self.k, rp, rc, cand_bitmap,
                              **({} if prep is None else {"prepared": prep}))
        if self.world == 1:
            return s, i
        import torch.distributed as dist
        # slices differ by at most one user: pad to the longest, gather, cut the padding away
        longest = (n + self.world - 1) // self.world
        packed = torch.zeros((longest, 2 * self.k), dtype=torch.int32, device=s.device)
        packed[: hi - lo] = torch.cat([s.view(torch.int32), i], dim=1)
        flat = torch.empty((self.world * longest, 2 * self.k), dtype=torch.int32, device=s.device)
        dist.all_gather_into_tensor(flat, packed, group=self.group)
        rows = [flat[r * longest: r * longest + ((r + 1) * n // self.world - r * n // self.world)]
                for r in range(self.world)]
        full = torch.cat(rows, 0)
        return full[:, : self.k].contiguous().view(torch.float32), full[:, self.k:].contiguous()


class ShardedTopK(_PreparedShard):
    """One rank's item shard ranked per user block, the shards' lists gathered and merged canonically.

    PREPARED ITEMS.  When a call takes the screened route (``ops.score_topk_route(...)["screened"]``) the engine builds the item
    half of that route's stage 0 once (``ops.prepare_items``: the packed fp16 copy of the shard, the live-row map under the
    bitmap, the maxima of the certificate's bound) and every later call reuses it, as long as the bitmap is the same tensor,
    neither tensor's ``_version`` has moved and the stream is the same; otherwise it builds a new one.  The contract that comes
    with it: the shard and the bitmap must not be changed behind the engine's back while it lives.  In-place torch edits are
    caught through ``_version``.  Writes through raw pointers are not -- the library's own optimiser kernels write that way --
    and need ``refresh()`` before the next call.  This matters for soundness, not only for speed: the certificate's R, N, N^
    come from the prepared copy, so a stale copy could certify a wrong list.  ``BaseRecommender`` builds its engine per
    evaluation, after training has stopped writing."""

    def __init__(self, item_shard: torch.Tensor, item_base: int, n_items_global: int, k: int,
                 world: int = 1, rank: int = 0, group=None):
        self.items = item_shard
        self.item_base = int(item_base)
        self.n_items_global = int(n_items_global)
        self.k = int(k)
        self.world, self.rank, self.group = world, rank, group
        # test hook: run the all-gather + merge even with one rank (exercises the RCCL path on a 1-GPU box)
        self.force_collective = bool(int(os.environ.get("CRH_FORCE_COLLECTIVE", "0")))

    def topk(self, user_emb, users, rated_rowptr=None, rated_col=None, cand_bitmap=None, n_splits: int = 0,
             kernel_events=None):
        kw = {}
        if kernel_events is not None:
            kw["kernel_events"] = kernel_events
        if n_splits:
            kw["n_splits"] = n_splits
        prep = self._prepared(user_emb.shape[0] if users is None else users.shape[0], cand_bitmap, self.item_base, n_splits)
        if prep is not None:
            kw["prepared"] = prep
        s, i = ops.score_topk(user_emb, users, self.items, self.k, rated_rowptr, rated_col, cand_bitmap,
                              item_base=self.item_base, **kw)
        if self.world == 1 and not self.force_collective:
            return s, i
        import torch.distributed as dist
        packed = torch.cat([s.view(torch.int32), i], dim=1).contiguous()          # (Bu, 2k) int32
        flat = torch.empty((self.world * packed.shape[0], packed.shape[1]), dtype=torch.int32,
                           device=packed.device)                                   # rank-major concatenation
        dist.all_gather_into_tensor(flat, packed, group=self.group)
        gathered = flat.view(self.world, packed.shape[0], packed.shape[1])
        gs = gathered[:, :, :self.k].contiguous().view(torch.float32)
        gi = gathered[:, :, self.k:].contiguous()
        return ops.merge_topk(gs, gi, self.k)
