"""Torch-tensor front ends of the C ABI (include/coldrec_hip.h).  Device memory and streams
come from PyTorch-ROCm; all arithmetic happens in libcoldrec_hip.so.  No CPU fallback."""
from __future__ import annotations

import ctypes
import weakref
import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

SUPPORTED_DIMS = (8, 16, 32, 64, 128, 256)
SUPPORTED_DIMS_F16 = (16, 32, 64, 128, 256)


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("coldrec_amd ops need tensors on the MI355X (cuda device); there is no CPU path")


def pad_dim(table: torch.Tensor) -> torch.Tensor:
    """Zero-pad the embedding width to the next width the MFMA kernel is built for.
    Trailing zeros are exact no-ops of the fp32 fma chain (fma(0,0,s) == s, s never -0)."""
    d = table.shape[1]
    dims = SUPPORTED_DIMS_F16 if table.dtype == torch.float16 else SUPPORTED_DIMS
    if d in dims:
        return table
    for w in dims:
        if w > d:
            out = torch.zeros((table.shape[0], w), dtype=table.dtype, device=table.device)
            out[:, :d] = table
            return out
    raise RuntimeError(f"embedding width {d} > 256 is not supported by score_topk")


def make_bitmap(n_items_global: int, masked_ids, device) -> Optional[torch.Tensor]:
    """uint32 words (stored as int32), bit (gi & 31) of word gi >> 5 set => item gi is masked."""
    if masked_ids is None or len(masked_ids) == 0:
        return None
    words = np.zeros((n_items_global + 31) // 32 + 1, dtype=np.uint32)
    ids = np.asarray(masked_ids, dtype=np.int64)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).to(device)


def rated_csr(rated_lists, device) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """Per-slot ascending int32 global item ids + int64 row offsets from a list of id arrays."""
    lens = np.fromiter((0 if r is None else len(r) for r in rated_lists), dtype=np.int64,
                       count=len(rated_lists))
    if lens.sum() == 0:
        return None, None
    rowptr = np.zeros(len(rated_lists) + 1, np.int64)
    np.cumsum(lens, out=rowptr[1:])
    col = np.empty(int(rowptr[-1]), np.int32)
    for r, ids in enumerate(rated_lists):
        if lens[r]:
            col[rowptr[r]:rowptr[r + 1]] = np.sort(np.asarray(ids, dtype=np.int64))
    return torch.from_numpy(rowptr).to(device), torch.from_numpy(col).to(device)


_ws_cache = {}


def _workspace(nbytes: int, device) -> torch.Tensor:
    """Grow-only scratch, ONE PER (device, stream): calls on different streams never alias, and calls on one stream
    are ordered by it.  Only the eager ops (scoring, dense ranking) use it; everything that may be captured into a
    hipGraph (the engines' BPR steps) owns a private buffer (``bpr_workspace``), because a captured graph keeps the raw
    pointer and a regrown shared buffer would hand that memory back to the caching allocator."""
    key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def _score_ws_bytes(n_users: int, n_items: int, d: int, k: int, half: bool = False, pack: bool = True) -> int:
    """Bytes of the workspace ``score_topk`` passes for a block of this shape (``d`` a width the library supports)."""
    L = _lib.lib()
    if not pack:
        return L.crh_score_topk_min_workspace_bytes(n_users, k)
    return (L.crh_score_topk_f16_workspace_bytes if half else L.crh_score_topk_workspace_bytes)(n_users, n_items, d, k)


def score_topk(user_emb: torch.Tensor, users: Optional[torch.Tensor], item_emb: torch.Tensor, k: int,
               rated_rowptr: Optional[torch.Tensor] = None, rated_col: Optional[torch.Tensor] = None,
               cand_bitmap: Optional[torch.Tensor] = None, item_base: int = 0, n_splits: int = 0,
               out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, kernel_events=None, pack: bool = True,
               prepared: Optional["PreparedItems"] = None):
    """Fused ``user_emb[users] @ item_emb.T`` -> masks -> top-k (model/MF.py:58-63 +
    model/BaseRecommender.py:175-182).  Returns (scores fp32, global item ids int32), each
    (n_users, k), canonical order.  fp32 tables: exact fp32 MFMA, bit-identical to the oracle's fma chain;
    fp16 tables (both): fp16 MFMA with fp32 accumulation (config 5, generated embeddings).  ``users`` int32 rows of user_emb or None for all rows.
    ``kernel_events``: optional (hipEvent_t, hipEvent_t) raw handles recorded around the scoring
    kernel alone (bench.py's roofline measurement).  ``pack=False`` withholds the workspace for the
    fragment-ordered copy of the item shard (row-major kernel: same results, less memory, ~0.9x speed).
    ``prepared``: a ``PreparedItems`` of ``prepare_items`` for this table, bitmap and base; a call that takes the screened route
    then skips the item half of its stage 0.  A state that does not fit the call is ignored: same results, nothing saved."""
    _need_cuda(user_emb, users, item_emb, rated_rowptr, rated_col, cand_bitmap)
    if user_emb.dtype != item_emb.dtype or user_emb.dtype not in (torch.float32, torch.float16):
        raise RuntimeError("score_topk: both tables fp32 (exact, canonical) or both fp16 (fp32 accumulate)")
    half = user_emb.dtype == torch.float16
    if user_emb.shape[1] != item_emb.shape[1]:
        raise RuntimeError("score_topk: user/item embedding widths differ")
    user_emb, item_emb = pad_dim(user_emb.contiguous()), pad_dim(item_emb.contiguous())
    if users is not None:
        users = users.to(torch.int32).contiguous()
    n_users = user_emb.shape[0] if users is None else users.shape[0]
    n_items, d = item_emb.shape
    if rated_rowptr is not None:
        assert rated_rowptr.dtype == torch.int64 and rated_col.dtype == torch.int32
        assert rated_rowptr.shape[0] == n_users + 1
    if cand_bitmap is not None:
        assert cand_bitmap.dtype == torch.int32
    dev = user_emb.device
    if out is None:
        out = (torch.empty((n_users, k), dtype=torch.float32, device=dev),
               torch.empty((n_users, k), dtype=torch.int32, device=dev))
    L = _lib.lib()
    ws_bytes = _score_ws_bytes(n_users, n_items, d, k, half, pack)
    ws = _workspace(ws_bytes, dev)
    args = (_lib.ptr(user_emb), _lib.ptr(users), n_users, _lib.ptr(item_emb), n_items, d,
            _lib.ptr(rated_rowptr), _lib.ptr(rated_col), _lib.ptr(cand_bitmap), k,
            item_base, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(ws), ws_bytes,
            _lib.current_stream(), n_splits,
            kernel_events[0] if kernel_events else None,
            kernel_events[1] if kernel_events else None)
    if prepared is not None and not half and pack and prepared.fits(item_emb, cand_bitmap, item_base):
        # (built at first use, for this call's plan; the library compares the rest and ignores a state of another plan)
        rc = L.crh_score_topk_f32_prepared(*args, prepared.handle_for(n_users, ws, ws_bytes))
    else:
        rc = (L.crh_score_topk_f16_ex if half else L.crh_score_topk_f32_ex)(*args)
    _lib.check(rc, "crh_score_topk_f32")
    return out


class PreparedItems:
    """The item half of the screened route's stage 0 (the packed fp16 copy of the shard, the live-row map under the candidate
    bitmap, the maxima of the certificate's bound), built ONCE and handed to every ``score_topk`` call of an evaluation
    (``prepared=``).  It owns a private device buffer -- never the shared scratch, which other ops overwrite -- and the native
    handle, freed on deletion.

    The native state is built at the first call that uses it, for that call's plan (user count and workspace decide whether the
    fp16 pass is compacted and ordered), or explicitly by ``build(n_users, k)``.  Calls of another plan ignore it.

    CONTRACT.  The state is a copy: the table and the bitmap must not change while it is in use.  In-place torch edits are seen
    through the tensors' ``_version`` (``fits`` then fails and the call rebuilds per call); writes through raw pointers -- the
    library's own optimiser kernels write that way -- are NOT seen: make a new ``PreparedItems`` after them.  This matters for
    soundness, not only for speed: the certificate's R, N, N^ are those of the prepared copy."""

    def __init__(self, item_emb: torch.Tensor, cand_bitmap: Optional[torch.Tensor] = None, item_base: int = 0):
        _need_cuda(item_emb, cand_bitmap)
        if item_emb.dtype != torch.float32 or item_emb.dim() != 2 or item_emb.shape[1] != 128 or not item_emb.is_contiguous():
            raise RuntimeError("prepare_items: the screened route ranks contiguous fp32 tables of width 128")
        if cand_bitmap is not None and (cand_bitmap.dtype != torch.int32 or not cand_bitmap.is_contiguous()):
            raise RuntimeError("prepare_items: cand_bitmap must be contiguous int32 words")
        self.item_emb, self.cand_bitmap, self.item_base = item_emb, cand_bitmap, int(item_base)
        self.item_ptr, self.item_version = item_emb.data_ptr(), item_emb._version
        self.bitmap_ptr = None if cand_bitmap is None else cand_bitmap.data_ptr()
        self.bitmap_version = None if cand_bitmap is None else cand_bitmap._version
        self.stream = torch.cuda.current_stream(item_emb.device).cuda_stream
        nbytes = int(_lib.lib().crh_score_screen_items_bytes(item_emb.shape[0], 0 if cand_bitmap is None else 1))
        self.buf = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=item_emb.device)
        self.handle = None

    def fits(self, item_emb: torch.Tensor, cand_bitmap: Optional[torch.Tensor], item_base: int = 0) -> bool:
        """Was this state made for exactly these tensors, unchanged since, on the current stream?"""
        if item_emb.data_ptr() != self.item_ptr or item_emb.shape != self.item_emb.shape or int(item_base) != self.item_base:
            return False
        if self.item_emb._version != self.item_version or item_emb._version != self.item_version:
            return False
        if (cand_bitmap is None) != (self.cand_bitmap is None):
            return False
        if cand_bitmap is not None and (cand_bitmap.data_ptr() != self.bitmap_ptr or cand_bitmap._version != self.bitmap_version
                                        or self.cand_bitmap._version != self.bitmap_version):
            return False
        return torch.cuda.current_stream(item_emb.device).cuda_stream == self.stream

    def handle_for(self, n_users: int, ws: torch.Tensor, ws_bytes: int):
        if self.handle is None:
            h = ctypes.c_void_p(None)
            rc = _lib.lib().crh_score_screen_items_prepare(self.item_ptr, self.item_emb.shape[0], 128, self.bitmap_ptr, self.item_base,
                                                           int(n_users), _lib.ptr(self.buf), self.buf.numel(), _lib.ptr(ws),
                                                           int(ws_bytes), self.stream, ctypes.byref(h))
            _lib.check(rc, "crh_score_screen_items_prepare")
            self.handle = h
        return self.handle

    def build(self, n_users: int, k: int) -> "PreparedItems":
        """Build the native state now, for ``score_topk`` calls of ``n_users`` users and this ``k`` on the current stream."""
        if torch.cuda.current_stream(self.item_emb.device).cuda_stream != self.stream:
            raise RuntimeError("PreparedItems.build: not the stream the state was made on")
        ws_bytes = _score_ws_bytes(int(n_users), self.item_emb.shape[0], 128, int(k))
        self.handle_for(n_users, _workspace(ws_bytes, self.item_emb.device), ws_bytes)
        return self

    def close(self) -> None:
        h, self.handle = self.handle, None
        if h is not None:
            _lib.lib().crh_score_screen_items_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def prepare_items(item_emb: torch.Tensor, cand_bitmap: Optional[torch.Tensor] = None, item_base: int = 0) -> PreparedItems:
    """A ``PreparedItems`` for ``score_topk(..., prepared=)``: see the class for what it holds and for its contract."""
    return PreparedItems(item_emb, cand_bitmap, item_base)


def screen_item_preps() -> int:
    """Runs of the item half of the screened route's stage 0 in this process, prepared or inside a call (a host counter)."""
    return int(_lib.lib().crh_score_topk_screen_item_preps())


ROUTE_NAMES = {1: "dense", 2: "fused-wave", 3: "fused-wg", 4: "fused-dma"}


def score_topk_route(n_users: int, n_items: int, d: int, k: int, half: bool = False, has_bitmap: bool = True,
                     n_splits: int = 0, pack: bool = True) -> dict:
    """Which kernels ``score_topk`` runs for a block of this shape: the library's own answer (crh_score_topk_route evaluates
    the dispatcher's predicates under the current environment switches; no GPU needed), with the workspace ``score_topk``
    would pass.  ``{"route", "seeded", "dma_form", "prefix_items", "n_splits", "kernel", "code", "screened"}``; ``kernel`` is the scoring
    kernel's name as rocprofv3 prints it; ``screened``: the call takes the screened route (fp16 screen, exact rescoring and
    certificate, exact fallback; crh_score_topk_screened), and route / kernel / code describe the exact route it replaces."""
    L = _lib.lib()
    d = d if d % 8 == 0 and (L.crh_score_topk_f16_supports_dim(d) if half else L.crh_score_topk_supports_dim(d)) else \
        next(w for w in (8, 16, 32, 64, 128, 256) if w >= d and (w >= 16 or not half))
    ws_bytes = _score_ws_bytes(n_users, n_items, d, k, half, pack)
    prefix, splits = ctypes.c_int64(0), ctypes.c_int(0)
    code = L.crh_score_topk_route(2 if half else 4, n_users, n_items, d, k, ws_bytes, 1 if has_bitmap else 0, n_splits,
                                  ctypes.byref(prefix), ctypes.byref(splits))
    _lib.check(code if code < 0 else 0, "crh_score_topk_route")
    screened = bool(L.crh_score_topk_screened(2 if half else 4, n_users, n_items, d, k, ws_bytes, 1 if has_bitmap else 0, n_splits))
    return {"route": ROUTE_NAMES[code & 15], "seeded": bool(code & 16), "dma_form": ("flags" if code & 32 else "barrier") if (code & 15) == 4 else None,
            "prefix_items": int(prefix.value),
            "n_splits": int(splits.value), "kernel": L.crh_score_topk_route_kernel(code).decode(), "code": int(code),
            "screened": screened}


def score_topk_screen_plan(n_users: int, n_items: int, d: int, k: int, has_bitmap: bool = True) -> dict:
    """The screened route's plan for a call ``score_topk_route`` reports as screened: ``{"cuts", "compact"}`` -- the item-range
    cuts of its fp16 pass, and whether that pass streams only the rows the candidate bitmap leaves (CRH_SCORE_SCREEN_COMPACT)."""
    cuts, compact = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(_lib.lib().crh_score_topk_screen_plan(n_users, n_items, _score_ws_bytes(n_users, n_items, d, k), 1 if has_bitmap else 0,
                                                     ctypes.byref(cuts), ctypes.byref(compact)), "crh_score_topk_screen_plan")
    return {"cuts": int(cuts.value), "compact": bool(compact.value)}


def score_topk_screen_ordered(n_users: int, n_items: int, d: int, k: int, has_bitmap: bool = True) -> bool:
    """Does a screened call of this shape stream the unmasked rows of its main range by descending norm (CRH_SCORE_SCREEN_ORDER)?
    True when the compaction is on, the fp16 pass is one cut and the workspace ``score_topk`` passes holds the sorted map."""
    return bool(_lib.lib().crh_score_topk_screen_ordered(n_users, n_items, _score_ws_bytes(n_users, n_items, d, k), 1 if has_bitmap else 0))


def score_topk_screen_map(cand_bitmap: torch.Tensor, item_emb: torch.Tensor, item_base: int = 0, prefix: int = 0,
                          ordered: bool = True):
    """Only the map construction of the screened route's stage 0 (a test entry point): ``(map, keys)``, int32 device tensors --
    the ids of the unmasked items of ``[item_base + prefix, item_base + n_items)`` in the order the fp16 pass streams them and
    the 16-bit norm keys of those rows."""
    _need_cuda(cand_bitmap, item_emb)
    assert cand_bitmap.dtype == torch.int32 and item_emb.dtype == torch.float32 and item_emb.shape[1] == 128
    item_emb = item_emb.contiguous()
    n_main = item_emb.shape[0] - prefix
    out_map = torch.empty(n_main, dtype=torch.int32, device=item_emb.device)
    out_keys = torch.empty(n_main, dtype=torch.int32, device=item_emb.device)
    count = ctypes.c_int64(0)
    rc = _lib.lib().crh_score_topk_screen_map(_lib.ptr(cand_bitmap), _lib.ptr(item_emb), item_emb.shape[0], item_base, prefix,
                                              1 if ordered else 0, _lib.ptr(out_map), _lib.ptr(out_keys), ctypes.byref(count),
                                              _lib.current_stream())
    _lib.check(rc, "crh_score_topk_screen_map")
    return out_map[:count.value], out_keys[:count.value]


def score_topk_screen_rated_tiles(n_users: int, n_items: int, d: int, k: int, has_bitmap: bool = True, has_rated: bool = True) -> bool:
    """Does a screened call of this shape gate the rated-list lookups of its fp16 pass by per-tile flags
    (CRH_SCORE_SCREEN_RATED_TILES)?  True when the compaction is on, the call has rated lists and the workspace ``score_topk``
    passes holds the flags and the inverse map."""
    return bool(_lib.lib().crh_score_topk_screen_rated_tiles(n_users, n_items, _score_ws_bytes(n_users, n_items, d, k),
                                                             1 if has_bitmap else 0, 1 if has_rated else 0))


def score_topk_screen_flags(cand_bitmap: torch.Tensor, item_emb: torch.Tensor, rated_rowptr: torch.Tensor, rated_col: torch.Tensor,
                            item_base: int = 0, prefix: int = 0, ordered: bool = True) -> torch.Tensor:
    """Only the rated-tile flags of the screened route (a test entry point): int32 device words ``[workgroups, blocks * 64]`` over
    the map ``score_topk_screen_map`` returns for the same arguments -- tile ``t`` of the stream in word ``t >> 3``, nibble
    ``4 * (t & 7)`` of its workgroup's row, bit ``w`` set iff a slot of wave ``w`` (128 slots) rated an item of the tile."""
    _need_cuda(cand_bitmap, item_emb, rated_rowptr, rated_col)
    assert cand_bitmap.dtype == torch.int32 and item_emb.dtype == torch.float32 and item_emb.shape[1] == 128
    assert rated_rowptr.dtype == torch.int64 and rated_col.dtype == torch.int32
    item_emb = item_emb.contiguous()
    n_users, n_main = rated_rowptr.shape[0] - 1, item_emb.shape[0] - prefix
    L = _lib.lib()
    groups = ((n_users + 127) // 128 + 3) // 4
    words = int(L.crh_score_topk_screen_flags_bytes(n_users, n_main)) // 4
    out = torch.empty((groups, words // groups), dtype=torch.int32, device=item_emb.device)
    rc = L.crh_score_topk_screen_flags(_lib.ptr(cand_bitmap), _lib.ptr(item_emb), item_emb.shape[0], item_base, prefix,
                                       1 if ordered else 0, _lib.ptr(rated_rowptr), _lib.ptr(rated_col), n_users, _lib.ptr(out),
                                       _lib.current_stream())
    _lib.check(rc, "crh_score_topk_screen_flags")
    return out


def score_topk_uncertified(device=None) -> int:
    """Users the last screened ``score_topk`` call on this device and stream could not certify (they took the exact fallback).
    Synchronises the stream; only meaningful right after a call that ``score_topk_route(...)["screened"]`` reports."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    key = (dev.type, dev.index, torch.cuda.current_stream(dev).cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None:
        raise RuntimeError("score_topk_uncertified: no scoring workspace on this stream")
    n = _lib.lib().crh_score_topk_uncertified(_lib.ptr(buf), _lib.current_stream())
    _lib.check(n if n < 0 else 0, "crh_score_topk_uncertified")
    return int(n)


def mask_topk(scores: torch.Tensor, k: int, rated_rowptr=None, rated_col=None, cand_bitmap=None,
              item_base: int = 0, write_back: bool = True):
    """Masks + top-k over a dense (n_users, n_items) fp32 block (model/BaseRecommender.py:175-183)."""
    _need_cuda(scores, rated_rowptr, rated_col, cand_bitmap)
    assert scores.dtype == torch.float32 and scores.dim() == 2 and scores.stride(1) == 1
    n_users, n_items = scores.shape
    dev = scores.device
    out = (torch.empty((n_users, k), dtype=torch.float32, device=dev),
           torch.empty((n_users, k), dtype=torch.int32, device=dev))
    rc = _lib.lib().crh_mask_topk_f32(_lib.ptr(scores), n_users, n_items, scores.stride(0),
                                      _lib.ptr(rated_rowptr), _lib.ptr(rated_col), _lib.ptr(cand_bitmap), k,
                                      item_base, 1 if write_back else 0, _lib.ptr(out[0]), _lib.ptr(out[1]),
                                      _lib.current_stream())
    _lib.check(rc, "crh_mask_topk_f32")
    return out


def merge_topk(scores: torch.Tensor, idx: torch.Tensor, k_out: int):
    """Canonical merge of (n_lists, n_users, k_in) partial lists -> (n_users, k_out)."""
    _need_cuda(scores, idx)
    assert scores.dtype == torch.float32 and idx.dtype == torch.int32
    scores, idx = scores.contiguous(), idx.contiguous()
    n_lists, n_users, k_in = scores.shape
    dev = scores.device
    out = (torch.empty((n_users, k_out), dtype=torch.float32, device=dev),
           torch.empty((n_users, k_out), dtype=torch.int32, device=dev))
    rc = _lib.lib().crh_merge_topk(_lib.ptr(scores), _lib.ptr(idx), n_lists, n_users, k_in, k_out,
                                   _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.current_stream())
    _lib.check(rc, "crh_merge_topk")
    return out


_warmed = set()


def warm_up(device) -> None:
    """Load the library's device code on ``device`` with one tiny launch per source file of the .so (HIP loads a code
    object lazily, at the first launch of any kernel in it: ~0.3 s for this library, which would otherwise land in a
    trainer's first epoch -- where the reference's own timer would count it, main.py:203-205).  The trainers call this
    when they are constructed, like the reference moves its model to the device before its timer starts
    (model/MF.py:13-16).  Idempotent per device; nothing is computed that anyone reads."""
    device = torch.device(device)
    if device.type != 'cuda' or (device.index, ) in _warmed:
        return
    _warmed.add((device.index, ))
    with torch.cuda.device(device):
        f32 = dict(dtype=torch.float32, device=device)
        u, v = torch.zeros((64, 8), **f32), torch.zeros((96, 8), **f32)
        score_topk(u, None, v, 4)                                            # score_topk.hip (+ merge: n_splits)
        score_topk(u, None, v, 4, n_splits=2)                                # merge_topk.hip
        mask_topk(torch.zeros((4, 64), **f32), 4, write_back=False)
        idx = torch.zeros(4, dtype=torch.int32, device=device)
        g, gv = torch.zeros_like(u), torch.zeros_like(v)
        bpr_fwd_bwd(u, v, v, idx, idx, idx, 0.0, g, gv, gv, plan=build_plans_device(idx, idx, idx, 4)[0])   # bpr_plan.hip, bpr.hip
        adam_dense(u.clone(), g, torch.zeros_like(u), torch.zeros_like(u), 1)  # optim.hip
        l2_norm(u)                                                           # l2_reg.hip
        rp = torch.arange(0, 65, dtype=torch.int64, device=device).clamp_(max=1)
        spmm_csr(rp, torch.zeros(1, dtype=torch.int32, device=device), torch.ones(1, **f32), u, y=torch.empty_like(u))
        # ... and the handful of ATen kernels the trainers' epoch loop touches (PyTorch loads its code lazily too): the
        # membership gather of the validation metrics, the loss read-back, the epoch upload
        dense = torch.zeros((4, 8), dtype=torch.bool, device=device)
        ids = torch.zeros((4, 3), dtype=torch.int32, device=device).long()
        ok = (ids >= 0) & (ids < 8)
        (dense[torch.arange(4, device=device).unsqueeze(1), ids.clamp(0, 7)] & ok).cpu()
        torch.zeros((3, 2), **f32).sum(dim=1).cpu()
        torch.empty(4, dtype=torch.int32, device=device).copy_(torch.zeros(4, dtype=torch.int32).pin_memory(), non_blocking=True)
        torch.cuda.synchronize(device)


# ------------------------------------------------------------------------------ training ops
def bpr_fwd_bwd(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx, reg: float,
                grad_user=None, grad_pos=None, grad_neg=None, loss_out: Optional[torch.Tensor] = None,
                plan: Optional[torch.Tensor] = None, workspace: Optional[torch.Tensor] = None):
    """bpr_loss + l2_reg_loss and their dense table gradients for one batch of triples
    (util/utils.py:25-29,44-48 + autograd at model/MF.py:22-26).  ``*_idx`` int32 device tensors or
    None (tables are already gathered).  Gradients are ACCUMULATED into ``grad_*`` (all three or
    none).  Returns ``loss_out`` = device tensor [bpr, l2]."""
    _need_cuda(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx, grad_user, grad_pos, grad_neg)
    d = user_table.shape[1]
    batch = user_idx.shape[0] if user_idx is not None else user_table.shape[0]
    for t in (user_table, pos_table, neg_table):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == d
    for ix in (user_idx, pos_idx, neg_idx):
        assert ix is None or (ix.dtype == torch.int32 and ix.is_contiguous() and ix.shape[0] == batch)
    dev = user_table.device
    if loss_out is None:
        loss_out = torch.empty(2, dtype=torch.float32, device=dev)
    L = _lib.lib()
    need = L.crh_bpr_workspace_bytes(batch)
    ws = workspace if workspace is not None else _workspace(need, dev)
    assert ws.numel() >= need, "bpr_fwd_bwd: private workspace too small for this batch"
    rc = L.crh_bpr_fwd_bwd_f32(_lib.ptr(user_table), _lib.ptr(pos_table), _lib.ptr(neg_table), d,
                               _lib.ptr(user_idx), _lib.ptr(pos_idx), _lib.ptr(neg_idx), batch, float(reg),
                               _lib.ptr(grad_user), _lib.ptr(grad_pos), _lib.ptr(grad_neg), _lib.ptr(loss_out),
                               _lib.ptr(plan), _lib.ptr(ws), ws.numel(), _lib.current_stream())
    _lib.check(rc, "crh_bpr_fwd_bwd_f32")
    return loss_out


def _bpr_checks(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx):
    d = user_table.shape[1]
    batch = user_idx.shape[0] if user_idx is not None else user_table.shape[0]
    for t in (user_table, pos_table, neg_table):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[1] == d
    for ix in (user_idx, pos_idx, neg_idx):
        assert ix is None or (ix.dtype == torch.int32 and ix.is_contiguous() and ix.shape[0] == batch)
    return d, batch


def bpr_fwd(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx, sums_out: torch.Tensor,
            workspace: torch.Tensor):
    """Forward of one rank's slice of the batch (data-parallel split): ``sums_out`` (4 floats, device)
    = [sum u^2, sum p^2, sum n^2, sum -log(1e-5+sigmoid(x))] of the slice.  ``workspace``: uint8 tensor of
    ``bpr_workspace_bytes(batch)`` that must be handed to ``bpr_bwd`` unchanged."""
    _need_cuda(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx, sums_out, workspace)
    d, batch = _bpr_checks(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx)
    assert sums_out.dtype == torch.float32 and sums_out.numel() >= 4
    rc = _lib.lib().crh_bpr_fwd_f32(_lib.ptr(user_table), _lib.ptr(pos_table), _lib.ptr(neg_table), d,
                                    _lib.ptr(user_idx), _lib.ptr(pos_idx), _lib.ptr(neg_idx), batch,
                                    _lib.ptr(sums_out), _lib.ptr(workspace), workspace.numel(),
                                    _lib.current_stream())
    _lib.check(rc, "crh_bpr_fwd_f32")
    return sums_out


def bpr_bwd(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx, global_batch: int, reg: float,
            sums: torch.Tensor, grad_user, grad_pos, grad_neg, loss_out: Optional[torch.Tensor],
            workspace: torch.Tensor, plan: Optional[torch.Tensor] = None):
    """Backward of one rank's slice with the all-reduced ``sums`` and the global batch size."""
    _need_cuda(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx, sums, grad_user, grad_pos, grad_neg,
               workspace)
    d, batch = _bpr_checks(user_table, pos_table, neg_table, user_idx, pos_idx, neg_idx)
    rc = _lib.lib().crh_bpr_bwd_f32(_lib.ptr(user_table), _lib.ptr(pos_table), _lib.ptr(neg_table), d,
                                    _lib.ptr(user_idx), _lib.ptr(pos_idx), _lib.ptr(neg_idx), batch,
                                    int(global_batch), float(reg), _lib.ptr(sums), _lib.ptr(grad_user),
                                    _lib.ptr(grad_pos), _lib.ptr(grad_neg), _lib.ptr(loss_out), _lib.ptr(plan),
                                    _lib.ptr(workspace), workspace.numel(), _lib.current_stream())
    _lib.check(rc, "crh_bpr_bwd_f32")
    return loss_out


def bpr_bwd_owned(user_table, item_table, user_idx, pos_idx, neg_idx, reg: float, sums: torch.Tensor, grad_user, grad_item,
                  loss_out: Optional[torch.Tensor], workspace: torch.Tensor, plan: torch.Tensor, own_mod: int, own_rem: int):
    """Deterministic backward over the plan's row slots ``w % own_mod == own_rem`` only (crh_bpr_bwd_owned_f32): the
    row-ownership split of the data-parallel touched-rows step; ``workspace`` carries a forward over the WHOLE batch."""
    _need_cuda(user_table, item_table, user_idx, pos_idx, neg_idx, sums, grad_user, grad_item, workspace, plan)
    d, batch = _bpr_checks(user_table, item_table, item_table, user_idx, pos_idx, neg_idx)
    rc = _lib.lib().crh_bpr_bwd_owned_f32(_lib.ptr(user_table), _lib.ptr(item_table), d, _lib.ptr(user_idx), _lib.ptr(pos_idx),
                                          _lib.ptr(neg_idx), batch, float(reg), _lib.ptr(sums), _lib.ptr(grad_user),
                                          _lib.ptr(grad_item), _lib.ptr(loss_out), _lib.ptr(plan), int(own_mod), int(own_rem),
                                          _lib.ptr(workspace), workspace.numel(), _lib.current_stream())
    _lib.check(rc, "crh_bpr_bwd_owned_f32")
    return loss_out


def rows_pack_cap(batch: int, own_mod: int) -> int:
    return int(_lib.lib().crh_rows_pack_cap(int(batch), int(own_mod)))


def rows_pack(table, plan, batch: int, user_rows: int, own_mod: int, own_rem: int, out_ids, out_rows) -> None:
    """(row id, row) of every plan slot this rank owns, from ``table`` (crh_rows_pack_f32); ids past the plan's rows are -1."""
    _need_cuda(table, plan, out_ids, out_rows)
    assert out_ids.dtype == torch.int32 and out_rows.dtype == torch.float32 and out_rows.is_contiguous() and table.is_contiguous()
    assert out_ids.numel() >= rows_pack_cap(batch, own_mod) and out_rows.shape[0] >= out_ids.numel()
    _lib.check(_lib.lib().crh_rows_pack_f32(_lib.ptr(table), _lib.ptr(plan), int(batch), int(user_rows), table.shape[1],
                                            int(own_mod), int(own_rem), _lib.ptr(out_ids), _lib.ptr(out_rows),
                                            _lib.current_stream()), "crh_rows_pack_f32")


def rows_unpack(table, ids, rows) -> None:
    """table[ids[e]] = rows[e] for ids[e] >= 0 (crh_rows_unpack_f32)."""
    _need_cuda(table, ids, rows)
    assert ids.dtype == torch.int32 and rows.dtype == torch.float32 and rows.is_contiguous() and ids.is_contiguous()
    _lib.check(_lib.lib().crh_rows_unpack_f32(_lib.ptr(table), _lib.ptr(ids), _lib.ptr(rows), ids.numel(), table.shape[1],
                                              _lib.current_stream()), "crh_rows_unpack_f32")


def bpr_workspace(batch: int, device) -> torch.Tensor:
    """A private scratch buffer for a bpr_fwd / bpr_bwd pair (the shared grow-only workspace may be
    reused by other ops between the two calls)."""
    return torch.empty(int(_lib.lib().crh_bpr_workspace_bytes(int(batch))), dtype=torch.uint8, device=device)


def build_plans(user_idx, pos_idx, neg_idx, batch_size: int) -> np.ndarray:
    """Host: reverse indices ("plans") for every batch of an epoch of triples (int32 numpy arrays as the
    sampler returns them).  Row b of the result is the plan of batch b (last batch: its own size)."""
    L = _lib.lib()
    u, p, n = (np.ascontiguousarray(x, dtype=np.int32) for x in (user_idx, pos_idx, neg_idx))
    n_rec = u.shape[0]
    n_batches = (n_rec + batch_size - 1) // batch_size
    stride = int(L.crh_bpr_plan_ints(batch_size))
    out = np.zeros((n_batches, stride), np.int32)
    for b in range(n_batches):
        lo, hi = b * batch_size, min((b + 1) * batch_size, n_rec)
        rc = L.crh_bpr_plan_build_host(u[lo:hi].ctypes.data, p[lo:hi].ctypes.data, n[lo:hi].ctypes.data,
                                       hi - lo, batch_size, out[b].ctypes.data)
        _lib.check(rc, "crh_bpr_plan_build_host")
    return out


def plan_shape(n_records: int, batch_size: int):
    """(n_batches, ints per plan) of ``build_plans_device``'s result."""
    return (n_records + batch_size - 1) // batch_size, int(_lib.lib().crh_bpr_plan_ints(int(batch_size)))


def build_plans_device(user_idx: torch.Tensor, pos_idx: torch.Tensor, neg_idx: torch.Tensor,
                       batch_size: int, lds_max_batch: int = 8192, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Plans of every batch of an epoch, (n_batches, stride) int32 on the GPU: one launch of crh_bpr_plan_build (LDS
    sort per batch) for batch_size <= 8192, crh_bpr_plan_build_large (several workgroups per batch) above that.
    ``lds_max_batch`` below 8192 sends smaller batches through the large builder too (tests); ``out``: build in place."""
    _need_cuda(user_idx, pos_idx, neg_idx)
    L = _lib.lib()
    n_rec = user_idx.numel()
    nb = (n_rec + batch_size - 1) // batch_size
    stride = int(L.crh_bpr_plan_ints(batch_size))
    u, p, n = (x.to(torch.int32).contiguous() for x in (user_idx, pos_idx, neg_idx))
    if out is not None:
        assert out.shape == (nb, stride) and out.dtype == torch.int32 and out.is_contiguous()
    if batch_size <= min(8192, lds_max_batch):
        plans = out if out is not None else torch.empty((nb, stride), dtype=torch.int32, device=user_idx.device)
        _lib.check(L.crh_bpr_plan_build(_lib.ptr(u), _lib.ptr(p), _lib.ptr(n), n_rec, int(batch_size),
                                        _lib.ptr(plans), _lib.current_stream()), "crh_bpr_plan_build")
        return plans
    plans = out if out is not None else torch.empty((nb, stride), dtype=torch.int32, device=user_idx.device)
    group = max(1, min(nb, (256 << 20) // (48 * int(batch_size) + 4096)))     # batches per call: workspace <= ~256 MB
    for b0 in range(0, nb, group):
        b1 = min(nb, b0 + group)
        lo, hi = b0 * batch_size, min(n_rec, b1 * batch_size)
        ws_bytes = int(L.crh_bpr_plan_build_large_workspace_bytes(hi - lo, int(batch_size)))
        ws = _workspace(ws_bytes, user_idx.device)
        _lib.check(L.crh_bpr_plan_build_large(_lib.ptr(u[lo:hi]), _lib.ptr(p[lo:hi]), _lib.ptr(n[lo:hi]), hi - lo,
                                              int(batch_size), _lib.ptr(plans[b0:b1]), _lib.ptr(ws), ws_bytes,
                                              _lib.current_stream()), "crh_bpr_plan_build_large")
    return plans


# ----------------------------------------------------------------------------- MF step in one launch
def mf_step_parts(n_rows: int, d: int) -> int:
    return int(_lib.lib().crh_mf_step_parts(int(n_rows), int(d)))


def bpr_fwd_parts(batch: int, d: int) -> int:
    return int(_lib.lib().crh_bpr_fwd_parts(int(batch), int(d)))


def mf_step_tables(plans: torch.Tensor, user_idx, pos_idx, neg_idx, batch_size: int, user_rows: int, item_rows: int,
                   out=None):
    """Flattened per-epoch tables of crh_mf_step_f32: (range (nb, rows, 2), mult (nb, rows), entries (nb, 3B, 2))."""
    _need_cuda(plans, user_idx, pos_idx, neg_idx)
    nb, R, n_rec = plans.shape[0], int(user_rows) + int(item_rows), user_idx.numel()
    assert nb == (n_rec + batch_size - 1) // batch_size
    if out is None:
        i32 = dict(dtype=torch.int32, device=plans.device)
        out = (torch.empty((nb, R, 2), **i32), torch.empty((nb, R), **i32), torch.zeros((nb, 3 * batch_size, 2), **i32))
    rng, mult, ent = out
    assert rng.shape == (nb, R, 2) and mult.shape == (nb, R) and ent.shape == (nb, 3 * batch_size, 2)
    _lib.check(_lib.lib().crh_mf_step_tables(_lib.ptr(plans), _lib.ptr(user_idx), _lib.ptr(pos_idx), _lib.ptr(neg_idx),
                                             n_rec, int(batch_size), int(user_rows), int(item_rows), _lib.ptr(rng),
                                             _lib.ptr(mult), _lib.ptr(ent), _lib.current_stream()),
               "crh_mf_step_tables")
    return out


def mf_step(table_in, table_out, m, v, user_rows: int, batch: int, reg: float, plan, rng, entries, mult_next,
            part_in, n_parts_in: int, part_out, loss_prev, batch_prev: int, loss_out, step_scalars,
            beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8, sgd_lr: Optional[float] = None) -> None:
    """One whole optimiser step of model/MF.py:19-27 in one launch (crh_mf_step_f32, see include/coldrec_hip.h);
    ``sgd_lr`` selects torch.optim.SGD(lr) instead of Adam (crh_mf_step_sgd_f32: m, v, step_scalars unused)."""
    _need_cuda(table_in, table_out, m, v, plan, rng, entries, part_in, part_out, step_scalars)
    R, d = table_in.shape
    for t in (table_in, table_out) + (() if sgd_lr is not None else (m, v)):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (R, d)
    for t in (plan, rng, entries):
        assert t.dtype == torch.int32 and t.is_contiguous()
    assert rng.shape == (R, 2) and (mult_next is None or (mult_next.shape == (R,) and mult_next.is_contiguous()))
    if sgd_lr is not None:
        rc = _lib.lib().crh_mf_step_sgd_f32(
            _lib.ptr(table_in), _lib.ptr(table_out), int(user_rows), R - int(user_rows), d, int(batch), float(reg),
            _lib.ptr(plan), _lib.ptr(rng), _lib.ptr(entries), _lib.ptr(mult_next), _lib.ptr(part_in), int(n_parts_in),
            _lib.ptr(part_out), _lib.ptr(loss_prev), int(batch_prev), _lib.ptr(loss_out), float(sgd_lr),
            _lib.current_stream())
        _lib.check(rc, "crh_mf_step_sgd_f32")
        return
    rc = _lib.lib().crh_mf_step_f32(
        _lib.ptr(table_in), _lib.ptr(table_out), _lib.ptr(m), _lib.ptr(v), int(user_rows), R - int(user_rows), d,
        int(batch), float(reg), _lib.ptr(plan), _lib.ptr(rng), _lib.ptr(entries), _lib.ptr(mult_next),
        _lib.ptr(part_in), int(n_parts_in), _lib.ptr(part_out), _lib.ptr(loss_prev), int(batch_prev),
        _lib.ptr(loss_out), beta1, beta2, eps, _lib.ptr(step_scalars), _lib.current_stream())
    _lib.check(rc, "crh_mf_step_f32")


def mf_step_finish(part_in, n_parts_in: int, batch: int, loss_out) -> None:
    _need_cuda(part_in, loss_out)
    _lib.check(_lib.lib().crh_mf_step_finish(_lib.ptr(part_in), int(n_parts_in), int(batch), _lib.ptr(loss_out),
                                             _lib.current_stream()), "crh_mf_step_finish")


def adam_step_scalars(first_step: int, n_steps: int, lr: float = 1e-3, betas=(0.9, 0.999)) -> np.ndarray:
    """(n_steps, 2) float32 host array of the step-dependent Adam factors for steps first_step.."""
    out = np.empty((n_steps, 2), np.float32)
    _lib.lib().crh_adam_step_scalars_range_host(float(lr), float(betas[0]), float(betas[1]), int(first_step),
                                                int(n_steps), out.ctypes.data)
    return out


def adam_dense(p, g, m, v, step: int, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
               zero_grad: bool = True, second=None, step_scalars: Optional[torch.Tensor] = None):
    """In-place dense Adam on (p, g, m, v) [and ``second`` = another such 4-tuple] -- model/MF.py:14,27."""
    ts = (p, g, m, v) + (tuple(second) if second else ())
    _need_cuda(*ts)
    for t in ts:
        assert t.dtype == torch.float32 and t.is_contiguous()
    n0 = p.numel()
    s = second if second else (None, None, None, None)
    n1 = s[0].numel() if second else 0
    rc = _lib.lib().crh_adam_dense_f32(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n0,
                                       _lib.ptr(s[0]), _lib.ptr(s[1]), _lib.ptr(s[2]), _lib.ptr(s[3]), n1,
                                       float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                                       1 if zero_grad else 0, _lib.ptr(step_scalars), _lib.current_stream())
    _lib.check(rc, "crh_adam_dense_f32")


def adam_rows(p, g, m, v, last_step, plan, batch: int, user_rows: int, step: int, scalar_table, mode: int,
              betas=(0.9, 0.999), eps: float = 1e-8):
    """Touched-rows replay of dense Adam (crh_adam_rows_f32): mode 0 catch-up / 1 step / 2 flush."""
    _need_cuda(p, g, m, v, last_step, plan, scalar_table)
    assert last_step.dtype == torch.int32 and scalar_table.dtype == torch.float32
    assert scalar_table.numel() >= 2 * (step + 1), "scalar table too short for this step"
    rc = _lib.lib().crh_adam_rows_f32(_lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), _lib.ptr(last_step),
                                      p.shape[0], p.shape[1], _lib.ptr(plan), int(batch), int(user_rows), int(step),
                                      _lib.ptr(scalar_table), float(betas[0]), float(betas[1]), float(eps), int(mode),
                                      _lib.current_stream())
    _lib.check(rc, "crh_adam_rows_f32")


def sgd_dense(p, g, lr: float, zero_grad: bool = True):
    """In-place torch.optim.SGD(lr) defaults on a dense tensor: p <- fma(-lr, g, p) (crh_sgd_dense_f32)."""
    _need_cuda(p, g)
    assert p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
    _lib.check(_lib.lib().crh_sgd_dense_f32(_lib.ptr(p), _lib.ptr(g), p.numel(), float(lr), 1 if zero_grad else 0,
                                            _lib.current_stream()), "crh_sgd_dense_f32")


def sgd_rows(p, g, plan, batch: int, user_rows: int, lr: float):
    """The same update on the rows of one batch's plan only (crh_sgd_rows_f32); clears the consumed gradient rows."""
    _need_cuda(p, g, plan)
    assert p.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous() and plan.dtype == torch.int32
    _lib.check(_lib.lib().crh_sgd_rows_f32(_lib.ptr(p), _lib.ptr(g), p.shape[1], _lib.ptr(plan), int(batch),
                                           int(user_rows), float(lr), _lib.current_stream()), "crh_sgd_rows_f32")


def spmm_csr_sgd(rowptr, col, val, x, acc_in, s_in: float, acc_out, s_out: float, sched, p, lr: float,
                 zero_acc_in: bool = False) -> None:
    """g = (acc_in*s_in + A @ x)*s_out -> p <- fma(-lr, g, p) in the SpMM's epilogue (crh_spmm_csr_sgd_f32)."""
    _need_cuda(rowptr, col, val, x, acc_in, acc_out, p)
    n_rows, d = rowptr.shape[0] - 1, x.shape[1]
    assert x.dtype == torch.float32 and x.is_contiguous()          # x may hold more rows than A (row-sharded propagation)
    assert p.dtype == torch.float32 and p.is_contiguous() and p.shape == (n_rows, d)
    rc = _lib.lib().crh_spmm_csr_sgd_f32(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), n_rows, _lib.ptr(x), d,
                                         _lib.ptr(acc_in), float(s_in), _lib.ptr(acc_out), float(s_out),
                                         ctypes.byref(sched.for_launch(n_rows, d, col, val)) if sched is not None else None, _lib.ptr(p), float(lr),
                                         int(bool(zero_acc_in)), _lib.current_stream())
    _lib.check(rc, "crh_spmm_csr_sgd_f32")


def l2_norm(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """|x|_F as a device scalar (crh_l2_norm_f32; deterministic two-stage reduction)."""
    _need_cuda(x)
    assert x.dtype == torch.float32 and x.is_contiguous()
    L = _lib.lib()
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = torch.empty(int(L.crh_l2_workspace_bytes()), dtype=torch.uint8, device=x.device)
    _lib.check(L.crh_l2_norm_f32(_lib.ptr(x), x.numel(), _lib.ptr(out), _lib.ptr(ws), ws.numel(), _lib.current_stream()),
               "crh_l2_norm_f32")
    return out


def l2_reg_bwd(x: torch.Tensor, reg: float, norm: torch.Tensor, grad_out: Optional[torch.Tensor]) -> torch.Tensor:
    """d(reg * |x|_F / rows)/dx * grad_out (crh_l2_reg_bwd_f32)."""
    _need_cuda(x, norm, grad_out)
    gx = torch.empty_like(x)
    go = None if grad_out is None else grad_out.reshape(1).float().contiguous()
    _lib.check(_lib.lib().crh_l2_reg_bwd_f32(_lib.ptr(x), x.numel(), x.shape[0], float(reg), _lib.ptr(norm), _lib.ptr(go),
                                             _lib.ptr(gx), 0, _lib.current_stream()), "crh_l2_reg_bwd_f32")
    return gx


def spmm_csr_adam(rowptr, col, val, x, acc_in, s_in: float, acc_out, s_out: float, sched, p, m, v, step: int,
                  lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, step_scalars=None,
                  zero_acc_in: bool = False) -> None:
    """g = (acc_in*s_in + A @ x)*s_out -> one Adam step on (p, m, v) in the SpMM's epilogue (crh_spmm_csr_adam_f32);
    ``zero_acc_in`` clears acc_in row by row once consumed.  Same bits as spmm_csr(acc_out=g) + adam_dense."""
    _need_cuda(rowptr, col, val, x, acc_in, acc_out, p, m, v, step_scalars)
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    n_rows, d = rowptr.shape[0] - 1, x.shape[1]
    assert x.dtype == torch.float32 and x.is_contiguous()          # x may hold more rows than A (row-sharded propagation)
    for t in (p, m, v):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape == (n_rows, d)
    rc = _lib.lib().crh_spmm_csr_adam_f32(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), n_rows, _lib.ptr(x), d,
                                          _lib.ptr(acc_in), float(s_in), _lib.ptr(acc_out), float(s_out),
                                          ctypes.byref(sched.for_launch(n_rows, d, col, val)) if sched is not None else None, _lib.ptr(p),
                                          _lib.ptr(m), _lib.ptr(v), float(lr), float(betas[0]), float(betas[1]),
                                          float(eps), int(step), _lib.ptr(step_scalars), int(bool(zero_acc_in)),
                                          _lib.current_stream())
    _lib.check(rc, "crh_spmm_csr_adam_f32")


class SpmmSchedule:
    """Load-balancing schedule of one CSR matrix (see crh_spmm_sched), built once per graph on the host with numpy.
    Work items are ROWS, ordered by descending length: the lane groups of a wave (8 rows at d=128 with 4 column
    slices) then walk rows of about the same length instead of waiting for the longest of a Zipf-shaped sample, and
    the longest rows start first.  Rows with more than crh_spmm_segment_edges() edges are "heavy" (a workgroup
    each); they sit at the end of the list with seg_slot >= 0 and the light path skips them.  Rows are independent,
    so the order does not change any result."""

    SLAB_MAX_EDGES = 1 << 26          # the record stream is built for graphs up to this many stored edges
    GIANT = 1024                      # heavy rows above this many edges are cut into 2 (above 4x: 4) column ranges; 0 = never
    SLAB_BUCKETS = 12                 # CRH_SPMM_SLAB_BUCKETS of include/coldrec_hip.h

    def __init__(self, rowptr, device, seg: Optional[int] = None, col=None, val=None):
        """``col`` / ``val`` (the matrix's edge arrays, host or device): with them the schedule can also lay the light rows
        out as a record stream (crh_spmm_sched::slab) for the lane-group width of a launch -- see ``for_launch``."""
        rp = rowptr.cpu().numpy() if torch.is_tensor(rowptr) else np.asarray(rowptr)
        rp = rp.astype(np.int64)
        self._rp, self._col, self._val, self._device, self._slabs = rp, col, val, device, {}
        self._checked, self._baked = None, None
        deg = np.diff(rp)
        if seg is None:
            # heavy threshold: crh_spmm_segment_edges() (64) for sparse graphs; for dense ones (MovieLens shape: mean
            # degree 133, nine rows in ten above 64) a workgroup per row is the costlier path: 256 there
            # (SpMM 59.0 -> 54.7 us; CiteULike shape, mean 11.5: 20 us at 64, 32 us at 256)
            seg = int(_lib.lib().crh_spmm_segment_edges())
            if "CRH_SPMM_SEG" not in os.environ and len(deg) and float(deg.mean()) > 48.0:
                seg *= 4
        self.seg = int(seg)
        heavy = deg > seg
        order = np.argsort(-deg, kind="stable")
        order = np.concatenate([order[~heavy[order]], order[heavy[order]]])
        seg_row = order.astype(np.int32)
        seg_slot = np.where(heavy[order], 0, -1).astype(np.int32)
        seg_ptr = np.zeros(len(seg_row) + 1, np.int64)              # not read any more (kept for the ABI struct)
        # heavy rows: one entry per heavy BLOCK, longest rows first (they lead the grid: the longest chains start with the
        # first wave of workgroups).  Rows above GIANT edges are cut into 2 (4 above 4 * GIANT) column ranges of the slice,
        # one workgroup each with half (a quarter) of the lanes per lane group: multi_count = n_sub | sub << 8.
        giant, giant4 = self.GIANT, 4 * self.GIANT
        hrows = np.nonzero(heavy)[0]
        hrows = hrows[np.argsort(-deg[hrows], kind="stable")]
        n_sub = np.where(deg[hrows] > giant4, 4, np.where(deg[hrows] > giant, 2, 1)) if giant > 0 else np.ones(len(hrows), np.int64)
        multi_row = np.repeat(hrows, n_sub).astype(np.int32)
        sub = (np.arange(len(multi_row)) - np.repeat(np.cumsum(n_sub) - n_sub, n_sub)).astype(np.int64)
        multi_count = (np.repeat(n_sub, n_sub) | (sub << 8)).astype(np.int32)
        assert np.isin(multi_count & 0xff, (1, 2, 4)).all() and ((multi_count >> 8) < (multi_count & 0xff)).all()
        multi_first = np.zeros(len(multi_row) + 1, np.int64)          # not read any more (kept for the ABI struct)
        # one 16-byte descriptor per work item: {row, first edge, edges, slot}
        desc = None
        if len(deg) and int(rp[-1]) < (1 << 31):
            desc = np.stack([seg_row, rp[:-1][order].astype(np.int32), deg[order].astype(np.int32), seg_slot], 1)
            desc = np.ascontiguousarray(desc.astype(np.int32).reshape(-1))
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        self.t = (to(seg_row), to(seg_ptr), to(seg_slot), to(multi_row), to(multi_first[:-1].astype(np.int32)),
                  to(multi_count))
        self.desc = to(desc) if desc is not None else None
        self.c = _lib.SpmmSched(_lib.ptr(self.t[0]), _lib.ptr(self.t[1]), _lib.ptr(self.t[2]), len(seg_row),
                                _lib.ptr(self.t[3]) if len(multi_row) else None,
                                _lib.ptr(self.t[4]) if len(multi_row) else None,
                                _lib.ptr(self.t[5]) if len(multi_row) else None, len(multi_row),
                                int(multi_first[-1]), int(rp[-1]), _lib.ptr(self.desc))
        self.c.version = _lib.SPMM_SCHED_VERSION
        self.n_partial = int(multi_first[-1])
        self.n_seg = len(seg_row)
        self._ws = {}
        self._light = order[~heavy[order]].astype(np.int64)        # light rows in work-item order (descending length)

    def _build_slab(self, G: int):
        """The light rows as a stream of (col, val-bits) pairs for lane groups of G lanes: record = header pair {row, cnt}
        + the edges in order, padded to whole units of G pairs; rows are in descending length, so equal unit counts are
        contiguous buckets.  Returns (stream tensor, first, units, base) or None when it does not apply."""
        if self._col is None or self._val is None or G != 8 or int(self._rp[-1]) > self.SLAB_MAX_EDGES:    # (kernel: G == 8 only)
            return None
        rows = self._light
        deg = (self._rp[rows + 1] - self._rp[rows]).astype(np.int64)
        units = np.where(deg <= G - 1, 1, 1 + (deg - (G - 1) + G - 1) // G)
        cuts = np.nonzero(np.diff(units))[0] + 1 if len(units) else np.zeros(0, np.int64)
        first = np.concatenate([[0], cuts]).astype(np.int64) if len(units) else np.zeros(0, np.int64)
        if len(first) > self.SLAB_BUCKETS or len(rows) >= (1 << 31) - 1:
            return None
        start = np.zeros(len(rows) + 1, np.int64)
        np.cumsum(units * G, out=start[1:])
        n_pairs = int(start[-1]) + 2 * G                                   # tail: a one-unit record's second-unit read
        col = self._col.cpu().numpy() if torch.is_tensor(self._col) else np.asarray(self._col)
        val = self._val.cpu().numpy() if torch.is_tensor(self._val) else np.asarray(self._val)
        # what exactly is being baked in: version counters of the source tensors and two checksums of the host copies taken
        # NOW (a later in-place ``val.mul_(c)`` must not pass for "the same edges" because the pointer is the same).
        # Position-weighted (sum of (i + 1) x_i in int64, wrapping on both sides): a permutation of the edges does not pass either
        wts = np.arange(1, len(col) + 1, dtype=np.int64)
        with np.errstate(over="ignore"):
            self._baked = (self._col._version if torch.is_tensor(self._col) else None,
                           self._val._version if torch.is_tensor(self._val) else None, len(col),
                           int((col.astype(np.int64) * wts).sum()),
                           int((np.ascontiguousarray(val, np.float32).view(np.int32).astype(np.int64) * wts).sum()))
        stream = np.zeros((n_pairs, 2), np.uint32)
        stream[start[:-1], 0] = rows.astype(np.uint32)
        stream[start[:-1], 1] = deg.astype(np.uint32)
        tot = int(deg.sum())
        if tot:
            within = np.arange(tot, dtype=np.int64) - np.repeat(np.cumsum(deg) - deg, deg)
            dst = np.repeat(start[:-1] + 1, deg) + within
            src = np.repeat(self._rp[rows], deg) + within
            stream[dst, 0] = col[src].astype(np.uint32)
            stream[dst, 1] = np.ascontiguousarray(val[src], np.float32).view(np.uint32)
        return (torch.from_numpy(stream.view(np.int32)).to(self._device), first, units[first] if len(first) else first,
                start[first] if len(first) else first)

    def _same_edges(self, col, val) -> bool:
        """Are the launch's edge arrays the ones the record stream was built from?  The stream bakes (col, val) of the LIGHT
        rows in while the heavy rows read the launch's arrays: a caller that hands a rescaled ``val`` (or another matrix) to
        a reused schedule would get a mix of both.  The schedule's own tensors pass by identity + version counter;
        any other pair is checked by two position-weighted 64-bit checksums against the bake-time sums (one reduction each) --
        remembered only for the same tensor objects -- and a pair that does not match, or cannot be checked because the stream
        is being captured, takes the descriptor path, which reads the launch's arrays."""
        if col is None or val is None:
            return True
        baked = getattr(self, "_baked", None)
        if baked is None:
            return False                                      # no stream was built: nothing to vouch for
        # (1) the very tensor OBJECTS the schedule holds (kept alive by it), untouched since the bake: no device work
        if col is self._col and val is self._val and (col._version, val._version) == baked[:2]:
            return True
        # (2) the pair checked last, still the same objects at the same versions.  Keyed by object identity through weak
        # references, never by address: a fresh ``val`` every step is usually recycled at the address of the last one
        # (an address-keyed entry then vouched for contents it never saw)
        last = self._checked
        if last is not None and last[0]() is col and last[1]() is val and last[2:4] == (col._version, val._version):
            return last[4]
        if col.is_cuda and torch.cuda.is_current_stream_capturing():
            if not getattr(self, "_warned_capture", False):
                self._warned_capture = True
                import warnings
                warnings.warn("SpmmSchedule: an edge-array pair met inside a stream capture has not been checked against the "
                              "record stream; this launch (and the captured graph) takes the slower descriptor path -- bind the "
                              "pair once eagerly (sched.for_launch(n, d, col, val)) before capturing")
            return False                                      # not remembered: an eager launch decides
        # (3) position-weighted checksums of the launch's arrays against the BAKE-TIME sums (a permutation changes them)
        ok = col.numel() == baked[2] and val.numel() == baked[2]
        if ok:
            w = torch.arange(1, col.numel() + 1, dtype=torch.int64, device=col.device)
            ok = int((col.to(torch.int64) * w).sum()) == baked[3] and \
                int((val.view(torch.int32).to(torch.int64) * w).sum()) == baked[4]
        self._checked = (weakref.ref(col), weakref.ref(val), col._version, val._version, ok)
        return ok

    def for_launch(self, n_rows: int, d: int, col=None, val=None):
        """Point the C struct at the record stream laid out for THIS launch's lane-group width (built once per width);
        without edge arrays, where the stream does not apply, or when the launch's (col, val) are not the arrays the stream
        was built from (``_same_edges``), the launch takes the descriptor path.  A schedule is bound to ONE (col, val)."""
        c = self.c
        G = int(_lib.lib().crh_spmm_lane_group(int(n_rows), int(d), int(self._rp[-1]))) if self._col is not None else 0
        if G not in self._slabs:
            self._slabs[G] = self._build_slab(G) if G else None
        slab = self._slabs[G]
        if slab is not None and not self._same_edges(col, val):
            slab = None
        if slab is None:
            c.slab, c.slab_lanes, c.slab_buckets, c.n_slab = None, 0, 0, 0
            return c
        stream, first, units, base = slab
        c.slab, c.slab_lanes, c.slab_buckets, c.n_slab = _lib.ptr(stream), G, len(first), len(self._light)
        for b in range(self.SLAB_BUCKETS):
            c.slab_first[b] = int(first[b]) if b < len(first) else 0x7fffffff
            c.slab_units[b] = int(units[b]) if b < len(first) else 1
            c.slab_base[b] = int(base[b]) if b < len(first) else 0
        return c

    def workspace(self, d: int, device) -> Optional[torch.Tensor]:
        """Heavy rows are combined on chip: crh_spmm_workspace_bytes() is 0 and no scratch is needed."""
        return None


def spmm_csr(rowptr, col, val, x, y=None, acc_in=None, s_in: float = 1.0, acc_out=None, s_out: float = 1.0,
             sched: Optional[SpmmSchedule] = None):
    """P = A @ x; y = P; acc_out = (acc_in*s_in + P)*s_out  (model/LightGCN.py:88-93, fused layer sum)."""
    _need_cuda(rowptr, col, val, x, y, acc_in, acc_out)
    assert rowptr.dtype == torch.int64 and col.dtype == torch.int32 and val.dtype == torch.float32
    assert x.dtype == torch.float32 and x.is_contiguous()
    n_rows, d = rowptr.shape[0] - 1, x.shape[1]
    ws = sched.workspace(d, x.device) if sched is not None else None
    rc = _lib.lib().crh_spmm_csr_f32(_lib.ptr(rowptr), _lib.ptr(col), _lib.ptr(val), n_rows, _lib.ptr(x), d,
                                     _lib.ptr(y), _lib.ptr(acc_in), float(s_in), _lib.ptr(acc_out), float(s_out),
                                     ctypes.byref(sched.for_launch(n_rows, d, col, val)) if sched is not None else None,
                                     _lib.ptr(ws), ws.numel() * 4 if ws is not None else 0,
                                     _lib.current_stream())
    _lib.check(rc, "crh_spmm_csr_f32")


# ---- what the fused losses check alike: op = the name in front of a message, what = the noun the message uses ----------

def _check_2d_f32(op: str, what: str, *tensors) -> None:
    for t in tensors:
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
            raise RuntimeError(f"{op}: {what} must be contiguous 2-D float32 tensors")


def _grad_buffer(op: str, what: str, g, like: torch.Tensor, want: bool, overwritten: bool):
    """The gradient buffer of ``like``: the one given (checked), else a new one when wanted -- ``empty`` when the kernel
    writes every row, ``zeros`` when rows it does not touch must read zero --, else None."""
    if g is None:
        if not want:
            return None
        return torch.empty_like(like) if overwritten else torch.zeros_like(like)
    if g.dtype != torch.float32 or not g.is_contiguous() or g.shape != like.shape:
        raise RuntimeError(f"{op}: gradient buffers must be contiguous float32 tensors of {what}")
    return g


def _check_width(op: str, d: int, widest: int = 256) -> None:
    if d % 4 != 0 or d < 4 or d > widest:
        raise RuntimeError(f"{op}: width {d} must be a multiple of 4 in [4, {widest}]")


def _check_one_device(op: str, whose: str, dev, *tensors) -> None:
    for t in tensors:
        if t is not None and t.device != dev:
            raise RuntimeError(f"{op}: every tensor must be on {whose} device")


def _check_ids_in_tables(op: str, what: str, user_range, item_range, user_table, item_table) -> None:
    """what: "ids", or "the plan's ids" where the ranges were measured when the plan was made."""
    if user_range[0] < 0 or user_range[1] >= user_table.shape[0] or item_range[0] < 0 \
            or item_range[1] >= item_table.shape[0]:
        raise RuntimeError(f"{op}: {what} lie outside the tables")


_AT_LEAST = {1: "one element", 3: "three elements", 4: "four elements", 5: "five elements", 6: "six elements"}


def _loss_buffer(op: str, loss, n: int, device) -> torch.Tensor:
    if loss is None:
        return torch.empty(n, dtype=torch.float32, device=device)
    if loss.dtype != torch.float32 or not loss.is_contiguous() or loss.numel() < n:
        raise RuntimeError(f"{op}: loss must be a contiguous float32 buffer of at least {_AT_LEAST[n]}")
    return loss


def _new_workspace(nbytes: int, device) -> torch.Tensor:
    """Private scratch of one fused-loss shape (the caching allocator hands out 512-byte aligned blocks)."""
    return torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)


def _workspace_arg(op: str, workspace, make, *shape) -> torch.Tensor:
    """The workspace given (checked), else ``make(*shape)``."""
    if workspace is None:
        return make(*shape)
    if workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise RuntimeError(f"{op}: workspace must be a contiguous uint8 tensor")
    return workspace


# ---- contrastive learning (infonce.hip) ------------------------------------------------------------------------------

def infonce_workspace_bytes(n_max: int, d: int) -> int:
    return int(_lib.lib().crh_infonce_workspace_bytes(int(n_max), int(d)))


def infonce_workspace(n_max: int, d: int, device) -> torch.Tensor:
    """Private scratch of one crh_infonce_f32 shape."""
    return _new_workspace(infonce_workspace_bytes(n_max, d), device)


def infonce(view1: torch.Tensor, view2: torch.Tensor, tau: float, b_cos: bool = True, rows1=None, rows2=None, n_dev=None,
            n_max: Optional[int] = None, scale: float = 1.0, accumulate: bool = False, grad1=None, grad2=None, loss=None,
            workspace=None, want_grad1: bool = True, want_grad2: bool = True):
    """InfoNCE loss and both input gradients in one call (crh_infonce_f32).  view1 / view2: fp32 contiguous (rows, d),
    d % 4 == 0 <= 256 (``util.utils.InfoNCE`` pads other widths); rows1 / rows2: optional unique int32 row ids (the batch is
    view[rows[:N]]), n_dev: optional device int32 N.  Returns (loss, grad1, grad2); grad* = d loss / d view * scale,
    written (or added, ``accumulate``) at the batch's rows only.  A gradient that is neither given nor wanted is not
    computed (None is returned for it; without grad2 the column pass is skipped)."""
    _need_cuda(view1, view2, rows1, rows2, n_dev, grad1, grad2, loss, workspace)
    dev = view1.device
    _check_2d_f32("infonce", "views", view1, view2)
    if view1.shape[1] != view2.shape[1]:
        raise RuntimeError("infonce: views differ in width")
    _check_one_device("infonce", "the views'", dev, view2, rows1, rows2, n_dev, grad1, grad2, loss, workspace)
    for r in (rows1, rows2):
        if r is not None and (r.dtype != torch.int32 or not r.is_contiguous() or r.dim() != 1):
            raise RuntimeError("infonce: row ids must be contiguous 1-D int32")
    if n_dev is not None and (n_dev.dtype != torch.int32 or n_dev.numel() < 1):
        raise RuntimeError("infonce: n_dev must be a device int32 scalar")
    loss = _loss_buffer("infonce", loss, 1, dev)
    d = view1.shape[1]
    if n_max is None:
        n_max = rows1.shape[0] if rows1 is not None else view1.shape[0]
    if rows1 is None and view1.shape[0] < n_max or rows2 is None and view2.shape[0] < n_max \
            or rows1 is not None and rows1.shape[0] < n_max or rows2 is not None and rows2.shape[0] < n_max:
        raise RuntimeError("infonce: fewer rows than n_max")

    def whole(v, rows):   # every row is overwritten only when the batch is the whole view
        return rows is None and n_dev is None and not accumulate and v.shape[0] == n_max

    grad1 = _grad_buffer("infonce", "the views' shapes", grad1, view1, want_grad1, whole(view1, rows1))
    grad2 = _grad_buffer("infonce", "the views' shapes", grad2, view2, want_grad2, whole(view2, rows2))
    workspace = _workspace_arg("infonce", workspace, infonce_workspace, n_max, d, dev)
    _lib.check(_lib.lib().crh_infonce_f32(_lib.ptr(view1), _lib.ptr(rows1), _lib.ptr(view2), _lib.ptr(rows2), _lib.ptr(n_dev),
                                          int(n_max), int(d), float(tau), int(bool(b_cos)), float(scale), int(bool(accumulate)),
                                          _lib.ptr(grad1), _lib.ptr(grad2), _lib.ptr(loss), _lib.ptr(workspace),
                                          workspace.numel(), _lib.current_stream()), "crh_infonce_f32")
    return loss, grad1, grad2


# ---- NCL's whole-table contrast (table_nce.hip) ----------------------------------------------------------------------

def table_nce_workspace_bytes(batch_max: int, n_rows: int, d: int) -> int:
    return int(_lib.lib().crh_table_nce_workspace_bytes(int(batch_max), int(n_rows), int(d)))


def table_nce_workspace(batch_max: int, n_rows: int, d: int, device) -> torch.Tensor:
    """Private scratch of one crh_table_nce_f32 shape: linear in n_rows, nothing of size batch x n_rows."""
    return _new_workspace(table_nce_workspace_bytes(batch_max, n_rows, d), device)


def table_nce(ctx: torch.Tensor, table: torch.Tensor, idx: torch.Tensor, tau: float, n_dev=None,
              batch_max: Optional[int] = None, scale: float = 1.0, accumulate: bool = False, grad_ctx=None, grad_table=None,
              loss=None, workspace=None, want_grad_ctx: bool = True, want_grad_table: bool = True):
    """sum_b (logsumexp_j <normalize(ctx[idx_b]), normalize(table[j])> / tau - the same at j = idx_b) and both input
    gradients in one call (crh_table_nce_f32; reference model/NCL.py:68-94).  ctx / table: fp32 contiguous (n_rows, d),
    d % 4 == 0 <= 256, possibly the same tensor; idx: int32 row ids in [0, n_rows) -- NOT checked --, duplicates allowed;
    n_dev: optional device int32 batch size.  Returns (loss, grad_ctx, grad_table): grad_ctx = d loss / d ctx * scale at the
    batch's rows only (a new buffer is zero elsewhere), grad_table = d loss / d table * scale at every row; ``accumulate``
    adds into given buffers.  A gradient that is neither given nor wanted is not computed (None is returned for it;
    without grad_table the column pass is skipped)."""
    _need_cuda(ctx, table, idx, n_dev, grad_ctx, grad_table, loss, workspace)
    dev = ctx.device
    _check_2d_f32("table_nce", "ctx and table", ctx, table)
    if ctx.shape != table.shape:
        raise RuntimeError("table_nce: ctx and table differ in shape")
    _check_one_device("table_nce", "ctx's", dev, table, idx, n_dev, grad_ctx, grad_table, loss, workspace)
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.dim() != 1:
        raise RuntimeError("table_nce: row ids must be contiguous 1-D int32")
    if n_dev is not None and (n_dev.dtype != torch.int32 or n_dev.numel() < 1):
        raise RuntimeError("table_nce: n_dev must be a device int32 scalar")
    loss = _loss_buffer("table_nce", loss, 1, dev)
    n_rows, d = table.shape
    if batch_max is None:
        batch_max = idx.shape[0]
    if idx.shape[0] < batch_max:
        raise RuntimeError("table_nce: fewer row ids than batch_max")
    grad_ctx = _grad_buffer("table_nce", "ctx's shape", grad_ctx, ctx, want_grad_ctx, False)
    grad_table = _grad_buffer("table_nce", "the table's shape", grad_table, table, want_grad_table,
                              n_dev is None and not accumulate and batch_max > 0)   # every table row is written
    workspace = _workspace_arg("table_nce", workspace, table_nce_workspace, batch_max, n_rows, d, dev)
    _lib.check(_lib.lib().crh_table_nce_f32(_lib.ptr(ctx), _lib.ptr(table), int(n_rows), _lib.ptr(idx), _lib.ptr(n_dev),
                                            int(batch_max), int(d), float(tau), float(scale), int(bool(accumulate)),
                                            _lib.ptr(grad_ctx), _lib.ptr(grad_table), _lib.ptr(loss), _lib.ptr(workspace),
                                            workspace.numel(), _lib.current_stream()), "crh_table_nce_f32")
    return loss, grad_ctx, grad_table


# ---- CLCRec's contrastive loss (clcrec.hip) --------------------------------------------------------------------------

def clcrec_max_neg() -> int:
    return int(_lib.lib().crh_clcrec_max_neg())


def clcrec_workspace_bytes(batch: int, n_neg: int, d: int, n_slots: int) -> int:
    return int(_lib.lib().crh_clcrec_workspace_bytes(int(batch), int(n_neg), int(d), int(n_slots)))


def clcrec_workspace(batch: int, n_neg: int, d: int, n_slots: int, device) -> torch.Tensor:
    return _new_workspace(clcrec_workspace_bytes(batch, n_neg, d, n_slots), device)


def _grouped(ids: torch.Tensor):
    """ids (M,) int64 -> (the distinct ids ascending, every position's index into them, the positions grouped by id -- a
    stable sort, so ascending inside an id --, the groups' sizes and offsets)."""
    uniq, inv = torch.unique(ids, return_inverse=True)
    order = torch.sort(inv, stable=True).indices
    cnt = torch.bincount(inv, minlength=uniq.shape[0])
    ptr = torch.zeros(uniq.shape[0] + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(cnt, 0, out=ptr[1:])
    return uniq, inv, order, cnt, ptr


def _owner_chunks(ids: torch.Tensor, chunk: int):
    """``_grouped`` with every group cut into chunks of ``chunk`` positions: (distinct ids, grouped positions, offsets,
    offsets into the chunk list, each chunk's group, every position's index into the distinct ids)."""
    uniq, inv, order, cnt, ptr = _grouped(ids)
    nch = (cnt + (chunk - 1)) // chunk
    chunk_ptr = torch.zeros(uniq.shape[0] + 1, dtype=torch.int64, device=ids.device)
    torch.cumsum(nch, 0, out=chunk_ptr[1:])
    chunk_own = torch.repeat_interleave(torch.arange(uniq.shape[0], device=ids.device), nch)
    return uniq, order, ptr, chunk_ptr, chunk_own, inv


def _owner_index(items: torch.Tensor, users: torch.Tensor, chunk: int) -> dict:
    """The inverse-index half of a plan: ``_owner_chunks`` of the item and of the user occurrences as int32 tensors, with
    the counts the kernels take."""
    out = {}
    for side, ids in (("item", items), ("user", users)):
        own_ids, occ, ptr, chunk_ptr, chunk_own = (t.to(torch.int32).contiguous() for t in _owner_chunks(ids, chunk)[:5])
        out.update({f"n_{side}s": int(own_ids.shape[0]), f"n_{side}_chunks": int(chunk_own.shape[0]), f"{side}_ids": own_ids,
                    f"{side}_ptr": ptr, f"{side}_occ": occ, f"{side}_chunk_ptr": chunk_ptr, f"{side}_chunk_own": chunk_own})
    return out


def _owner_args(plan: dict) -> tuple:
    """The inverse-index arguments of crh_ccfcrec_f32, crh_gar_f32, crh_mtpr_f32 and crh_vbpr_f32 in ABI order: the item
    side's five arrays and two counts, then the user side's."""
    p, ptr = plan, _lib.ptr
    return (ptr(p["item_ids"]), ptr(p["item_ptr"]), ptr(p["item_occ"]), ptr(p["item_chunk_ptr"]), ptr(p["item_chunk_own"]),
            int(p["n_items"]), int(p["n_item_chunks"]),
            ptr(p["user_ids"]), ptr(p["user_ptr"]), ptr(p["user_occ"]), ptr(p["user_chunk_ptr"]), ptr(p["user_chunk_own"]),
            int(p["n_users"]), int(p["n_user_chunks"]))


def _triple_plan_checks(op: str, plan: dict, user_table, item_table, *others) -> tuple:
    """What ``gar``, ``mtpr`` and ``vbpr`` check of their plan: its arrays on the tables' device with the call's other
    tensors, its ids inside the tables.  Returns (user min, user max, item min, item max) as the ABI takes them."""
    _check_one_device(op, "the tables'", user_table.device, item_table, *others, plan["users"])
    (u_lo, u_hi), (i_lo, i_hi) = plan["user_range"], plan["item_range"]
    _check_ids_in_tables(op, "ids", (u_lo, u_hi), (i_lo, i_hi), user_table, item_table)
    return int(u_lo), int(u_hi), int(i_lo), int(i_hi)


def _check_ids_in_plan(op: str, user_range, item_range, n_users: Optional[int], n_items: Optional[int]) -> None:
    if n_users is not None and (user_range[0] < 0 or user_range[1] >= n_users):
        raise RuntimeError(f"{op}: user id outside the user table")
    if n_items is not None and (item_range[0] < 0 or item_range[1] >= n_items):
        raise RuntimeError(f"{op}: item id outside the item table")


def clcrec_plan(users: torch.Tensor, items: torch.Tensor, n_users: Optional[int] = None,
                n_items: Optional[int] = None) -> dict:
    """The index side of one crh_clcrec_f32 step.  users (B,), items (B, 1 + G): integer device tensors (column 0 = the
    positive).  Returns int32 device tensors: users, items (flat), slot (the feat row of every flat row), slot_item (the
    distinct items, ascending: what the encoder has to encode), and the inverse indices -- the flat rows grouped by slot
    (slot_ptr, slot_rows; a stable sort, so ascending inside a slot), the slots' rows cut into chunks of
    crh_clcrec_chunk_rows() (chunk_ptr, chunk_slot), the records grouped by user (user_ids, user_ptr, user_recs).
    With n_users / n_items given, ids outside the tables raise instead of reaching the kernel."""
    _need_cuda(users, items)
    if users.dim() != 1 or items.dim() != 2 or items.shape[0] != users.shape[0] or items.shape[1] < 2 or users.shape[0] < 1:
        raise RuntimeError("clcrec_plan: users must be (B,) and items (B, 1 + G) with B >= 1, G >= 1")
    if users.dtype.is_floating_point or items.dtype.is_floating_point or users.device != items.device:
        raise RuntimeError("clcrec_plan: users and items must be integer tensors on one device")
    flat = items.reshape(-1).long()
    ulong = users.long()
    user_range, item_range = (int(ulong.min()), int(ulong.max())), (int(flat.min()), int(flat.max()))
    _check_ids_in_plan("clcrec_plan", user_range, item_range, n_users, n_items)

    chunk = int(_lib.lib().crh_clcrec_chunk_rows())
    slot_item, slot_rows, slot_ptr, chunk_ptr, chunk_slot, slot = _owner_chunks(flat, chunk)
    user_ids, _, user_recs, _, user_ptr = _grouped(ulong)
    c = lambda t: t.to(torch.int32).contiguous()
    return dict(batch=int(users.shape[0]), n_neg=int(items.shape[1] - 1), n_slots=int(slot_item.shape[0]),
                n_chunks=int(chunk_slot.shape[0]), n_users=int(user_ids.shape[0]),
                user_range=user_range, item_range=item_range,
                users=c(ulong), items=c(flat), slot=c(slot), slot_item=c(slot_item), slot_ptr=c(slot_ptr),
                slot_rows=c(slot_rows), chunk_ptr=c(chunk_ptr), chunk_slot=c(chunk_slot), user_ids=c(user_ids),
                user_ptr=c(user_ptr), user_recs=c(user_recs))


def clcrec(user_table: torch.Tensor, item_table: torch.Tensor, feat: torch.Tensor, plan: dict, mix_count: torch.Tensor,
           temp: float, lr_lambda: float, reg: float, scale: float = 1.0, grad_user=None, grad_item=None, grad_feat=None,
           loss=None, workspace=None, want_user: bool = True, want_item: bool = True, want_feat: bool = True):
    """CLCRec's loss and its three gradients in one call (crh_clcrec_f32).  user_table (nu, d), item_table (ni, d), feat
    (plan['n_slots'], d): fp32 contiguous, d % 4 == 0 <= 256; plan: ``clcrec_plan``; mix_count: int32 (B (1 + G),), how often
    the step's random index drew each flat row.  Returns (loss4 = [L1, L2, R, total], grad_user, grad_item, grad_feat);
    gradients are d total / d table * scale, zero at rows the batch does not touch; one that is neither given nor wanted
    is not computed (None)."""
    _need_cuda(user_table, item_table, feat, mix_count, grad_user, grad_item, grad_feat, loss, workspace)
    dev = user_table.device
    _check_2d_f32("clcrec", "tables and feat", user_table, item_table, feat)
    d = user_table.shape[1]
    if item_table.shape[1] != d or feat.shape[1] != d:
        raise RuntimeError("clcrec: tables and feat differ in width")
    _check_width("clcrec", d)
    B, G, S = plan["batch"], plan["n_neg"], plan["n_slots"]
    if feat.shape[0] != S:
        raise RuntimeError("clcrec: feat must have one row per slot of the plan")
    _check_ids_in_tables("clcrec", "the plan's ids", plan["user_range"], plan["item_range"], user_table, item_table)
    if mix_count.dtype != torch.int32 or not mix_count.is_contiguous() or mix_count.numel() != B * (1 + G):
        raise RuntimeError("clcrec: mix_count must be a contiguous int32 tensor of B * (1 + G) elements")
    _check_one_device("clcrec", "the tables'", dev, item_table, feat, mix_count, plan["users"], grad_user, grad_item,
                      grad_feat, loss, workspace)

    grad_user = _grad_buffer("clcrec", "the tables' shapes", grad_user, user_table, want_user, False)
    grad_item = _grad_buffer("clcrec", "the tables' shapes", grad_item, item_table, want_item, False)
    grad_feat = _grad_buffer("clcrec", "the tables' shapes", grad_feat, feat, want_feat, True)
    loss = _loss_buffer("clcrec", loss, 4, dev)
    workspace = _workspace_arg("clcrec", workspace, clcrec_workspace, B, G, d, S, dev)
    p = plan
    _lib.check(_lib.lib().crh_clcrec_f32(
        _lib.ptr(user_table), _lib.ptr(item_table), _lib.ptr(feat), _lib.ptr(p["users"]), _lib.ptr(p["items"]),
        _lib.ptr(p["slot"]), _lib.ptr(p["slot_item"]), _lib.ptr(mix_count), _lib.ptr(p["slot_ptr"]), _lib.ptr(p["slot_rows"]),
        _lib.ptr(p["chunk_ptr"]), _lib.ptr(p["chunk_slot"]), int(p["n_chunks"]), _lib.ptr(p["user_ids"]),
        _lib.ptr(p["user_ptr"]), _lib.ptr(p["user_recs"]), int(p["n_users"]), int(B), int(G), int(d), int(S), float(temp),
        float(lr_lambda), float(reg), float(scale), _lib.ptr(grad_user), _lib.ptr(grad_item), _lib.ptr(grad_feat),
        _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(), _lib.current_stream()), "crh_clcrec_f32")
    return loss, grad_user, grad_item, grad_feat


# ---- CCFCRec's loss (ccfcrec.hip) ------------------------------------------------------------------------------------

def ccfcrec_max_rows() -> int:
    return int(_lib.lib().crh_ccfcrec_max_rows())


def ccfcrec_rows(n_pos: int, n_neg: int, n_self: int) -> int:
    """R = 1 + P + P N + S: the item rows one record gathers."""
    return 1 + int(n_pos) + int(n_pos) * int(n_neg) + int(n_self)


def ccfcrec_workspace_bytes(batch: int, n_pos: int, n_neg: int, n_self: int, d: int, n_items: int, n_users: int) -> int:
    return int(_lib.lib().crh_ccfcrec_workspace_bytes(int(batch), int(n_pos), int(n_neg), int(n_self), int(d),
                                                      int(n_items), int(n_users)))


def ccfcrec_workspace(batch: int, n_pos: int, n_neg: int, n_self: int, d: int, n_items: int, n_users: int,
                      device) -> torch.Tensor:
    return _new_workspace(ccfcrec_workspace_bytes(batch, n_pos, n_neg, n_self, d, n_items, n_users), device)


def ccfcrec_plan(users: torch.Tensor, items: torch.Tensor, neg_users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor,
                 self_neg: torch.Tensor, n_users: Optional[int] = None, n_items: Optional[int] = None) -> dict:
    """The index side of one crh_ccfcrec_f32 step.  users, items, neg_users (B,), pos (B, P), neg (B, P, N), self_neg
    (B, S): integer device tensors.  Returns int32 device tensors: users, neg_users, items (B R flat: the record's item, its
    positives, negatives, self-negatives) and the inverse indices -- the flat rows grouped by item (item_ids, item_ptr,
    item_occ; a stable sort, so ascending inside an item) and cut into chunks of crh_ccfcrec_chunk_rows() (item_chunk_ptr,
    item_chunk_own), and the same over the 2B user occurrences (users, then neg_users).  With n_users / n_items given,
    ids outside the tables raise instead of reaching the kernel."""
    _need_cuda(users, items, neg_users, pos, neg, self_neg)
    B = users.shape[0] if users.dim() == 1 else 0
    if B < 1 or items.shape != (B,) or neg_users.shape != (B,) or pos.dim() != 2 or neg.dim() != 3 or self_neg.dim() != 2 \
            or pos.shape[0] != B or neg.shape[:2] != pos.shape or self_neg.shape[0] != B or pos.shape[1] < 1 \
            or neg.shape[2] < 1 or self_neg.shape[1] < 1:
        raise RuntimeError("ccfcrec_plan: users, items, neg_users must be (B,), pos (B, P), neg (B, P, N), self_neg (B, S) "
                           "with B, P, N, S >= 1")
    ts = (users, items, neg_users, pos, neg, self_neg)
    if any(t.dtype.is_floating_point or t.device != users.device for t in ts):
        raise RuntimeError("ccfcrec_plan: the six index tensors must be integer tensors on one device")
    P, N, S = int(pos.shape[1]), int(neg.shape[2]), int(self_neg.shape[1])
    flat = torch.cat([items.long().view(B, 1), pos.long(), neg.long().reshape(B, P * N), self_neg.long()], 1).reshape(-1)
    both = torch.cat([users.long(), neg_users.long()])
    user_range, item_range = (int(both.min()), int(both.max())), (int(flat.min()), int(flat.max()))
    _check_ids_in_plan("ccfcrec_plan", user_range, item_range, n_users, n_items)
    c = lambda t: t.to(torch.int32).contiguous()
    return dict(batch=B, n_pos=P, n_neg=N, n_self=S, user_range=user_range, item_range=item_range, users=c(both[:B]),
                neg_users=c(both[B:]), items=c(flat),
                **_owner_index(flat, both, int(_lib.lib().crh_ccfcrec_chunk_rows())))


def ccfcrec(user_table: torch.Tensor, item_table: torch.Tensor, q: torch.Tensor, plan: dict, tau: float, lambda1: float,
            scale: float = 1.0, grad_user=None, grad_item=None, grad_q=None, loss=None, workspace=None,
            want_user: bool = True, want_item: bool = True, want_q: bool = True):
    """CCFCRec's loss and its three gradients in one call (crh_ccfcrec_f32).  user_table (nu, d), item_table (ni, d), q
    (B, d) = the content encoder's output for the records' items: fp32 contiguous, d % 4 == 0 <= 256; plan:
    ``ccfcrec_plan``.  Returns (loss5 = [L_c, L_s, L_r1, L_r2, total], grad_user, grad_item, grad_q); gradients are
    d total / d table * scale, zero at rows the batch does not touch; one that is neither given nor wanted is not
    computed (None).  Rows of zero norm are outside the contract (the reference divides by the norm)."""
    _need_cuda(user_table, item_table, q, grad_user, grad_item, grad_q, loss, workspace)
    dev = user_table.device
    _check_2d_f32("ccfcrec", "tables and q", user_table, item_table, q)
    d = user_table.shape[1]
    if item_table.shape[1] != d or q.shape[1] != d:
        raise RuntimeError("ccfcrec: tables and q differ in width")
    _check_width("ccfcrec", d)
    B, P, N, S = plan["batch"], plan["n_pos"], plan["n_neg"], plan["n_self"]
    if ccfcrec_rows(P, N, S) > ccfcrec_max_rows():
        raise RuntimeError(f"ccfcrec: 1 + P + P N + S = {ccfcrec_rows(P, N, S)} rows per record exceed the cap "
                           f"{ccfcrec_max_rows()}")
    if q.shape[0] != B:
        raise RuntimeError("ccfcrec: q must have one row per record of the plan")
    _check_ids_in_tables("ccfcrec", "the plan's ids", plan["user_range"], plan["item_range"], user_table, item_table)
    _check_one_device("ccfcrec", "the tables'", dev, item_table, q, plan["users"], grad_user, grad_item, grad_q, loss,
                      workspace)

    grad_user = _grad_buffer("ccfcrec", "the tables' shapes", grad_user, user_table, want_user, False)
    grad_item = _grad_buffer("ccfcrec", "the tables' shapes", grad_item, item_table, want_item, False)
    grad_q = _grad_buffer("ccfcrec", "the tables' shapes", grad_q, q, want_q, True)
    loss = _loss_buffer("ccfcrec", loss, 5, dev)
    workspace = _workspace_arg("ccfcrec", workspace, ccfcrec_workspace, B, P, N, S, d, plan["n_items"], plan["n_users"],
                               dev)
    p = plan
    _lib.check(_lib.lib().crh_ccfcrec_f32(
        _lib.ptr(user_table), int(user_table.shape[0]), _lib.ptr(item_table), int(item_table.shape[0]), _lib.ptr(q),
        _lib.ptr(p["users"]), _lib.ptr(p["neg_users"]), _lib.ptr(p["items"]), int(p["user_range"][0]),
        int(p["user_range"][1]), int(p["item_range"][0]), int(p["item_range"][1]), *_owner_args(p), int(B), int(P), int(N),
        int(S), int(d), float(tau), float(lambda1), float(scale), _lib.ptr(grad_user), _lib.ptr(grad_item), _lib.ptr(grad_q),
        _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(), _lib.current_stream()), "crh_ccfcrec_f32")
    return loss, grad_user, grad_item, grad_q


# ---- ALDI's loss (aldi.hip) ------------------------------------------------------------------------------------------

def aldi_workspace_bytes(batch: int, d: int) -> int:
    return int(_lib.lib().crh_aldi_workspace_bytes(int(batch), int(d)))


def aldi_workspace(batch: int, d: int, device) -> torch.Tensor:
    return _new_workspace(aldi_workspace_bytes(batch, d), device)


def aldi(user_table: torch.Tensor, item_table: torch.Tensor, users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor,
         gen_user: torch.Tensor, gen_pos: torch.Tensor, gen_neg: torch.Tensor, item_weight: torch.Tensor, alpha: float,
         beta: float, gamma: float, scale: float = 1.0, want_user: bool = True, want_pos: bool = True,
         want_neg: bool = True, grad_user=None, grad_pos=None, grad_neg=None, loss=None, workspace=None, id_range=None):
    """ALDI's loss and its three gradients in one call (crh_aldi_f32).  user_table (nu, d), item_table (ni, d): the frozen
    teacher; users, pos, neg (B,) integer ids; gen_user, gen_pos, gen_neg (B, d): the student towers' outputs; item_weight
    (ni,); fp32 contiguous, d % 4 == 0 <= 256.  Returns (loss5 = [L_bpr, L_rate, L_rank, L_iden, total], d_gen_user,
    d_gen_pos, d_gen_neg); gradients are d total / d gen_* * scale; one that is neither given nor wanted is not computed
    (None).  id_range = ((user min, user max), (item min, item max)) when the caller knows them (a trainer that sampled the
    ids on the host); measured here otherwise, which waits for the device."""
    _need_cuda(user_table, item_table, users, pos, neg, gen_user, gen_pos, gen_neg, item_weight, grad_user, grad_pos,
               grad_neg, loss, workspace)
    dev = user_table.device
    _check_2d_f32("aldi", "tables and tower outputs", user_table, item_table, gen_user, gen_pos, gen_neg)
    d = user_table.shape[1]
    _check_width("aldi", d)
    B = users.shape[0] if users.dim() == 1 else 0
    if B < 1 or pos.shape != (B,) or neg.shape != (B,):
        raise RuntimeError("aldi: users, pos, neg must be (B,) with B >= 1")
    if item_table.shape[1] != d or any(t.shape != (B, d) for t in (gen_user, gen_pos, gen_neg)):
        raise RuntimeError("aldi: the tower outputs must be (B, d) of the tables' width")
    if item_weight.dtype != torch.float32 or not item_weight.is_contiguous() or item_weight.shape != (item_table.shape[0],):
        raise RuntimeError("aldi: item_weight must be a contiguous float32 vector with one entry per item")
    ids = (users, pos, neg)
    if any(t.dtype.is_floating_point for t in ids):
        raise RuntimeError("aldi: users, pos, neg must be integer tensors")
    _check_one_device("aldi", "the tables'", dev, item_table, *ids, gen_user, gen_pos, gen_neg, item_weight, grad_user,
                      grad_pos, grad_neg, loss, workspace)
    if id_range is None:
        items = torch.cat([pos.reshape(-1), neg.reshape(-1)])
        id_range = ((int(users.min()), int(users.max())), (int(items.min()), int(items.max())))
    (u_lo, u_hi), (i_lo, i_hi) = id_range
    _check_ids_in_tables("aldi", "ids", (u_lo, u_hi), (i_lo, i_hi), user_table, item_table)
    users, pos, neg = (t.to(torch.int32).contiguous() for t in ids)

    grad_user, grad_pos, grad_neg = (_grad_buffer("aldi", "the tower outputs' shape", g, gen_user, want, True)
                                     for g, want in ((grad_user, want_user), (grad_pos, want_pos), (grad_neg, want_neg)))
    loss = _loss_buffer("aldi", loss, 5, dev)
    workspace = _workspace_arg("aldi", workspace, aldi_workspace, B, d, dev)
    _lib.check(_lib.lib().crh_aldi_f32(
        _lib.ptr(user_table), int(user_table.shape[0]), _lib.ptr(item_table), int(item_table.shape[0]), _lib.ptr(users),
        _lib.ptr(pos), _lib.ptr(neg), int(u_lo), int(u_hi), int(i_lo), int(i_hi), _lib.ptr(gen_user), _lib.ptr(gen_pos),
        _lib.ptr(gen_neg), _lib.ptr(item_weight), int(B), int(d), float(alpha), float(beta), float(gamma), float(scale),
        _lib.ptr(grad_user), _lib.ptr(grad_pos), _lib.ptr(grad_neg), _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(),
        _lib.current_stream()), "crh_aldi_f32")
    return loss, grad_user, grad_pos, grad_neg


# ---- GAR's loss (gar.hip) --------------------------------------------------------------------------------------------

def gar_chunk_rows() -> int:
    return int(_lib.lib().crh_gar_chunk_rows())


def gar_workspace_bytes(batch: int, d: int, n_items: int, n_users: int) -> int:
    return int(_lib.lib().crh_gar_workspace_bytes(int(batch), int(d), int(n_items), int(n_users)))


def gar_workspace(batch: int, d: int, n_items: int, n_users: int, device) -> torch.Tensor:
    return _new_workspace(gar_workspace_bytes(batch, d, n_items, n_users), device)


def _triple_plan(op: str, chunk_rows, users, pos, neg, n_users, n_items, id_range, chunk) -> dict:
    """``gar_plan`` / ``mtpr_plan``: op fronts the messages, chunk_rows() is the library's chunk size."""
    B = users.shape[0] if users.dim() == 1 else 0
    if B < 1 or pos.shape != (B,) or neg.shape != (B,):
        raise RuntimeError(f"{op}: users, pos, neg must be (B,) with B >= 1")
    if any(t.dtype.is_floating_point or t.device != users.device for t in (users, pos, neg)):
        raise RuntimeError(f"{op}: users, pos, neg must be integer tensors on one device")
    ulong = users.long()
    both = torch.cat([pos.long(), neg.long()])
    if id_range is None:
        id_range = ((int(ulong.min()), int(ulong.max())), (int(both.min()), int(both.max())))
    user_range, item_range = (tuple(int(x) for x in r) for r in id_range)
    _check_ids_in_plan(op, user_range, item_range, n_users, n_items)
    c = lambda t: t.to(torch.int32).contiguous()
    return dict(batch=B, user_range=user_range, item_range=item_range, users=c(ulong), pos=c(both[:B]), neg=c(both[B:]),
                **_owner_index(both, ulong, chunk_rows() if chunk is None else chunk))


def gar_plan(users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, n_users: Optional[int] = None,
             n_items: Optional[int] = None, id_range=None, chunk: Optional[int] = None) -> dict:
    """The index side of one crh_gar_f32 step.  users, pos, neg (B,): integer tensors on one device.  Returns int32 tensors:
    users, pos, neg and the inverse indices -- the records grouped by user (user_ids, user_ptr, user_occ; a stable sort,
    so ascending inside a user) and cut into chunks of crh_gar_chunk_rows() (user_chunk_ptr, user_chunk_own), and the same
    over the 2B item occurrences (pos, then neg).  id_range = ((user min, user max), (item min, item max)) when the caller
    knows them (a trainer that sampled the ids on the host); measured here otherwise, which waits for the device.  With
    n_users / n_items given, ids outside the tables raise instead of reaching the kernel.  ``chunk`` is the library's
    unless given (the grouping is plain tensor code and runs on any device)."""
    return _triple_plan("gar_plan", gar_chunk_rows, users, pos, neg, n_users, n_items, id_range, chunk)


def gar(user_table: torch.Tensor, item_table: torch.Tensor, gen: torch.Tensor, plan: dict, alpha: float, beta: float,
        reg: float, cold_user: bool = False, scale: float = 1.0, want_user: bool = True, want_item: bool = True,
        want_gen: bool = True, grad_user=None, grad_item=None, grad_gen=None, loss=None, workspace=None):
    """GAR's loss and its three gradients in one call (crh_gar_f32).  user_table (nu, d), item_table (ni, d): the trained
    tables; gen (B, d) = the generator's output for the records (the positives' content, or the users' when cold_user);
    fp32 contiguous, d % 4 == 0 <= 256; plan: ``gar_plan``.  Returns (loss4 = [L_gen, L_rec, R, total], grad_user,
    grad_item, grad_gen); gradients are d total / d . * scale, the tables' zero at rows the batch does not touch; one
    that is neither given nor wanted is not computed (None)."""
    _need_cuda(user_table, item_table, gen, plan["users"], grad_user, grad_item, grad_gen, loss, workspace)
    dev = user_table.device
    _check_2d_f32("gar", "tables and the generator's output", user_table, item_table, gen)
    d = user_table.shape[1]
    _check_width("gar", d)
    B = plan["batch"]
    if item_table.shape[1] != d or gen.shape != (B, d):
        raise RuntimeError("gar: the generator's output must be (B, d) of the tables' width, one row per record of the plan")
    id_range = _triple_plan_checks("gar", plan, user_table, item_table, gen, grad_user, grad_item, grad_gen, loss, workspace)

    grad_user = _grad_buffer("gar", "the tables' and the generator output's shapes", grad_user, user_table, want_user, False)
    grad_item = _grad_buffer("gar", "the tables' and the generator output's shapes", grad_item, item_table, want_item, False)
    grad_gen = _grad_buffer("gar", "the tables' and the generator output's shapes", grad_gen, gen, want_gen, True)
    loss = _loss_buffer("gar", loss, 4, dev)
    workspace = _workspace_arg("gar", workspace, gar_workspace, B, d, plan["n_items"], plan["n_users"], dev)
    p = plan
    _lib.check(_lib.lib().crh_gar_f32(
        _lib.ptr(user_table), int(user_table.shape[0]), _lib.ptr(item_table), int(item_table.shape[0]), _lib.ptr(gen),
        _lib.ptr(p["users"]), _lib.ptr(p["pos"]), _lib.ptr(p["neg"]), *id_range, *_owner_args(p), int(B), int(d),
        int(bool(cold_user)), float(alpha), float(beta), float(reg), float(scale), _lib.ptr(grad_user), _lib.ptr(grad_item),
        _lib.ptr(grad_gen), _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(), _lib.current_stream()), "crh_gar_f32")
    return loss, grad_user, grad_item, grad_gen


# ---- MTPR's loss (mtpr.hip) and the touched-rows Adagrad (adagrad.hip) -----------------------------------------------

def mtpr_chunk_rows() -> int:
    return int(_lib.lib().crh_mtpr_chunk_rows())


def mtpr_workspace_bytes(batch: int, d: int, cold_user: bool, n_items: int, n_users: int) -> int:
    return int(_lib.lib().crh_mtpr_workspace_bytes(int(batch), int(d), int(bool(cold_user)), int(n_items), int(n_users)))


def mtpr_workspace(batch: int, d: int, cold_user: bool, n_items: int, n_users: int, device) -> torch.Tensor:
    return _new_workspace(mtpr_workspace_bytes(batch, d, cold_user, n_items, n_users), device)


def mtpr_plan(users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, n_users: Optional[int] = None,
              n_items: Optional[int] = None, id_range=None, chunk: Optional[int] = None) -> dict:
    """The index side of one crh_mtpr_f32 step: ``gar_plan``'s arrays (same arguments, same id_range shortcut, same
    errors) with the owners' occurrences cut into chunks of crh_mtpr_chunk_rows().  user_ids / item_ids are the distinct
    ids, ascending: what ``adagrad_rows`` steps."""
    return _triple_plan("mtpr_plan", mtpr_chunk_rows, users, pos, neg, n_users, n_items, id_range, chunk)


def mtpr(user_table: torch.Tensor, item_table: torch.Tensor, h: torch.Tensor, weu: torch.Tensor, wei: torch.Tensor,
         plan: dict, wd1: float, cold_user: bool = False, scale: float = 1.0, want_user: bool = True,
         want_item: bool = True, want_h: bool = True, want_weu: bool = True, want_wei: bool = True, grad_user=None,
         grad_item=None, grad_h=None, grad_weu=None, grad_wei=None, loss=None, workspace=None):
    """MTPR's four ranking terms, the tables' regulariser and their five gradients in one call (crh_mtpr_f32).  d = the
    embedding width (d % 4 == 0, 4 <= d <= 128); weu, wei (2 d, d).  Item mode: user_table (nu, 2 d), item_table (ni, d),
    h (2 B, d) = the content projections of the positives, then of the negatives.  User mode (cold_user): user_table
    (nu, d), item_table (ni, 2 d), h (B, d) = the users' content projections.  fp32 contiguous; plan: ``mtpr_plan``.
    Returns (loss6 = [L_i, L_f, L_if, L_fi, R_emb, sum], grad_user, grad_item, grad_h, grad_weu, grad_wei); gradients
    are d sum / d . * scale.  The table gradients are written at the rows the batch touches ONLY: a caller's buffer keeps
    every other row as it was (a new one is zeroed).  A gradient that is neither given nor wanted is not computed (None)."""
    _need_cuda(user_table, item_table, h, weu, wei, plan["users"], grad_user, grad_item, grad_h, grad_weu, grad_wei, loss,
               workspace)
    dev = user_table.device
    _check_2d_f32("mtpr", "tables, content rows and projections", user_table, item_table, h, weu, wei)
    cold_user = bool(cold_user)
    d = weu.shape[1]
    _check_width("mtpr", d, 128)
    B = plan["batch"]
    wp, wq, hr = (d, 2 * d, B) if cold_user else (2 * d, d, 2 * B)
    if weu.shape != (2 * d, d) or wei.shape != (2 * d, d):
        raise RuntimeError("mtpr: weu and wei must be (2 d, d)")
    if user_table.shape[1] != wp or item_table.shape[1] != wq or h.shape != (hr, d):
        raise RuntimeError("mtpr: item mode takes tables (nu, 2 d), (ni, d) and h (2 B, d); user mode (nu, d), (ni, 2 d) "
                           "and h (B, d), B the plan's batch")
    id_range = _triple_plan_checks("mtpr", plan, user_table, item_table, h, weu, wei, grad_user, grad_item, grad_h, grad_weu,
                                   grad_wei, loss, workspace)

    what = "the shapes of the tables, the content rows and the projections"
    grad_user = _grad_buffer("mtpr", what, grad_user, user_table, want_user, False)
    grad_item = _grad_buffer("mtpr", what, grad_item, item_table, want_item, False)
    grad_h = _grad_buffer("mtpr", what, grad_h, h, want_h, True)
    grad_weu = _grad_buffer("mtpr", what, grad_weu, weu, want_weu, True)
    grad_wei = _grad_buffer("mtpr", what, grad_wei, wei, want_wei, True)
    loss = _loss_buffer("mtpr", loss, 6, dev)
    workspace = _workspace_arg("mtpr", workspace, mtpr_workspace, B, d, cold_user, plan["n_items"], plan["n_users"], dev)
    p = plan
    _lib.check(_lib.lib().crh_mtpr_f32(
        _lib.ptr(user_table), int(user_table.shape[0]), _lib.ptr(item_table), int(item_table.shape[0]), _lib.ptr(h),
        _lib.ptr(weu), _lib.ptr(wei), _lib.ptr(p["users"]), _lib.ptr(p["pos"]), _lib.ptr(p["neg"]), *id_range,
        *_owner_args(p), int(B), int(d), int(cold_user), float(wd1), float(scale), _lib.ptr(grad_user), _lib.ptr(grad_item),
        _lib.ptr(grad_h), _lib.ptr(grad_weu), _lib.ptr(grad_wei), _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(),
        _lib.current_stream()), "crh_mtpr_f32")
    return loss, grad_user, grad_item, grad_h, grad_weu, grad_wei


# ---- the two-tower BPR loss of VBPR and AMR (vbpr.hip) ---------------------------------------------------------------

def vbpr_chunk_rows() -> int:
    return int(_lib.lib().crh_vbpr_chunk_rows())


def vbpr_workspace_bytes(batch: int, d: int, cold_user: bool, n_items: int, n_users: int) -> int:
    return int(_lib.lib().crh_vbpr_workspace_bytes(int(batch), int(d), int(bool(cold_user)), int(n_items), int(n_users)))


def vbpr_workspace(batch: int, d: int, cold_user: bool, n_items: int, n_users: int, device) -> torch.Tensor:
    return _new_workspace(vbpr_workspace_bytes(batch, d, cold_user, n_items, n_users), device)


def vbpr_plan(users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, n_users: Optional[int] = None,
              n_items: Optional[int] = None, id_range=None, chunk: Optional[int] = None) -> dict:
    """The index side of one crh_vbpr_f32 step: ``gar_plan``'s arrays (same arguments, same id_range shortcut, same
    errors) with the owners' occurrences cut into chunks of crh_vbpr_chunk_rows().  user_ids / item_ids are the distinct
    ids, ascending: what ``adagrad_rows`` steps and the order of ``vbpr``'s grad_hsum rows."""
    return _triple_plan("vbpr_plan", vbpr_chunk_rows, users, pos, neg, n_users, n_items, id_range, chunk)


def vbpr(user_table: torch.Tensor, item_table: torch.Tensor, aux_table: torch.Tensor, h: torch.Tensor, plan: dict,
         wd1: float, h_adv: Optional[torch.Tensor] = None, lmd: float = 1.0, cold_user: bool = False, scale: float = 1.0,
         want_user: bool = True, want_item: bool = True, want_aux: bool = True, want_h: bool = True,
         want_h_adv: bool = True, want_hsum: bool = False, want_loss: bool = True, grad_user=None, grad_item=None,
         grad_aux=None, grad_h=None, grad_h_adv=None, grad_hsum=None, loss=None, workspace=None):
    """The two-tower BPR loss of VBPR / AMR and its gradients in one call (crh_vbpr_f32).  user_table (nu, d), item_table
    (ni, d); d % 4 == 0, 4 <= d <= 256.  Item mode: aux_table (nu, d), h (2 B, d) = the content projections of the
    positives, then of the negatives; h_adv = None or the projections of the perturbed content, h's shape.  User mode
    (cold_user): aux_table (ni, d), h (B, d) = the users' content projections, no h_adv.  fp32 contiguous; plan:
    ``vbpr_plan``.  Returns (loss4 = [L_bpr, L_adv, R_emb, sum], grad_user, grad_item, grad_aux, grad_h, grad_h_adv,
    grad_hsum); gradients are d sum / d . * scale.  The table gradients are written at the rows the batch touches ONLY: a
    caller's buffer keeps every other row as it was (a new one is zeroed).  grad_hsum (n_items or n_users of the plan, d):
    row s = grad_h's (+ grad_h_adv's) rows summed over the occurrences of the plan's item_ids[s] (user mode: user_ids[s]).
    An output that is neither given nor wanted is not computed (None); want_h_adv counts only with h_adv; with
    want_loss=False and no ``loss`` the loss is not computed either -- ``vbpr(..., want_user=False, want_item=False,
    want_aux=False, want_h=False, want_hsum=True, want_loss=False)`` computes grad_hsum alone."""
    _need_cuda(user_table, item_table, aux_table, h, h_adv, plan["users"], grad_user, grad_item, grad_aux, grad_h,
               grad_h_adv, grad_hsum, loss, workspace)
    dev = user_table.device
    _check_2d_f32("vbpr", "tables and content rows", user_table, item_table, aux_table, h,
                  *(() if h_adv is None else (h_adv,)))
    cold_user = bool(cold_user)
    d = user_table.shape[1]
    _check_width("vbpr", d)
    B = plan["batch"]
    if cold_user and (h_adv is not None or grad_h_adv is not None):
        raise RuntimeError("vbpr: h_adv is item mode's only (the reference's AMR cannot train cold users)")
    if h_adv is None and grad_h_adv is not None:
        raise RuntimeError("vbpr: grad_h_adv without h_adv")
    aux_rows, hr = (item_table.shape[0], B) if cold_user else (user_table.shape[0], 2 * B)
    if item_table.shape[1] != d or aux_table.shape != (aux_rows, d) or h.shape != (hr, d) \
            or (h_adv is not None and h_adv.shape != h.shape):
        raise RuntimeError("vbpr: item mode takes tables (nu, d), (ni, d), aux (nu, d) and h, h_adv (2 B, d); user mode aux "
                           "(ni, d) and h (B, d), B the plan's batch")
    id_range = _triple_plan_checks("vbpr", plan, user_table, item_table, aux_table, h, h_adv, grad_user, grad_item, grad_aux,
                                   grad_h, grad_h_adv, grad_hsum, loss, workspace)

    what = "the shapes of the tables and the content rows"
    grad_user = _grad_buffer("vbpr", what, grad_user, user_table, want_user, False)
    grad_item = _grad_buffer("vbpr", what, grad_item, item_table, want_item, False)
    grad_aux = _grad_buffer("vbpr", what, grad_aux, aux_table, want_aux, False)
    grad_h = _grad_buffer("vbpr", what, grad_h, h, want_h, True)
    if h_adv is not None:
        grad_h_adv = _grad_buffer("vbpr", what, grad_h_adv, h_adv, want_h_adv, True)
    n_own = plan["n_users"] if cold_user else plan["n_items"]
    if grad_hsum is None:
        grad_hsum = torch.empty((n_own, d), dtype=torch.float32, device=dev) if want_hsum else None
    elif grad_hsum.dtype != torch.float32 or not grad_hsum.is_contiguous() or grad_hsum.shape != (n_own, d):
        raise RuntimeError("vbpr: grad_hsum must be a contiguous float32 tensor of (the plan's distinct cold objects, d)")
    if loss is not None or want_loss:
        loss = _loss_buffer("vbpr", loss, 4, dev)
    if all(t is None for t in (grad_user, grad_item, grad_aux, grad_h, grad_h_adv, grad_hsum, loss)):
        raise RuntimeError("vbpr: nothing to compute")
    workspace = _workspace_arg("vbpr", workspace, vbpr_workspace, B, d, cold_user, plan["n_items"], plan["n_users"], dev)
    p = plan
    _lib.check(_lib.lib().crh_vbpr_f32(
        _lib.ptr(user_table), int(user_table.shape[0]), _lib.ptr(item_table), int(item_table.shape[0]),
        _lib.ptr(aux_table), _lib.ptr(h), _lib.ptr(h_adv), _lib.ptr(p["users"]), _lib.ptr(p["pos"]), _lib.ptr(p["neg"]),
        *id_range, *_owner_args(p), int(B), int(d), int(cold_user), float(wd1), float(lmd), float(scale),
        _lib.ptr(grad_user), _lib.ptr(grad_item), _lib.ptr(grad_aux), _lib.ptr(grad_h), _lib.ptr(grad_h_adv),
        _lib.ptr(grad_hsum), _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(), _lib.current_stream()), "crh_vbpr_f32")
    return loss, grad_user, grad_item, grad_aux, grad_h, grad_h_adv, grad_hsum


# ---- DUIF's projected BPR step (duif.hip) ----------------------------------------------------------------------------

def duif_chunk_rows() -> int:
    return int(_lib.lib().crh_duif_chunk_rows())


def duif_part_chunk() -> int:
    """How many weight-gradient partials one first-stage sum adds."""
    return int(_lib.lib().crh_duif_part_chunk())


def duif_parts(rows: int, d: int, c: int) -> int:
    """The weight-gradient partials of ``rows`` projected rows (2 B in item mode, B in user mode): a function of the shape."""
    return int(_lib.lib().crh_duif_parts(int(rows), int(d), int(c)))


def duif_workspace_bytes(batch: int, d: int, c: int, cold_user: bool, n_own: int) -> int:
    return int(_lib.lib().crh_duif_workspace_bytes(int(batch), int(d), int(c), int(bool(cold_user)), int(n_own)))


def duif_workspace(batch: int, d: int, c: int, cold_user: bool, n_own: int, device) -> torch.Tensor:
    return _new_workspace(duif_workspace_bytes(batch, d, c, cold_user, n_own), device)


def duif_plan(users: torch.Tensor, pos: torch.Tensor, neg: torch.Tensor, cold_user: bool, n_users: Optional[int] = None,
              n_items: Optional[int] = None, id_range=None, chunk: Optional[int] = None) -> dict:
    """The index side of one crh_duif_f32 step.  users, pos, neg (B,): integer tensors on one device.  Only the FREE side's
    occurrences are grouped -- the B users in item mode, the 2 B items (pos, then neg) in user mode --: own_ids (the
    distinct ids, ascending), own_ptr, own_occ (a stable sort, so ascending inside an id), cut into chunks of
    crh_duif_chunk_rows() (own_chunk_ptr, own_chunk_own).  The projected side's ids are converted to int32 and nothing
    more: projection is per occurrence.  id_range, n_users, n_items and ``chunk``: as ``gar_plan``'s."""
    B = users.shape[0] if users.dim() == 1 else 0
    if B < 1 or pos.shape != (B,) or neg.shape != (B,):
        raise RuntimeError("duif_plan: users, pos, neg must be (B,) with B >= 1")
    if any(t.dtype.is_floating_point or t.device != users.device for t in (users, pos, neg)):
        raise RuntimeError("duif_plan: users, pos, neg must be integer tensors on one device")
    cold_user = bool(cold_user)
    ulong = users.long()
    both = torch.cat([pos.long(), neg.long()])
    if id_range is None:
        id_range = ((int(ulong.min()), int(ulong.max())), (int(both.min()), int(both.max())))
    user_range, item_range = (tuple(int(x) for x in r) for r in id_range)
    _check_ids_in_plan("duif_plan", user_range, item_range, n_users, n_items)
    c = lambda t: t.to(torch.int32).contiguous()
    chunk = duif_chunk_rows() if chunk is None else chunk
    own_ids, occ, ptr, chunk_ptr, chunk_own = (c(t) for t in _owner_chunks(both if cold_user else ulong, chunk)[:5])
    return dict(batch=B, cold_user=cold_user, user_range=user_range, item_range=item_range, users=c(ulong), pos=c(both[:B]),
                neg=c(both[B:]), n_own=int(own_ids.shape[0]), n_own_chunks=int(chunk_own.shape[0]), own_ids=own_ids,
                own_ptr=ptr, own_occ=occ, own_chunk_ptr=chunk_ptr, own_chunk_own=chunk_own)


def duif(table: torch.Tensor, content: torch.Tensor, w: torch.Tensor, plan: dict, reg: float, cold_user: bool = False,
         scale: float = 1.0, want_table: bool = True, want_w: bool = True, want_h: bool = False, grad_table=None,
         grad_w=None, loss=None, workspace=None):
    """One DUIF step, forward and backward, in one call (crh_duif_f32).  table (n_free, d): the trained table of the side
    without content (the users in item mode, the items when cold_user); content (n_content, c): the other side's content
    rows; w (d, c) = nn.Linear(c, d, bias=False).weight; fp32 contiguous, d % 4 == 0, 4 <= d <= 256, 1 <= c <= 4096;
    plan: ``duif_plan`` of the same cold_user.  Returns (loss3 = [L_bpr, R, total], grad_table, grad_w, H): gradients are
    d total / d . * scale, grad_table zero at rows the batch does not touch (a caller's buffer keeps those rows as they
    were); H = content[ids] @ w.T, one row per projected occurrence (item mode: the B positives, then the B negatives;
    user mode: the B users).  An output that is neither given nor wanted is not computed (None)."""
    _need_cuda(table, content, w, plan["users"], grad_table, grad_w, loss, workspace)
    dev = table.device
    _check_2d_f32("duif", "the table, the content and the projection", table, content, w)
    cold_user = bool(cold_user)
    if cold_user != plan["cold_user"]:
        raise RuntimeError("duif: the plan was made for the other cold object")
    d, c = table.shape[1], content.shape[1]
    _check_width("duif", d)
    if c < 1 or c > 4096:
        raise RuntimeError(f"duif: content width {c} must lie in [1, 4096]")
    if w.shape != (d, c):
        raise RuntimeError("duif: the projection must be (d, c): the table's width by the content's, nn.Linear's layout")
    _check_one_device("duif", "the table's", dev, content, w, plan["users"], grad_table, grad_w, loss, workspace)
    free, proj = (plan["item_range"], plan["user_range"]) if cold_user else (plan["user_range"], plan["item_range"])
    if free[0] < 0 or free[1] >= table.shape[0] or proj[0] < 0 or proj[1] >= content.shape[0]:
        raise RuntimeError("duif: ids lie outside the tables")
    B = plan["batch"]
    what = "the table's and the projection's shapes"
    grad_table = _grad_buffer("duif", what, grad_table, table, want_table, False)
    grad_w = _grad_buffer("duif", what, grad_w, w, want_w, True)
    h = torch.empty((B if cold_user else 2 * B, d), dtype=torch.float32, device=dev) if want_h else None
    loss = _loss_buffer("duif", loss, 3, dev)
    workspace = _workspace_arg("duif", workspace, duif_workspace, B, d, c, cold_user, plan["n_own"], dev)
    p, ptr = plan, _lib.ptr
    _lib.check(_lib.lib().crh_duif_f32(
        ptr(table), int(table.shape[0]), ptr(content), int(content.shape[0]), int(c), ptr(w), ptr(p["users"]), ptr(p["pos"]),
        ptr(p["neg"]), int(free[0]), int(free[1]), int(proj[0]), int(proj[1]), ptr(p["own_ids"]), ptr(p["own_ptr"]),
        ptr(p["own_occ"]), ptr(p["own_chunk_ptr"]), ptr(p["own_chunk_own"]), int(p["n_own"]), int(p["n_own_chunks"]), int(B),
        int(d), int(cold_user), float(reg), float(scale), ptr(grad_table), ptr(grad_w), ptr(h), ptr(loss), ptr(workspace),
        workspace.numel(), _lib.current_stream()), "crh_duif_f32")
    return loss, grad_table, grad_w, h


def adagrad_rows(p: torch.Tensor, g: torch.Tensor, state_sum: torch.Tensor, ids: torch.Tensor, lr: float,
                 eps: float = 1e-10, zero_grad: bool = True) -> None:
    """One step of torch.optim.Adagrad's defaults over the rows ``ids`` (int32, distinct) of p, in place:
    state_sum += g * g; p -= lr * g / (sqrt(state_sum) + eps); then g's consumed rows are cleared (crh_adagrad_rows_f32).
    p, g, state_sum: (rows, d) contiguous float32, d % 4 == 0 <= 256.  A row whose gradient is zero keeps its bits."""
    _need_cuda(p, g, state_sum, ids)
    _check_2d_f32("adagrad_rows", "p, g and state_sum", p, g, state_sum)
    if g.shape != p.shape or state_sum.shape != p.shape:
        raise RuntimeError("adagrad_rows: p, g and state_sum must have one shape")
    d = p.shape[1]
    _check_width("adagrad_rows", d)
    if ids.dtype != torch.int32 or ids.dim() != 1 or not ids.is_contiguous() or ids.shape[0] > p.shape[0]:
        raise RuntimeError("adagrad_rows: ids must be a contiguous int32 vector of distinct rows")
    _check_one_device("adagrad_rows", "p's", p.device, g, state_sum, ids)
    _lib.check(_lib.lib().crh_adagrad_rows_f32(_lib.ptr(p), _lib.ptr(g), _lib.ptr(state_sum), _lib.ptr(ids),
                                               int(ids.shape[0]), int(p.shape[0]), int(d), float(lr), float(eps),
                                               int(bool(zero_grad)), _lib.current_stream()), "crh_adagrad_rows_f32")


# ---- the two frozen-table generator losses: MetaEmbedding's (metaemb.hip) and DeepMusic's (deepmusic.hip) ------------

def metaemb_workspace_bytes(n: int, d: int) -> int:
    return int(_lib.lib().crh_metaemb_workspace_bytes(int(n), int(d)))


def metaemb_workspace(n: int, d: int, device) -> torch.Tensor:
    return _new_workspace(metaemb_workspace_bytes(n, d), device)


def deepmusic_workspace_bytes(batch: int, d: int) -> int:
    return int(_lib.lib().crh_deepmusic_workspace_bytes(int(batch), int(d)))


def deepmusic_workspace(batch: int, d: int, device) -> torch.Tensor:
    return _new_workspace(deepmusic_workspace_bytes(batch, d), device)


def _frozen_table_checks(op: str, table, ids, gen, id_range, *others):
    """What ``metaemb`` and ``deepmusic`` check alike: one frozen table, (N,) ids into it and (N, d) generated rows on one
    device.  Returns (N, d, (id min, id max), the ids as int32)."""
    _need_cuda(table, ids, gen, *others)
    _check_2d_f32(op, "the table and the generated rows", table, gen)
    d = table.shape[1]
    _check_width(op, d)
    N = ids.shape[0] if ids.dim() == 1 else 0
    if N < 1 or ids.dtype.is_floating_point:
        raise RuntimeError(f"{op}: ids must be an (N,) integer tensor with N >= 1")
    if gen.shape != (N, d):
        raise RuntimeError(f"{op}: the generated rows must be (N, d) of the table's width, one row per id")
    _check_one_device(op, "the table's", table.device, ids, gen, *others)
    if id_range is None:
        id_range = (int(ids.min()), int(ids.max()))
    lo, hi = (int(x) for x in id_range)
    if lo < 0 or hi >= table.shape[0]:
        raise RuntimeError(f"{op}: ids lie outside the table")
    return N, d, (lo, hi), ids.to(torch.int32).contiguous()


def metaemb(table: torch.Tensor, ids: torch.Tensor, emb: torch.Tensor, n_pos: int, alpha: float, cold_lr: float,
            scale: float = 1.0, want_grad: bool = True, want_scores: bool = False, grad_emb=None, loss=None, scores=None,
            workspace=None, id_range=None):
    """MetaEmbedding's loss and its gradient in one call (crh_metaemb_f32).  table (rows, d): the frozen table; ids (N,)
    integer ids into it; emb (N, d): the generated rows, one per occurrence; occurrences below n_pos have the target 1,
    the rest 0; fp32 contiguous, d % 4 == 0 <= 256.  Returns (loss3 = [L_a, L_b, ME], grad_emb, scores): grad_emb is
    d ME / d emb * scale, scores the (2, N) scores y_a, y_b; one that is neither given nor wanted is not computed (None).
    id_range = (id min, id max) when the caller knows them; measured here otherwise, which waits for the device."""
    N, d, (lo, hi), ids = _frozen_table_checks("metaemb", table, ids, emb, id_range, grad_emb, loss, scores, workspace)
    dev = table.device
    if not 0 <= int(n_pos) <= N:
        raise RuntimeError(f"metaemb: n_pos = {n_pos} out of [0, {N}]")
    grad_emb = _grad_buffer("metaemb", "the generated rows' shape", grad_emb, emb, want_grad, True)
    if scores is None:
        scores = torch.empty((2, N), dtype=torch.float32, device=dev) if want_scores else None
    elif scores.dtype != torch.float32 or not scores.is_contiguous() or scores.shape != (2, N):
        raise RuntimeError("metaemb: scores must be a contiguous float32 tensor of (2, N)")
    loss = _loss_buffer("metaemb", loss, 3, dev)
    workspace = _workspace_arg("metaemb", workspace, metaemb_workspace, N, d, dev)
    _lib.check(_lib.lib().crh_metaemb_f32(
        _lib.ptr(table), int(table.shape[0]), _lib.ptr(ids), lo, hi, _lib.ptr(emb), int(N), int(n_pos), int(d),
        float(alpha), float(cold_lr), float(scale), _lib.ptr(grad_emb), _lib.ptr(loss), _lib.ptr(scores),
        _lib.ptr(workspace), workspace.numel(), _lib.current_stream()), "crh_metaemb_f32")
    return loss, grad_emb, scores


def deepmusic(table: torch.Tensor, ids: torch.Tensor, gen: torch.Tensor, reg: float, scale: float = 1.0,
              want_grad: bool = True, grad_gen=None, loss=None, workspace=None, id_range=None):
    """DeepMusic's loss and its gradient in one call (crh_deepmusic_f32).  table (rows, d): the frozen table; ids (B,)
    integer ids into it; gen (B, d): the generated rows; fp32 contiguous, d % 4 == 0 <= 256.  Returns (loss3 = [L_mse, R,
    total], grad_gen = d total / d gen * scale, or None when neither given nor wanted).  id_range as ``metaemb``'s."""
    B, d, (lo, hi), ids = _frozen_table_checks("deepmusic", table, ids, gen, id_range, grad_gen, loss, workspace)
    dev = table.device
    grad_gen = _grad_buffer("deepmusic", "the generated rows' shape", grad_gen, gen, want_grad, True)
    loss = _loss_buffer("deepmusic", loss, 3, dev)
    workspace = _workspace_arg("deepmusic", workspace, deepmusic_workspace, B, d, dev)
    _lib.check(_lib.lib().crh_deepmusic_f32(
        _lib.ptr(table), int(table.shape[0]), _lib.ptr(ids), lo, hi, _lib.ptr(gen), int(B), int(d), float(reg),
        float(scale), _lib.ptr(grad_gen), _lib.ptr(loss), _lib.ptr(workspace), workspace.numel(), _lib.current_stream()),
        "crh_deepmusic_f32")
    return loss, grad_gen


# ---- NGCF's propagation layer (ngcf.hip) -----------------------------------------------------------------------------

def ngcf_workspace_bytes(n_rows: int, d: int) -> int:
    return int(_lib.lib().crh_ngcf_workspace_bytes(int(n_rows), int(d)))


def ngcf_workspace(n_rows: int, d: int, device) -> torch.Tensor:
    """Private scratch of one crh_ngcf_layer_bwd_f32 shape: the weight-gradient partials (at most 2048) and their sums."""
    return _new_workspace(ngcf_workspace_bytes(n_rows, d), device)


def _ngcf_checks(op: str, x: torch.Tensor, w: torch.Tensor, same_shape, others) -> None:
    dev = x.device
    _check_2d_f32(op, "tables and weights", x, w, *[t for t in same_shape if t is not None])
    for t in same_shape:
        if t is not None and t.shape != x.shape:
            raise RuntimeError(f"{op}: every table must have x's shape")
    if w.shape != (2 * x.shape[1], x.shape[1]):
        raise RuntimeError(f"{op}: w must be the stacked [Wgc; Wbi] of shape (2 d, d)")
    for t in (w, *same_shape, *others):
        if t is not None and t.device != dev:
            raise RuntimeError(f"{op}: every tensor must be on x's device")


def ngcf_layer_fwd(x: torch.Tensor, s: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, y=None,
                   acc_in=None, s_in: float = 1.0, acc_out=None, s_out: float = 1.0, want_y: bool = True):
    """One NGCF layer (crh_ngcf_layer_fwd_f32; reference model/NGCF.py:94-99): x_k = leaky_relu(s Wgc^T + bgc +
    (x * s) Wbi^T + bbi, 0.01) with s = A x, w = [Wgc; Wbi] stacked (2 d, d) and b = [bgc; bbi] (2, d) or None;
    y = x_k, acc_out = (acc_in * s_in + x_k) * s_out (the SpMM's layer-sum convention; acc_out may be acc_in).  x, s:
    fp32 contiguous (n_rows, d), d % 4 == 0 <= 256.  Returns (y, acc_out); ``want_y=False`` without ``y`` skips x_k's
    store (the last layer of an evaluation forward)."""
    _need_cuda(x, s, w, b, y, acc_in, acc_out)
    _ngcf_checks("ngcf_layer_fwd", x, w, (s, y, acc_in, acc_out), (b,))
    if b is not None and (b.dtype != torch.float32 or not b.is_contiguous() or b.shape != (2, x.shape[1])):
        raise RuntimeError("ngcf_layer_fwd: b must be the stacked [bgc; bbi], contiguous float32 of shape (2, d)")
    if y is None and (want_y or acc_out is None):
        y = torch.empty_like(x)
    _lib.check(_lib.lib().crh_ngcf_layer_fwd_f32(_lib.ptr(x), _lib.ptr(s), _lib.ptr(w), _lib.ptr(b), x.shape[0], x.shape[1],
                                                 _lib.ptr(y), _lib.ptr(acc_in), float(s_in), _lib.ptr(acc_out), float(s_out),
                                                 _lib.current_stream()), "crh_ngcf_layer_fwd_f32")
    return y, acc_out


def ngcf_layer_bwd(x: torch.Tensor, s: torch.Tensor, xk: torch.Tensor, g: Optional[torch.Tensor], dout: torch.Tensor,
                   c: float, w: torch.Tensor, ds=None, local=None, dw=None, db=None, workspace=None):
    """The backward of ``ngcf_layer_fwd`` (crh_ngcf_layer_bwd_f32): with dz = g * (xk > 0 ? 1 : 0.01) -- g = None means
    g = c * dout, the top layer -- and T = dz Wbi, returns (ds, local, dw, db): ds = dz Wgc + x * T, local = c * dout +
    s * T (so that g_{k-1} = local + A ds: the next SpMM's acc_in), dw = [dz^T s; dz^T (x * s)] in w's layout and db = dz's
    column sums (the gradient of both biases).  ``local`` may be ``g`` and ``ds`` may be ``s``; every output is written
    whole, in an order of sums fixed by the shape (two identical calls give identical bits)."""
    _need_cuda(x, s, xk, g, dout, w, ds, local, dw, db, workspace)
    _ngcf_checks("ngcf_layer_bwd", x, w, (s, xk, g, dout), (ds, local, dw, db, workspace))
    ds = _grad_buffer("ngcf_layer_bwd", "x's shape", ds, x, True, True)
    local = _grad_buffer("ngcf_layer_bwd", "x's shape", local, x, True, True)
    dw = _grad_buffer("ngcf_layer_bwd", "w's shape", dw, w, True, True)
    if db is None:
        db = torch.empty(x.shape[1], dtype=torch.float32, device=x.device)
    elif db.dtype != torch.float32 or not db.is_contiguous() or db.shape != (x.shape[1],):
        raise RuntimeError("ngcf_layer_bwd: gradient buffers must be contiguous float32 tensors of the bias's shape (d,)")
    workspace = _workspace_arg("ngcf_layer_bwd", workspace, ngcf_workspace, x.shape[0], x.shape[1], x.device)
    _lib.check(_lib.lib().crh_ngcf_layer_bwd_f32(_lib.ptr(x), _lib.ptr(s), _lib.ptr(xk), _lib.ptr(g), _lib.ptr(dout), float(c),
                                                 _lib.ptr(w), x.shape[0], x.shape[1], _lib.ptr(ds), _lib.ptr(local),
                                                 _lib.ptr(dw), _lib.ptr(db), _lib.ptr(workspace), workspace.numel(),
                                                 _lib.current_stream()), "crh_ngcf_layer_bwd_f32")
    return ds, local, dw, db


# ---- SimGCL / XSimGCL layer perturbation (perturb.hip) ---------------------------------------------------------------

def _perturb_checks(what: str, y: torch.Tensor, *others) -> None:
    _need_cuda(y, *others)
    if y.dtype != torch.float32 or not y.is_contiguous() or y.dim() != 2:
        raise RuntimeError(f"{what}: the rows must be a contiguous 2-D float32 tensor")
    for t in others:
        if t is None:
            continue
        if t.device != y.device:
            raise RuntimeError(f"{what}: every tensor must be on the rows' device")
        if t.dtype == torch.int64:
            if t.numel() < 1:
                raise RuntimeError(f"{what}: draw_dev must be a device int64 scalar")
        elif t.dtype != torch.float32 or not t.is_contiguous() or t.shape != y.shape:
            raise RuntimeError(f"{what}: noise and accumulators must be contiguous float32 tensors of the rows' shape")


def noise_uniform(n_rows: int, d: int, seed: int, draw: int = 0, draw_dev: Optional[torch.Tensor] = None,
                  out: Optional[torch.Tensor] = None, device=None) -> torch.Tensor:
    """The (n_rows, d) uniforms in [0, 1) that ``perturb_rows(noise=None)`` generates in registers for the same
    (seed, draw): Philox4x32-10, see crh_noise_uniform_f32.  ``draw_dev``: optional device int64 added to ``draw``."""
    if out is None:
        out = torch.empty((int(n_rows), int(d)), dtype=torch.float32, device=device if device is not None else
                          (draw_dev.device if draw_dev is not None else 'cuda'))
    _perturb_checks("noise_uniform", out, draw_dev)
    if draw_dev is not None and draw_dev.dtype != torch.int64:
        raise RuntimeError("noise_uniform: draw_dev must be a device int64 scalar")
    _lib.check(_lib.lib().crh_noise_uniform_f32(_lib.ptr(out), out.shape[0], out.shape[1], int(seed) & (2 ** 64 - 1),
                                                _lib.ptr(draw_dev), int(draw), _lib.current_stream()),
               "crh_noise_uniform_f32")
    return out


def perturb_rows(y: torch.Tensor, eps: float, noise: Optional[torch.Tensor] = None, seed: int = 0, draw: int = 0,
                 draw_dev: Optional[torch.Tensor] = None, acc_in: Optional[torch.Tensor] = None, s_in: float = 1.0,
                 acc_out: Optional[torch.Tensor] = None, s_out: float = 1.0) -> torch.Tensor:
    """y += sign(y) * normalize(r, dim=-1) * eps in place (model/SimGCL.py:106-108); acc_out = (acc_in*s_in + y)*s_out.
    r = ``noise`` (an (n_rows, d) buffer of uniforms) or, without it, the Philox stream of (seed, draw [+ *draw_dev])."""
    _perturb_checks("perturb_rows", y, noise, acc_in, acc_out, draw_dev)
    if draw_dev is not None and draw_dev.dtype != torch.int64:
        raise RuntimeError("perturb_rows: draw_dev must be a device int64 scalar")
    _lib.check(_lib.lib().crh_perturb_rows_f32(_lib.ptr(y), y.shape[0], y.shape[1], float(eps), _lib.ptr(noise),
                                               int(seed) & (2 ** 64 - 1), _lib.ptr(draw_dev), int(draw), _lib.ptr(acc_in),
                                               float(s_in), _lib.ptr(acc_out), float(s_out), _lib.current_stream()),
               "crh_perturb_rows_f32")
    return y
