"""OWNER MODEL -- TEST INFRASTRUCTURE ONLY (numpy restatement of the sum tree of loss_common.h's owner pass).

Written from ``lg_owner_chunk_kernel``, ``lg_owner_finish_kernel``, ``lg_cross_sum`` and ``lg_dispatch_lpr`` of
``coldrec_amd/csrc/loss_common.h``; nothing under ``coldrec_amd/`` may import it.  One side of a plan groups the
occurrences by owner (``ptr``, ``occ``) and cuts every owner's run into chunks of at most ``chunk`` occurrences
(``chunk_ptr``, ``chunk_own``); occurrence o owns row o of ``rows``.  An owner's row is summed like this:

  * a wave of 64 lanes holds RG = 64 / LPR lane groups of LPR = pow2(d / 4) lanes; one wave sums one chunk.  The chunk is
    walked in windows of 64 occurrences; in a window, lane group ``grp`` adds to its accumulator (from +0) the rows of the
    window's occurrences ``j * RG + grp`` for j = 0 .. LPR - 1, in that order, skipping those past the chunk's end; the
    next window goes on in the same accumulator;
  * the RG accumulators meet in an xor butterfly, ``v[g] += v[g ^ s]`` for s = RG / 2, RG / 4, .. 1 (``__shfl_xor`` by
    s * LPR lanes), every group adding at every step; group 0's value is the chunk's partial;
  * the finish adds an owner's partials from +0 in chunk order.

The columns are independent, so the model takes all d of them at once; the lanes of a group with ``col >= d`` hold no
column and do not enter it.  Only fp32 additions occur, each correctly rounded in numpy as on the GPU, so the model's row
is the one fp32 value the kernel's fixed order can give, and tests compare bits.
"""
from __future__ import annotations

import numpy as np

WAVE = 64
LANE_GROUPS = (1, 2, 4, 8, 16, 32, 64)


def lpr_for(d: int) -> int:
    """Lanes per row at width d: the least power of two that holds d / 4 lanes (``lg_dispatch_lpr``)."""
    d = int(d)
    assert d >= 4 and d % 4 == 0 and d <= 4 * WAVE
    return 1 << (d // 4 - 1).bit_length()


def chunk_bounds(ptr, chunk_ptr, chunk_own, chunk: int):
    """(k_begin, k_end) of every chunk: k_begin = ptr[s] + (ch - chunk_ptr[s]) * chunk, k_end clamped to ptr[s + 1]."""
    ptr, chunk_ptr, own = (np.asarray(t, np.int64) for t in (ptr, chunk_ptr, chunk_own))
    ch = np.arange(own.shape[0], dtype=np.int64)
    begin = ptr[own] + (ch - chunk_ptr[own]) * int(chunk)
    return begin, np.minimum(begin + int(chunk), ptr[own + 1])


def butterfly(acc: np.ndarray) -> np.ndarray:
    """``lg_cross_sum`` over the groups: (.., RG, d) -> the same shape, every group holding the sum."""
    acc = np.ascontiguousarray(acc, np.float32)
    rg = acc.shape[-2]
    assert rg & (rg - 1) == 0
    s = rg // 2
    while s >= 1:
        acc = acc + acc[..., np.arange(rg) ^ s, :]
        s //= 2
    return acc


def chunk_partials(ptr, occ, chunk_ptr, chunk_own, d: int, rows, chunk: int = 256) -> np.ndarray:
    """(n_chunks, d): what ``lg_owner_chunk_kernel`` leaves in ``part`` (the sums; not the count of a COUNT_FIRST pass)."""
    rows = np.ascontiguousarray(rows, np.float32)
    occ = np.asarray(occ, np.int64)
    assert rows.ndim == 2 and rows.shape[1] == int(d) and int(chunk) % WAVE == 0
    lpr = lpr_for(d)
    rg = WAVE // lpr
    begin, end = chunk_bounds(ptr, chunk_ptr, chunk_own, chunk)
    acc = np.zeros((begin.shape[0], rg, int(d)), np.float32)
    grp = np.arange(rg, dtype=np.int64)
    for k0 in range(0, int(chunk), WAVE):                 # the windows of a chunk
        for j in range(lpr):
            k = begin[:, None] + k0 + j * rg + grp[None, :]          # (chunks, RG): the occurrence slot each group reads
            have = k < end[:, None]
            if not have.any():
                continue
            o = occ[np.where(have, k, 0)]
            acc[have] = acc[have] + rows[o[have]]
    return butterfly(acc)[:, 0]


def owner_sums(ptr, occ, chunk_ptr, chunk_own, d: int, rows, chunk: int = 256) -> np.ndarray:
    """(n_owners, d): every owner's rows summed in the owner pass's order (``LgFinishSum``'s output)."""
    part = chunk_partials(ptr, occ, chunk_ptr, chunk_own, d, rows, chunk)
    chunk_ptr = np.asarray(chunk_ptr, np.int64)
    out = np.zeros((chunk_ptr.shape[0] - 1, int(d)), np.float32)
    per = np.diff(chunk_ptr)
    for c in range(int(per.max()) if per.size else 0):    # the c-th chunk of every owner that has one
        live = per > c
        out[live] = out[live] + part[chunk_ptr[:-1][live] + c]
    return out


def first_counts(ptr, occ, first: int) -> np.ndarray:
    """(n_owners,): an owner's occurrences below ``first`` -- what a COUNT_FIRST pass carries through the partials."""
    ptr, occ = np.asarray(ptr, np.int64), np.asarray(occ, np.int64)
    below = np.concatenate([[0], np.cumsum(occ < int(first))])
    return below[ptr[1:]] - below[ptr[:-1]]


def chain_sums(ptr, occ, rows) -> np.ndarray:
    """(n_owners, d): the plain left-to-right fp32 chain over an owner's occurrences -- what the pass is NOT."""
    rows = np.ascontiguousarray(rows, np.float32)
    ptr, occ = np.asarray(ptr, np.int64), np.asarray(occ, np.int64)
    out = np.zeros((ptr.shape[0] - 1, rows.shape[1]), np.float32)
    for s in range(out.shape[0]):
        acc = np.zeros(rows.shape[1], np.float32)
        for o in occ[ptr[s]:ptr[s + 1]]:
            acc = acc + rows[o]
        out[s] = acc
    return out
