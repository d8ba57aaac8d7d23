"""SPMM MODEL -- TEST INFRASTRUCTURE ONLY (numpy / C restatement of the sum tree of spmm.hip's heavy rows).

Written from the header comment and ``heavy_row<GG>`` / ``spmm_body`` of ``coldrec_amd/csrc/spmm.hip``; nothing under
``coldrec_amd/`` may import it.  A row with more than ``seg`` edges is summed by a whole workgroup of 256 lanes:

  * the 256 / GG lane groups of GG lanes cut the row's edge list into contiguous chunks of
    ``chunk = ceil(len / NGB)`` rounded up to a multiple of 8 edges; group g owns edges [g chunk, (g + 1) chunk) of the row,
    as far as the row goes (trailing groups may own nothing);
  * each group runs the oracle's edge-order ``fmaf`` chain from +0 over its chunk (an empty chunk leaves +0);
  * inside a wave the 64 / GG partial sums are folded by ``t[j] += t[j + 2^m]``, m = 0, 1, ... (``__shfl_down`` by GG, 2 GG,
    ... as read by the lanes below GG): a balanced tree over neighbouring groups;
  * the four waves meet in LDS as ``(w0 + w1) + (w2 + w3)``.

GG is the launch's lane-group width G for an uncut row and G / n_sub for a row cut into n_sub column ranges (``lanes_for``).
The feature columns are independent, so the model takes all d of them at once and the column ranges, the XCD column slices
and the padded lanes of a lane group do not enter it.

The chains are the C oracle's real ``fmaf`` (``oracle_np.spmm`` on a ``rowptr`` of absolute chunk offsets: one "row" per
lane group), never an fp64 emulation, which would round twice; the folds are numpy fp32 additions, each correctly rounded.
So the model's value of a heavy row is the one fp32 number the kernel's fixed order can give, and tests compare bits.
"""
from __future__ import annotations

import numpy as np

from oracle import oracle_np as orc

WG = 256          # lanes of a workgroup
WAVE = 64
LANE_GROUPS = (1, 2, 4, 8, 16, 32, 64)


def lanes_for(G: int, n_sub: int) -> int:
    """Lanes per lane group of a heavy row cut into ``n_sub`` column ranges at launch width G (the dispatch at the end of
    ``spmm_body``): G / n_sub; a cut wider than the lane group falls back to the whole group (only sub 0 works)."""
    G, n_sub = int(G), int(n_sub)
    assert G in LANE_GROUPS and n_sub in (1, 2, 4)
    return G // n_sub if G >= n_sub else G


def chunk_len(length: int, GG: int) -> int:
    """Edges per lane group of a row of ``length`` edges: ceil(length / NGB) rounded up to a multiple of 8."""
    ngb = WG // GG
    chunk = (int(length) + ngb - 1) // ngb
    return (chunk + 7) & ~7


def chunk_offsets(length: int, GG: int) -> np.ndarray:
    """NGB + 1 offsets into a row of ``length`` edges: group g owns [off[g], off[g + 1]) (empty once the row has ended)."""
    assert GG in LANE_GROUPS
    ngb = WG // GG
    return np.minimum(np.arange(ngb + 1, dtype=np.int64) * chunk_len(length, GG), int(length))


def fold(partials: np.ndarray) -> np.ndarray:
    """The combine of ``heavy_row``: (NGB, d) fp32 partial sums in lane-group order -> (d,) row."""
    t = np.ascontiguousarray(partials, np.float32)
    ngb, d = t.shape
    per_wave = ngb // 4                                   # 64 / GG lane groups in each of the 4 waves
    assert per_wave * 4 == ngb and per_wave & (per_wave - 1) == 0
    t = t.reshape(4, per_wave, d).copy()
    step = 1
    while step < per_wave:                                # __shfl_down by GG * step: every lane adds, lanes below GG are read
        nxt = t.copy()
        nxt[:, :per_wave - step] = t[:, :per_wave - step] + t[:, step:]
        t, step = nxt, step * 2
    w = t[:, 0]
    return (w[0] + w[1]) + (w[2] + w[3])


def heavy_partials(rowptr, col, val, X, row: int, GG: int) -> np.ndarray:
    """(NGB, d): the fmaf chain of every lane group of ``row`` over its chunk, from +0."""
    r0, r1 = int(rowptr[row]), int(rowptr[row + 1])
    return orc.spmm(r0 + chunk_offsets(r1 - r0, GG), col, val, X)


def heavy_row(rowptr, col, val, X, row: int, GG: int) -> np.ndarray:
    """Row ``row`` of A @ X as ``heavy_row<GG>`` sums it, all d columns."""
    return fold(heavy_partials(rowptr, col, val, X, row, GG))


def spmm_scheduled(rowptr, col, val, X, G: int, seg: int, n_sub_of_row) -> np.ndarray:
    """A @ X as a scheduled launch of lane-group width G gives it: rows of at most ``seg`` edges are the oracle's single
    chain, the others ``heavy_row`` under ``lanes_for(G, n_sub_of_row[row])`` (``n_sub_of_row``: one entry per row of A,
    read at the heavy rows only)."""
    rowptr = np.asarray(rowptr, np.int64)
    Y = orc.spmm(rowptr, col, val, X)
    for row in np.nonzero(np.diff(rowptr) > int(seg))[0]:
        Y[row] = heavy_row(rowptr, col, val, X, int(row), lanes_for(G, int(n_sub_of_row[row])))
    return Y


def n_sub_of_rows(n_rows: int, multi_row, multi_count) -> np.ndarray:
    """Per-row cut count from a schedule's heavy-block list (``multi_count`` = n_sub | sub << 8; 1 where not listed)."""
    out = np.ones(int(n_rows), np.int64)
    out[np.asarray(multi_row, np.int64)] = np.asarray(multi_count, np.int64) & 255
    return out
