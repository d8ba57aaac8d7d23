"""Edges of the CSR SpMM (coldrec_amd/csrc/spmm.hip): every lane-group width of `heavy_row<GG>`, with and without the column
cuts of giant rows, at the row lengths where the chunking of a heavy row changes -- compared BIT FOR BIT with the host model
of the kernel's sum tree (oracle/spmm_model.py: fmaf chains per lane group, shuffle tree per wave, (w0 + w1) + (w2 + w3)
across the waves).  No tolerance occurs in this file: the heavy path is a fixed order, so it has one right answer.

Per case (a launch width G, a cut threshold GIANT, a segment length):
  * Y of the scheduled launch == spmm_model.spmm_scheduled on every row (light rows: the oracle's chain);
  * Y of the unscheduled launch == oracle_np.spmm;
  * where G = 8, the record-stream schedule gives the same bits beside the heavy rows;
  * acc_out == the light path's epilogue on the same operands (a second launch with A = I over the first launch's Y);
  * the optimiser epilogues (Adam, SGD, zero_acc_in) == the unfused sequence, bitwise;
  * every written table sits between sentinel guard rows that come back untouched, and a repeat gives the same bits.

Row lengths per case (`edge_degrees`): seg, seg + 1, GIANT, GIANT + 1, 4 GIANT, 4 GIANT + 1; per n_sub class, under its own
GG, the first 8 NGB m - 1 / 8 NGB m / 8 NGB m + 1 inside the class (the chunk length steps from 8 m to 8 (m + 1)), a length
that leaves trailing lane groups empty (at GG = 64: wave 3) and one whose last active group holds exactly one edge; filler
rows of 0 - 24 edges keep the mean degree below 48, so the schedule's segment length stays 64.  val and X are N(0, 1) with a
tenth of the edges scaled by 1e-4: a dropped small edge still flips bits."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import oracle_np as orc
from oracle import spmm_model as sm
from tests.test_train_edges_gpu import beq, bits, guarded, guards_intact

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CUT = 96                               # the patched SpmmSchedule.GIANT: 97 - 384 edges in two column ranges, above in four
MAX_DEG = 2100                         # longest row (the width-grid graphs have 2 600 columns)
S_IN, S_OUT = 0.3, 0.7                 # not powers of two: z * s_in rounds, so fusing it into an fma would change bits

# width grid: d -> lanes per lane group of the launch (crh_spmm_lane_group); d = 12 ... 200 are padded lane groups
WIDTHS = [(4, 1), (8, 2), (12, 4), (16, 4), (20, 8), (32, 8), (36, 16), (64, 16), (68, 32), (128, 32), (132, 64), (200, 64),
          (256, 64)]
GRID = [(2600, d, G, giant, None) for d, G in WIDTHS for giant in (0, CUT)] + [(2600, 64, 16, CUT, 256)]
# XCD column slices (2 or 4) with cuts: nnz <= 200 000 keeps the slices under the edge re-read rule
SLICED = [(7000, 128, 16, CUT, None), (13000, 128, 8, CUT, None), (13000, 64, 8, CUT, None), (26000, 64, 4, CUT, None),
          (26000, 32, 4, CUT, None)]
CASES = GRID + SLICED


def classes(seg, giant):
    """[(n_sub, lo, hi)]: the heavy row lengths lo .. hi (inclusive) cut into n_sub column ranges"""
    if giant <= 0:
        return [(1, seg + 1, MAX_DEG)]
    out = [(1, seg + 1, giant)] if seg < giant else []
    if seg < 4 * giant:
        out.append((2, max(seg, giant) + 1, 4 * giant))
    return out + [(4, max(seg, 4 * giant) + 1, MAX_DEG)]


def edge_degrees(G, seg, giant):
    degs = {seg, seg + 1, CUT, CUT + 1, 4 * CUT, 4 * CUT + 1, 700, 1100}
    for n_sub, lo, hi in classes(seg, giant):
        GG = sm.lanes_for(G, n_sub)
        ngb, step = 256 // GG, 8 * (256 // GG)
        first = step * math.ceil(lo / step)                            # where the chunk length steps
        if first <= hi:
            degs |= {L for L in (first - 1, first, first + 1) if L <= MAX_DEG}
        idle = next(L for L in range(lo, hi + 1) if math.ceil(L / sm.chunk_len(L, GG)) < ngb)
        single = next(L for L in range(lo, hi + 1) if L % sm.chunk_len(L, GG) == 1)
        degs |= {idle, single}
        if GG == 64:
            assert np.diff(sm.chunk_offsets(idle, GG))[3] == 0         # the whole of wave 3 owns nothing
    return sorted(degs)


@functools.lru_cache(maxsize=None)
def graph(n, G, seg, giant):
    """(rowptr, col, val) with the edge lengths of (G, seg, giant) at random rows among fillers of 0 - 24 edges (0 - 10 on
    the largest graphs: nnz <= 200 000); columns distinct and ascending within a row"""
    rng = np.random.default_rng(1000 * G + giant + seg + n)
    special = np.array(edge_degrees(G, seg, giant))
    deg = np.concatenate([special, rng.integers(0, 25 if n <= 13000 else 11, n - len(special))])
    deg = deg[rng.permutation(n)].astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    nnz = int(rowptr[-1])
    assert nnz <= 200_000 and deg.mean() < 48
    # k distinct ascending columns of a row: k sorted draws from [0, n - k] plus 0 .. k - 1
    row_of = np.repeat(np.arange(n), deg)
    k_of = np.repeat(deg, deg)
    draw = (rng.random(nnz) * (n - k_of + 1)).astype(np.int64)
    draw = draw[np.lexsort((draw, row_of))]
    col = (draw + np.arange(nnz) - np.repeat(rowptr[:-1], deg)).astype(np.int32)
    assert col.min() >= 0 and col.max() < n
    val = rng.standard_normal(nnz).astype(np.float32)
    val[rng.random(nnz) < 0.1] *= np.float32(1e-4)
    for a in (rowptr, col, val):
        a.setflags(write=False)
    return rowptr, col, val


@functools.lru_cache(maxsize=4)
def operands(n, d, G, seg, giant):
    """host operands of one case and the two references that do not depend on the schedule"""
    rowptr, col, val = graph(n, G, seg, giant)
    rng = np.random.default_rng(d * 131 + giant + n)
    X = rng.standard_normal((n, d)).astype(np.float32)
    X[rng.random(n) < 0.1] *= np.float32(1e-4)
    Z = rng.standard_normal((n, d)).astype(np.float32)
    chain = orc.spmm(rowptr, col, val, X)
    for a in (X, Z, chain):
        a.setflags(write=False)
    return rowptr, col, val, X, Z, chain


def t(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the cached host arrays are read-only)


def ibits(a):
    return np.ascontiguousarray(a).view(np.int32)


def setup(monkeypatch, n, d, G, giant, seg):
    """schedule of the case under the patched cut threshold; returns its pieces and the set of heavy_row<GG> it launches"""
    from coldrec_amd import _lib, ops
    monkeypatch.setattr(ops.SpmmSchedule, "GIANT", giant)
    rowptr, col, val, X, Z, chain = operands(n, d, G, seg or 64, giant)
    assert int(_lib.lib().crh_spmm_lane_group(n, d, int(rowptr[-1]))) == G    # a changed heuristic fails here, loudly
    sched = ops.SpmmSchedule(rowptr, DEV, seg=seg)
    assert sched.seg == (seg or 64)
    n_sub = sm.n_sub_of_rows(n, sched.t[3].cpu().numpy(), sched.t[5].cpu().numpy())
    deg = np.diff(rowptr)
    heavy = np.nonzero(deg > sched.seg)[0]
    ggs = {sm.lanes_for(G, int(n_sub[r])) for r in heavy}
    assert ggs == {sm.lanes_for(G, s) for s, _, _ in classes(sched.seg, giant)}
    assert all(int(n_sub[r]) == next(s for s, lo, hi in classes(sched.seg, giant) if lo <= deg[r] <= hi) for r in heavy)
    return ops, sched, n_sub, ggs, (rowptr, col, val, X, Z, chain)


def case_id(c):
    n, d, G, giant, seg = c
    return "n%d-d%d-G%d-giant%d%s" % (n, d, G, giant, "-seg%d" % seg if seg else "")


def test_width_grid_launches_every_heavy_row_instantiation(monkeypatch):
    """the union of GG over the width grid is 1 ... 64 -- the narrow loop (GG < 8: 8 / GG entries per lane) and the wide one"""
    launched = {}
    for n, d, G, giant, seg in GRID:
        _, _, _, ggs, _ = setup(monkeypatch, n, d, G, giant, seg)
        for GG in ggs:
            launched.setdefault(GG, []).append((d, giant))
    print("heavy_row<GG> launched by (d, GIANT):", {k: launched[k] for k in sorted(launched)})
    assert set(launched) == {1, 2, 4, 8, 16, 32, 64}
    # padded lane groups under cuts whose last column range is partly (d = 200: float4 columns 48, 49 of 48 .. 63) or
    # wholly (d = 12: sub 3 of 3 columns; d = 132: sub 3 = columns 48 .. 63 of 33) idle
    for d in (12, 20, 36, 68, 132, 200):
        assert any(dd == d and g == CUT for v in launched.values() for dd, g in v)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_heavy_rows_equal_the_sum_tree_model(monkeypatch, case):
    n, d, G, giant, seg = case
    ops, sched, n_sub, _, (rowptr, col, val, X, Z, chain) = setup(monkeypatch, n, d, G, giant, seg)
    want = sm.spmm_scheduled(rowptr, col, val, X, G, sched.seg, n_sub)
    deg = np.diff(rowptr)
    heavy = deg > sched.seg
    assert (ibits(want[heavy]) != ibits(chain[heavy])).any()                  # the tree is not the chain on this data
    rp, cl, vl, tX, tZ = t(rowptr), t(col), t(val), t(X), t(Z)
    # unscheduled: a lane group per row, the oracle's chain on every row
    yb0, Y0 = guarded(n, d)
    ops.spmm_csr(rp, cl, vl, tX, y=Y0)
    assert np.array_equal(ibits(Y0.cpu().numpy()), ibits(chain)) and guards_intact(yb0)
    # scheduled: light rows the chain, heavy rows the tree under their own GG
    yb, Y = guarded(n, d)
    ab, A = guarded(n, d)
    ops.spmm_csr(rp, cl, vl, tX, y=Y, acc_in=tZ, s_in=S_IN, acc_out=A, s_out=S_OUT, sched=sched)
    got = Y.cpu().numpy()
    bad = np.nonzero((ibits(got) != ibits(want)).any(1))[0]
    assert len(bad) == 0, [(int(r), int(deg[r]), int(n_sub[r])) for r in bad[:8]]
    assert guards_intact(yb) and guards_intact(ab) and beq(tZ, t(Z))
    yb2, Y2 = guarded(n, d)
    ab2, A2 = guarded(n, d)
    ops.spmm_csr(rp, cl, vl, tX, y=Y2, acc_in=tZ, s_in=S_IN, acc_out=A2, s_out=S_OUT, sched=sched)
    assert beq(Y, Y2) and beq(A, A2) and guards_intact(yb2) and guards_intact(ab2)
    # acc_out without assuming how (z s_in + P) s_out is contracted: A = I over the first launch's Y makes the LIGHT path
    # apply the same epilogue to the same operands (fmaf(1, y, +0) = y)
    eye = (torch.arange(n + 1, dtype=torch.int64, device=DEV), torch.arange(n, dtype=torch.int32, device=DEV),
           torch.ones(n, dtype=torch.float32, device=DEV))
    ab3, A3 = guarded(n, d)
    yb3, Y3 = guarded(n, d)
    ops.spmm_csr(*eye, Y, y=Y3, acc_in=tZ, s_in=S_IN, acc_out=A3, s_out=S_OUT)
    assert beq(Y3, Y) and beq(A3, A) and guards_intact(ab3) and guards_intact(yb3)
    if G == 8:
        # the record stream carries the light rows beside the heavy workgroups
        slab = ops.SpmmSchedule(rowptr, DEV, seg=seg, col=col, val=val)
        assert slab.for_launch(n, d, cl, vl).slab and slab.for_launch(n, d).slab_lanes == 8
        yb4, Y4 = guarded(n, d)
        ab4, A4 = guarded(n, d)
        ops.spmm_csr(rp, cl, vl, tX, y=Y4, acc_in=tZ, s_in=S_IN, acc_out=A4, s_out=S_OUT, sched=slab)
        assert beq(Y4, Y) and beq(A4, A) and guards_intact(yb4) and guards_intact(ab4)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_optimiser_epilogues_on_heavy_rows(monkeypatch, case):
    """crh_spmm_csr_adam_f32 / _sgd_f32 with zero_acc_in == crh_spmm_csr_f32(acc_out = g) + crh_adam_dense_f32 /
    crh_sgd_dense_f32, bit for bit on p, m, v and g, with acc_in cleared -- the identity of test_spmm_adam_epilogue_ops_level
    and test_spmm_sgd_epilogue_ops_level at every lane-group width and cut"""
    n, d, G, giant, seg = case
    ops, sched, n_sub, _, (rowptr, col, val, X, Z, chain) = setup(monkeypatch, n, d, G, giant, seg)
    rng = np.random.default_rng(d + giant)
    rp, cl, vl, tX, tZ = t(rowptr), t(col), t(val), t(X), t(Z)
    p0 = t((rng.standard_normal((n, d)) * 0.1).astype(np.float32))
    m0 = t((rng.standard_normal((n, d)) * 1e-3).astype(np.float32))
    v0 = t((rng.random((n, d)) * 1e-5).astype(np.float32))
    scheds = [sched] + ([ops.SpmmSchedule(rowptr, DEV, seg=seg, col=col, val=val)] if G == 8 else [])
    for sc in scheds:
        g = torch.empty_like(tX)
        ops.spmm_csr(rp, cl, vl, tX, acc_in=tZ, s_in=S_IN, acc_out=g, s_out=S_OUT, sched=sc)
        # Adam
        p1, m1, v1 = p0.clone(), m0.clone(), v0.clone()
        ops.adam_dense(p1, g.clone(), m1, v1, 7, lr=1e-2, zero_grad=False)
        bufs = [guarded(n, d) for _ in range(5)]
        (pb, p2), (mb, m2), (vb, v2), (zb, z2), (gb, g2) = bufs
        p2.copy_(p0), m2.copy_(m0), v2.copy_(v0), z2.copy_(tZ)
        ops.spmm_csr_adam(rp, cl, vl, tX, z2, S_IN, g2, S_OUT, sc, p2, m2, v2, 7, lr=1e-2, zero_acc_in=True)
        assert beq(g, g2) and beq(p1, p2) and beq(m1, m2) and beq(v1, v2)
        assert not bool(bits(z2).any()) and all(guards_intact(b) for b, _ in bufs)
        assert not beq(p1, p0)
        # SGD
        q1 = p0.clone()
        ops.sgd_dense(q1, g.clone(), 0.037, zero_grad=False)
        bufs = [guarded(n, d) for _ in range(3)]
        (qb, q2), (zb, z3), (gb, g3) = bufs
        q2.copy_(p0), z3.copy_(tZ)
        ops.spmm_csr_sgd(rp, cl, vl, tX, z3, S_IN, g3, S_OUT, sc, q2, 0.037, zero_acc_in=True)
        assert beq(g, g3) and beq(q1, q2) and not bool(bits(z3).any()) and all(guards_intact(b) for b, _ in bufs)
        assert not beq(q1, p0)
