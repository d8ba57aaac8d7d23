"""The host model of the SpMM's heavy rows (oracle/spmm_model.py) checked on its own, without a GPU: the chunking covers a
row, the modelled sum tree is a valid fp32 evaluation of the row (a derived bound against fp64), it collapses to the oracle's
single chain where every order is exact, and it is NOT the single chain on ordinary inputs -- so the bitwise GPU tests of
tests/test_spmm_edges_gpu.py pin something the chain tests do not."""
import math

import numpy as np
import pytest

from oracle import oracle_np as orc
from oracle import spmm_model as sm

U32 = 2.0 ** -24                       # unit roundoff of fp32
GGS = sm.LANE_GROUPS


def row_lengths(GG):
    """lengths around every place the chunking changes: one edge, one chunk, the first and second step of the chunk length
    (8 NGB m + {-1, 0, 1}), a row that leaves trailing lane groups (at GG = 64: the whole last wave) empty"""
    ngb = 256 // GG
    return sorted({1, 7, 8, 9, 64, 65, 8 * ngb - 1, 8 * ngb, 8 * ngb + 1, 16 * ngb - 1, 16 * ngb, 16 * ngb + 1, 2049})


def one_row(rng, length, d, n=4200, grid=None):
    col = np.sort(rng.choice(n, length, replace=False)).astype(np.int32)
    if grid is None:
        val = rng.standard_normal(length).astype(np.float32)
        X = rng.standard_normal((n, d)).astype(np.float32)
        val[rng.random(length) < 0.1] *= np.float32(1e-4)
    else:
        val = (rng.integers(-2 * grid, 2 * grid + 1, length) / grid).astype(np.float32)
        X = (rng.integers(-2 * grid, 2 * grid + 1, (n, d)) / grid).astype(np.float32)
    return np.array([0, length], np.int64), col, val, X


def test_lanes_for_is_the_kernels_dispatch():
    """spmm_body: n_sub == 4 and G >= 4 -> G / 4; n_sub == 2 and G >= 2 -> G / 2; otherwise the whole lane group"""
    for G in GGS:
        assert sm.lanes_for(G, 1) == G
        assert sm.lanes_for(G, 2) == (G // 2 if G >= 2 else G)
        assert sm.lanes_for(G, 4) == (G // 4 if G >= 4 else G)
    assert sm.lanes_for(2, 4) == 2 and sm.lanes_for(1, 2) == 1 and sm.lanes_for(1, 4) == 1
    assert {sm.lanes_for(G, s) for G in GGS for s in (1, 2, 4)} == set(GGS)


@pytest.mark.parametrize("GG", GGS)
def test_chunks_cover_every_edge_once_in_order(GG):
    ngb = 256 // GG
    for length in row_lengths(GG) + list(range(1, 300, 13)):
        off = sm.chunk_offsets(length, GG)
        chunk = sm.chunk_len(length, GG)
        assert len(off) == ngb + 1 and off[0] == 0 and off[-1] == length and (np.diff(off) >= 0).all()
        assert chunk % 8 == 0 and chunk * ngb >= length and (chunk - 8) * ngb < length
        owned = np.concatenate([np.arange(off[g], off[g + 1]) for g in range(ngb)])
        assert np.array_equal(owned, np.arange(length))                       # every edge once, ascending
        sizes = np.diff(off)
        active = int(math.ceil(length / chunk))
        assert (sizes[:active - 1] == chunk).all() and sizes[active - 1] == length - (active - 1) * chunk
        assert (sizes[active:] == 0).all()
    # the edge cases the GPU file relies on
    if ngb >= 16:
        assert (np.diff(sm.chunk_offsets(65, GG)) > 0).sum() == 9 and np.diff(sm.chunk_offsets(65, GG))[8] == 1
    if GG == 64:
        assert np.diff(sm.chunk_offsets(65, GG)).tolist() == [24, 24, 17, 0]  # wave 3 owns nothing


@pytest.mark.parametrize("GG", GGS)
def test_model_is_within_the_derived_bound_of_fp64(GG):
    """Bound.  A product v_e x_e enters the result through: the fmaf chain of its lane group, in which it is part of at most
    `chunk` rounded results (one rounding per fmaf, the product itself is not rounded); then log2(64 / GG) shuffle additions
    and 2 additions across the waves, one rounding each.  With h = chunk + log2(64 / GG) + 2 roundings of relative size
    <= u = 2^-24 on its way, the standard recursive-summation argument (Higham, Accuracy and Stability, section 4.2: every
    term is multiplied by at most h factors (1 + delta), |delta| <= u) gives

        |model - exact| <= gamma_h * sum_e |v_e x_e|,   gamma_h = h u / (1 - h u).

    The exact sum is taken in fp64: products of two fp32 numbers are exact there and the fp64 accumulation adds at most
    len * 2^-53 * sum |v x|, which is added to the bound."""
    rng = np.random.default_rng(100 + GG)
    d = 8
    for length in row_lengths(GG):
        rowptr, col, val, X = one_row(rng, length, d)
        got = sm.heavy_row(rowptr, col, val, X, 0, GG).astype(np.float64)
        prod = val.astype(np.float64)[:, None] * X.astype(np.float64)[col]
        exact, mag = prod.sum(0), np.abs(prod).sum(0)
        h = sm.chunk_len(length, GG) + int(math.log2(64 // GG)) + 2
        gamma = h * U32 / (1.0 - h * U32)
        assert (np.abs(got - exact) <= (gamma + length * 2.0 ** -53) * mag).all(), (GG, length)


@pytest.mark.parametrize("GG", GGS)
def test_model_equals_chain_where_every_order_is_exact(GG):
    """val and X on a 2^-4 grid in [-2, 2]: products are multiples of 2^-8 of at most 4, and any partial sum of up to 4 097
    of them stays below 2^15: 15 integer and 8 fraction bits, within fp32's 24 -- every association is exact, so tree and
    chain must agree bit for bit (a model that dropped, doubled or misplaced an edge would not)."""
    rng = np.random.default_rng(200 + GG)
    for length in row_lengths(GG):
        rowptr, col, val, X = one_row(rng, length, 8, grid=16)
        tree = sm.heavy_row(rowptr, col, val, X, 0, GG)
        chain = orc.spmm(rowptr, col, val, X)[0]
        assert np.array_equal(tree.view(np.int32), chain.view(np.int32)), (GG, length)
        assert np.array_equal(chain.astype(np.float64), (val.astype(np.float64)[:, None] * X.astype(np.float64)[col]).sum(0))


def test_model_is_not_the_chain_and_depends_on_the_lane_group():
    """On N(0, 1) inputs a 2 049-edge row's tree differs from the single chain in most of 64 columns, and the trees of two
    lane-group widths differ from each other: a bitwise comparison with the model tells a wrong GG from the right one."""
    rng = np.random.default_rng(7)
    rowptr, col, val, X = one_row(rng, 2049, 64)
    chain = orc.spmm(rowptr, col, val, X)[0]
    trees = {GG: sm.heavy_row(rowptr, col, val, X, 0, GG) for GG in GGS}
    for GG, tree in trees.items():
        assert (tree.view(np.int32) != chain.view(np.int32)).sum() >= 32, GG
    for a in GGS:
        for b in GGS:
            if a < b:
                assert (trees[a].view(np.int32) != trees[b].view(np.int32)).sum() >= 16, (a, b)


def test_fold_is_the_documented_tree():
    """fold() on partials whose sums are order-sensitive, against the tree written out by hand for GG = 16 (4 groups per
    wave): ((g0 + g1) + (g2 + g3)) per wave, then (w0 + w1) + (w2 + w3)."""
    rng = np.random.default_rng(3)
    p = (rng.standard_normal((16, 64)) * 10.0 ** rng.integers(-3, 4, (16, 64))).astype(np.float32)
    w = [(p[4 * k] + p[4 * k + 1]) + (p[4 * k + 2] + p[4 * k + 3]) for k in range(4)]
    want = (w[0] + w[1]) + (w[2] + w[3])
    assert np.array_equal(sm.fold(p).view(np.int32), want.view(np.int32))
    assert sm.fold(p).dtype == np.float32
    left_to_right = ((w[0] + w[1]) + w[2]) + w[3]
    assert not np.array_equal(left_to_right.view(np.int32), want.view(np.int32))   # the data can tell the orders apart


def test_spmm_scheduled_uses_the_chain_up_to_seg_and_the_tree_above():
    rng = np.random.default_rng(5)
    deg = np.array([0, 3, 64, 65, 96, 97, 384, 385, 12])
    n, d = 600, 12
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    col = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in deg]).astype(np.int32)
    val = rng.standard_normal(len(col)).astype(np.float32)
    X = rng.standard_normal((n, d)).astype(np.float32)
    n_sub = sm.n_sub_of_rows(len(deg), [7, 7, 7, 7, 6, 6, 5, 5, 4, 3], [4, 4 | 1 << 8, 4 | 2 << 8, 4 | 3 << 8, 2, 2 | 1 << 8, 2, 2 | 1 << 8, 1, 1])
    assert n_sub.tolist() == [1, 1, 1, 1, 1, 2, 2, 4, 1]
    Y = sm.spmm_scheduled(rowptr, col, val, X, 4, 64, n_sub)
    chain = orc.spmm(rowptr, col, val, X)
    light = deg <= 64
    assert np.array_equal(Y[light].view(np.int32), chain[light].view(np.int32))
    for row, GG in ((3, 4), (4, 4), (5, 2), (6, 2), (7, 1)):
        assert np.array_equal(Y[row].view(np.int32), sm.heavy_row(rowptr, col, val, X, row, GG).view(np.int32))
    Y256 = sm.spmm_scheduled(rowptr, col, val, X, 4, 256, n_sub)
    assert np.array_equal(Y256[:6].view(np.int32), chain[:6].view(np.int32))
    assert np.array_equal(Y256[6:8].view(np.int32), Y[6:8].view(np.int32))
