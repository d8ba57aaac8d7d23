"""The host model of the fused losses' owner pass (oracle/owner_model.py) checked on its own, without a GPU: its dispatch
is lg_dispatch_lpr's, it adds every occurrence exactly once, its sum tree is a valid fp32 evaluation of an owner's row (a
derived bound against fp64), and it is NOT the plain left-to-right chain on ordinary inputs -- so the bitwise GPU test of
tests/test_owner_pass_gpu.py pins something a chain would not.  The profile batch of tests/owner_cases.py is checked here
too: every size present on both sides, the widths reaching all seven lane-group widths."""
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import owner_model as om
from tests import owner_cases as oc

U32 = 2.0 ** -24                       # unit roundoff of fp32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = oc.CHUNK


def plan_of(sizes, chunk=CHUNK, seed=0):
    """One side of a plan for owners of ``sizes`` occurrences, shuffled: (ptr, occ, chunk_ptr, chunk_own, owner of each
    occurrence), through the package's own grouping."""
    from coldrec_amd import ops
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    _uniq, order, ptr, chunk_ptr, chunk_own, _inv = (t.numpy() for t in ops._owner_chunks(torch.from_numpy(ids), chunk))
    return ptr, order, chunk_ptr, chunk_own, ids


def test_dispatch_is_the_kernels():
    """lg_dispatch_lpr's ladder, read from the header: `lanes <= n` -> LPR n for n = 1 .. 32, else 64."""
    text = open(os.path.join(ROOT, "coldrec_amd", "csrc", "loss_common.h")).read()
    body = text[text.index("inline void lg_dispatch_lpr"):]
    body = body[:body.index("\n}")]
    ladder = [(int(a), int(b)) for a, b in re.findall(r"lanes <= (\d+)\) f\(std::integral_constant<int, (\d+)>", body)]
    last = re.findall(r"else f\(std::integral_constant<int, (\d+)>", body)
    assert ladder == [(n, n) for n in (1, 2, 4, 8, 16, 32)] and last == ["64"] and "const int lanes = d / 4;" in body
    for d in range(4, 257, 4):
        want = next((lpr for top, lpr in ladder if d // 4 <= top), int(last[0]))
        assert om.lpr_for(d) == want, d
    assert {om.lpr_for(d) for d in oc.WIDTHS} == set(om.LANE_GROUPS)
    assert {om.lpr_for(w) for d in oc.MTPR_WIDTHS for w in (d, 2 * d)} == set(om.LANE_GROUPS)
    # each lane-group width at a width that fills it and, from 4 lanes up, at one that leaves lanes without a column
    for lpr in om.LANE_GROUPS:
        mine = [d for d in oc.WIDTHS if om.lpr_for(d) == lpr]
        assert 4 * lpr in mine and (lpr < 4 or any(d < 4 * lpr for d in mine)), lpr
    assert int(re.search(r"constexpr int LG_CHUNK = (\d+);", text).group(1)) == CHUNK


def test_profile_batch_holds_every_size_on_both_sides():
    from coldrec_amd import ops
    users, pos, neg = oc.profile_ids()
    plan = ops.vbpr_plan(users, pos, neg, chunk=CHUNK)
    assert sorted(oc.owner_sizes(plan, "user")) == sorted(oc.SIZES)
    assert sorted(oc.owner_sizes(plan, "item")) == sorted(oc.SIZES + oc.SIZES)
    assert users.shape[0] == oc.B < 3000 and any(users[k] > users[k + 1] for k in range(oc.B - 1))
    per = torch.diff(plan["item_chunk_ptr"]).tolist()
    assert sorted(set(per)) == [1, 2, 3] and per == [-(-n // CHUNK) for n in oc.owner_sizes(plan, "item")]
    # a window after the first with `have` partly false: owners of 65 .. 255 occurrences and of 257 + k
    assert {65, 127, 129, 255, 257, 320, 513} <= set(oc.SIZES)


def test_gar_count_batch_is_what_it_claims():
    from coldrec_amd import ops
    own, user_sizes = oc.gar_owners()
    users, pos, neg, items = oc.gar_count_ids()
    n = users.shape[0]
    assert n == sum(user_sizes) < 3000 and len(own) == len(oc.GAR_ITEM_OWNERS) + 1
    plan = ops.gar_plan(users, pos, neg, chunk=CHUNK)
    assert plan["item_ids"].tolist() == sorted(items.tolist())
    sizes = dict(zip(plan["item_ids"].tolist(), oc.owner_sizes(plan, "item")))
    first = dict(zip(plan["item_ids"].tolist(), om.first_counts(plan["item_ptr"], plan["item_occ"], n).tolist()))
    assert [(sizes[int(i)], first[int(i)]) for i in items] == own
    # a plan lists an owner's positives first
    occ, ptr = plan["item_occ"].numpy(), plan["item_ptr"].numpy()
    assert all((np.diff((occ[ptr[s]:ptr[s + 1]] >= n).astype(int)) >= 0).all() for s in range(len(own)))
    firsts = {f for _, f in own} | {"n" for m, f in own if f == m} | {"n-1" for m, f in own if f == m - 1}
    assert {0, 1, 63, 64, 65, 255, 256, 257, "n", "n-1"} <= firsts
    chunks = lambda m: -(-m // CHUNK)
    for c in (1, 2, 3):                                    # cuts inside, at and beside a window and a chunk edge on each
        mine = [(m, f) for m, f in oc.GAR_ITEM_OWNERS if chunks(m) == c]
        assert any(0 < f < m for m, f in mine) and any(f in (0, m) for m, f in mine) and any(f == m - 1 for m, f in mine), c
    assert chunks(oc.GAR_ITEM_OWNERS[oc.GAR_MISCOUNTED][0]) == 3
    assert sorted(oc.owner_sizes(plan, "user")) == sorted(user_sizes) and set(oc.SIZES) <= set(user_sizes)
    (U, V, _, _, _, _), coef = oc.gar_count_inputs(64)
    ratio = float(V[neg].double().norm() / V[pos].double().norm())             # = rinv[1] / rinv[2]
    print(f"|negative block| / |positive block| = {ratio:.3f}; reg = {coef[2]:g} at B = {n}")
    assert ratio < 0.5 and coef[2] == n


@pytest.mark.parametrize("d", oc.WIDTHS)
def test_every_occurrence_is_added_exactly_once(d):
    """Rows on an integer grid in [-8, 8]: any partial sum of up to 513 of them stays below 2^13, every order is exact, and
    the model must equal np.add.at (a model that dropped, doubled or misplaced an occurrence at a window or chunk edge
    would not); so must the count of the occurrences below ``first``."""
    sizes = list(oc.SIZES) + [3 * CHUNK, 3 * CHUNK + 1]
    ptr, occ, chunk_ptr, chunk_own, ids = plan_of(sizes, seed=d)
    rng = np.random.default_rng(d)
    rows = rng.integers(-8, 9, (len(ids), d)).astype(np.float32)
    got = om.owner_sums(ptr, occ, chunk_ptr, chunk_own, d, rows, CHUNK)
    want = np.zeros((len(sizes), d), np.float64)
    np.add.at(want, ids, rows.astype(np.float64))
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.float64), want)
    assert np.array_equal(om.chain_sums(ptr, occ, rows).astype(np.float64), want)
    first = len(ids) // 3
    assert np.array_equal(om.first_counts(ptr, occ, first), np.bincount(ids[:first], minlength=len(sizes)))
    part = om.chunk_partials(ptr, occ, chunk_ptr, chunk_own, d, rows, CHUNK)
    assert part.shape == (len(chunk_own), d) and part.shape[0] == sum(-(-n // CHUNK) for n in sizes)


@pytest.mark.parametrize("d", oc.WIDTHS)
def test_model_is_within_the_derived_bound_of_fp64(d):
    """Bound.  A row enters its owner's result through: the chain of its lane group, in which it is part of at most
    4 LPR - 1 rounded sums (a chunk's 256 occurrences are dealt to RG = 64 / LPR groups, LPR per window and four windows;
    the first addition, to +0, is exact); then the log2(RG) additions of the butterfly; then at most n_chunks - 1 rounded
    additions of the finish (the first, to +0, is exact).  With h = 4 LPR - 1 + log2(RG) + n_chunks - 1 roundings of
    relative size <= u = 2^-24 on its way, the standard argument (Higham, Accuracy and Stability, section 4.2) gives

        |model - exact| <= gamma_h * sum |rows|,   gamma_h = h u / (1 - h u).

    The exact sum is taken in fp64, whose own accumulation adds at most n 2^-53 sum |rows|."""
    sizes = list(oc.SIZES)
    ptr, occ, chunk_ptr, chunk_own, ids = plan_of(sizes, seed=100 + d)
    rng = np.random.default_rng(100 + d)
    rows = rng.standard_normal((len(ids), d)).astype(np.float32)
    rows[rng.random(len(ids)) < 0.1] *= np.float32(1e-6)
    got = om.owner_sums(ptr, occ, chunk_ptr, chunk_own, d, rows, CHUNK).astype(np.float64)
    exact, mag = np.zeros((len(sizes), d)), np.zeros((len(sizes), d))
    np.add.at(exact, ids, rows.astype(np.float64))
    np.add.at(mag, ids, np.abs(rows.astype(np.float64)))
    lpr = om.lpr_for(d)
    for s, n in enumerate(sizes):
        h = 4 * lpr - 1 + int(math.log2(64 // lpr)) + -(-n // CHUNK) - 1
        gamma = h * U32 / (1.0 - h * U32)
        assert (np.abs(got[s] - exact[s]) <= (gamma + n * 2.0 ** -53) * mag[s]).all(), (d, n)


def test_model_is_not_the_chain_and_depends_on_the_lane_group():
    """On N(0, 1) rows the tree of an owner of 200 (one chunk) differs from the plain chain in most columns at every
    LPR < 64 (at LPR = 64 one group walks the chunk in order: the chain), that of an owner of 513 (three chunks) at every
    LPR, and the trees of two lane-group widths differ from each other: a bitwise comparison tells a wrong order from the
    right one."""
    sizes = [200, 513]
    ptr, occ, chunk_ptr, chunk_own, ids = plan_of(sizes, seed=7)
    rng = np.random.default_rng(7)
    rows = rng.standard_normal((len(ids), 256)).astype(np.float32)
    bits = lambda a: np.ascontiguousarray(a).view(np.int32)
    trees = {}
    for d in (4, 8, 16, 32, 64, 128, 256):
        sub = np.ascontiguousarray(rows[:, :d])
        tree, chain = om.owner_sums(ptr, occ, chunk_ptr, chunk_own, d, sub, CHUNK), om.chain_sums(ptr, occ, sub)
        trees[d] = tree[:, :4]
        differ = (bits(tree) != bits(chain)).mean(1)
        if om.lpr_for(d) < 64:
            assert differ[0] >= 0.5, d
        else:
            assert differ[0] == 0.0
        assert differ[1] >= 0.5, d
    for a in trees:
        for b in trees:
            if a < b:
                assert (bits(trees[a]) != bits(trees[b])).any(), (a, b)


def test_butterfly_and_walk_are_the_documented_tree():
    """The model at d = 64 (LPR = 16, RG = 4) against the tree written out by hand for an owner of 70 occurrences: group g
    chains the occurrences g, g + 4, .., g + 60 of the first window and, of the second, g + 64 for g < 6 - 4 .. (those the
    window still has); then (g0 + g2) + (g1 + g3) -- the xor butterfly by 2, then by 1."""
    ptr, occ, chunk_ptr, chunk_own, ids = plan_of([70], seed=3)
    rng = np.random.default_rng(3)
    rows = (rng.standard_normal((70, 64)) * 10.0 ** rng.integers(-3, 4, (70, 64))).astype(np.float32)
    g = []
    for grp in range(4):
        acc = np.zeros(64, np.float32)
        for k in [j * 4 + grp for j in range(16)] + [64 + j * 4 + grp for j in range(16) if 64 + j * 4 + grp < 70]:
            acc = acc + rows[occ[k]]
        g.append(acc)
    want = (g[0] + g[2]) + (g[1] + g[3])
    got = om.owner_sums(ptr, occ, chunk_ptr, chunk_own, 64, rows, CHUNK)[0]
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    pairs = (g[0] + g[1]) + (g[2] + g[3])
    assert not np.array_equal(pairs.view(np.int32), want.view(np.int32))       # the data can tell the pairings apart
    p = rng.standard_normal((8, 5)).astype(np.float32)
    b = om.butterfly(p)
    assert all(np.array_equal(b[0].view(np.int32), b[k].view(np.int32)) for k in range(8))
