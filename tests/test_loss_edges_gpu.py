"""GPU: the fused CLCRec, CCFCRec and ALDI losses (csrc/clcrec.hip, csrc/ccfcrec.hip, csrc/aldi.hip) at the shapes and
values their own test files (tests/test_clcrec_gpu.py, tests/test_ccfcrec_gpu.py, tests/test_aldi_gpu.py) never reach,
against the same float64 restatements, with those files' helpers (_inputs, _fused, distances).  No entry is skipped and
no tolerance excuses a case: a gradient row the restatement leaves exactly zero is compared against zero.

What each group reaches (LPR = the lanes of a row's group = pow2(d / 4); R = 64 / LPR rows per pass):

CLCRec
  widths      d = 8, 12 | 16, 28 | 32, 36 | 68, 100, 128 | 200, 252 -> clc_launch<2>, <4>, <4>, <8>, <8>, <16>, <32>, <32>,
              <32>, <64>, <64>: the instantiations 2, 4 and 32 nothing else launches, and widths with idle lanes beside
              every boundary.  B = 9 records over 4 users and 6 items: every owner has several occurrences, so
              clc_cross_sum and the __shfl(mine, j * R + grp) walk of the slot and user kernels carry real terms.
  row passes  the record kernel's `g0 += R` loop: d = 4 (R = 64) with 1 + G = 63, 64, 65, 129 (a short pass, a full one,
              one row into the second, one row into the third); d = 64 (R = 4) with 1 + G = 3, 4, 5; d = 256 (R = 1), G = 1.
  caps        G = clcrec_max_neg() (1024: 12 KiB of dynamic LDS, 17 strides of the 64-lane softmax loops) at d = 4, 256.
  slot chunks one slot with chunk - 1, chunk, chunk + 1, 2 chunk, 2 chunk + 1 occurrences (chunk = crh_clcrec_chunk_rows()):
              1, 1, 2, 2, 3 chunks -- k_begin's `(ch - chunk_ptr[s]) * CLC_CHUNK`, the k_end clamp, the `k0 += 64` loop's
              last short trip and clc_finish_kernel's loop over more than one partial; the occurrences are positives and
              negatives, mixed and unmixed rows.
  user runs   one user with 63, 64, 65, 128, 129 records: clc_user_kernel's `k0 += 64` loop at 1, 1, 2, 2, 3 trips.
  big logits  U x 3.0 at T = 0.1, and with V, feat x 1.0 at T = 0.05: max_g s2 - s2_0 > 69 in 31 and 36 of the 40 records
              (asserted on the restatement's scores for at least one), so clc_softmax_coef returns
              (m - s0) + logf(l) and the positive's coefficient is -l_off * inv_l with e0 flushed.
  zero rows   a zero feat row (nf < CLC_EPS: `pa * inv_nf + pc`), a zero item row as a positive and as a negative
              (np < CLC_EPS: `acc_h * inv_np`; `nv > 0.f` false) and a zero user row (`nu > 0.f` false).  The rows whose
              gradient F.normalize's clamp scales by 1 / eps (about 1e10 against 1e-2 elsewhere) are compared on their
              own, error over their own maximum, and the rest with them left out: both parts are compared.  At a row of
              exact zeros z = f / eps is zero too and both forms of the two `>= CLC_EPS` ternaries give the same bits,
              so the same feat row and item row also come with the norm 8e-13 < eps (z and h of length 0.8): there
              `pa` against `pa - z * zd` and `acc_h` against `acc_h - h * hd` differ by a good part of the row.
CCFCRec
  widths      the same eleven widths through ccf_launch<2> .. <64>, B = 9, P = 2, N = 3, S = 2, 4 users, 6 items.
  cap         R = ccfcrec_max_rows() (4096: 48 KiB of dynamic LDS) with P = 1, N = 4000, S = 94 at d = 4 and d = 256.
  user chunks 2 users, one with chunk - 1, chunk, chunk + 1, 2 chunk + 1 of the 2B occurrences users ++ neg_users (on both
              the u_b and the k_b side): ccf_user_chunk_kernel's chunk offset and clamp, ccf_user_finish_kernel's loop
              over 1, 1, 2, 3 partials.
  item chunks one item with chunk - 1 .. 2 chunk + 1 of the B R occurrences at R = 4, some of them at r = 0 (the rank
              vector's sum): ccf_item_chunk_kernel / ccf_item_finish_kernel the same way.
ALDI
  chunk tree  B = 15, 16, 17, 33, 48, 49, 64, 65, 80, 81 (1, 1, 2, 3, 3, 4, 4, 5, 5, 6 workgroups of 16 records; "wave g
              takes chunks g, g + 4, ..." with 0, 1 or 2 chunks per wave and a last workgroup of 1, 15 or 16 records) at
              d = 8 (2 lanes) and d = 64.
  saturated   teacher x 1.5, student x 1.3: |tp - tn| > 17 in about half of the 65 records and > 40 in some, both signs
              (z = sigmoid(t) rounds to 1 or 0: aldi_bce's `omz - oms` and `x * omz` forms), sp - sn beyond +-30.

Bars.  CLCRec keeps its file's 1e-5 (loss terms, relative) and 1e-4 (gradients, error / maximum); float32 torch on the
CPU lies 3.0e-6 / 1.8e-5 from float64 on the gradients of the two big-logit cases and 8.1e-8 or less on their loss terms
(tests/test_clcrec.py prints them), 1.4e-7 on the zero-norm rows compared apart.  In CCFCRec's user-chunk cases u_b and
k_b are the same user in most records, so dU is a sum of cancelling pairs: that is where float32 torch is furthest.  CCFCRec
and ALDI: 8x the worst distance of the float32 torch formula from the float64 one over the NEW cases, measured on the CPU
(tests/test_ccfcrec.py and tests/test_aldi.py print them again), or the file's own bar where that is larger:
    CCFCRec loss terms, relative:       worst 1.99e-7 (width d128) -> 8x = 1.59e-6; the file's bar 1.08e-6: EDGE bar = 1.59e-6
    CCFCRec gradients, error / maximum: worst 2.59e-6 (user with 513 occurrences, dU) -> 8x = 2.07e-5; the file's bar 3.07e-6: EDGE bar = 2.07e-5
    ALDI loss terms, error / total:     worst 1.14e-7 (B33-d64) -> 8x = 9.12e-7; the file's bar 6.21e-7: EDGE bar = 9.12e-7
    ALDI gradients, error / maximum:    worst 2.42e-7 (saturated) -> 8x = 1.94e-6; the file's bar 2.08e-6: EDGE bar = 2.08e-6 (the file's)
No bar is taken from what a kernel produced.  On the MI355X the kernels measure, at worst: CLCRec loss terms 1.2e-7,
gradients 3.0e-6 (dU at G = 1024, d = 256; 2.4e-6 at the big logits, 4e-7 and less elsewhere); ALDI 1.4e-7 / 3.4e-7; CCFCRec
loss terms 1.4e-7, gradients 1.5e-6 (the user in three chunks) -- and 1.1e-5 for dQ at R = 4096 with d = 256, where float32
torch lies 1.6e-7: LPR = 64 leaves one lane group, so pass B adds all 4096 rows in one float32 chain, and a host model of
that chain (float32 running sum, float64 everything else) lies 1.13e-5 from float64 itself.  Rounding of the chain, then, not
a wrong term; it passes because the user-chunk cases set CCFCRec's bar, and would not pass the file's own 3.07e-6.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import aldi_restate, ccfcrec_restate, clcrec_restate
from tests import test_aldi_gpu as ald
from tests import test_ccfcrec_gpu as ccf
from tests import test_clcrec_gpu as clc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WIDTHS = [8, 12, 16, 28, 32, 36, 68, 100, 128, 200, 252]

# float32 torch against float64 torch at the new cases, measured on the CPU (see the docstring)
CCF_F32_LOSS_WORST, CCF_F32_GRAD_WORST = 1.99e-7, 2.59e-6
ALD_F32_LOSS_WORST, ALD_F32_GRAD_WORST = 1.14e-7, 2.42e-7
CCF_LOSS_BAR, CCF_GRAD_BAR = max(8 * CCF_F32_LOSS_WORST, ccf.LOSS_BAR), max(8 * CCF_F32_GRAD_WORST, ccf.GRAD_BAR)
ALD_LOSS_BAR, ALD_GRAD_BAR = max(8 * ALD_F32_LOSS_WORST, ald.LOSS_BAR), max(8 * ALD_F32_GRAD_WORST, ald.GRAD_BAR)


def _lib():
    from coldrec_amd import _lib as L
    return L.lib()


def _bit_equal(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


# ======================================================================================================== CLCRec
#                  B  G  d  nu ni   T   lam  num_sample
CLC_WIDTH_CASES = [(9, 5, d, 4, 6, 0.5, 0.5, 0.5) for d in WIDTHS]
CLC_PASS_CASES = ([(3, g1 - 1, 4, 3, 20, 0.5, 0.5, 0.5) for g1 in (63, 64, 65, 129)]
                  + [(3, g1 - 1, 64, 3, 20, 0.5, 0.5, 0.5) for g1 in (3, 4, 5)] + [(3, 1, 256, 3, 20, 0.5, 0.5, 0.5)])
CLC_IDS = lambda c: "B%d-G%d-d%d" % c[:3]


def _clc_run_twice(case, inp, want):
    got = clc._fused(case, inp)
    clc._compare(CLC_IDS(case), got, want)
    assert _bit_equal(got, clc._fused(case, inp)), "two identical calls differ in their bits"
    return got


def _clc_untouched_are_zero(case, inp, got):
    users, items = inp[3], inp[4]
    um, im = torch.ones(case[3], dtype=torch.bool), torch.ones(case[4], dtype=torch.bool)
    um[users] = False
    im[items.reshape(-1)] = False
    assert (got[1].cpu()[um] == 0).all() and (got[2].cpu()[im] == 0).all()


@pytest.mark.parametrize("case", CLC_WIDTH_CASES + CLC_PASS_CASES, ids=CLC_IDS)
def test_clcrec_widths_and_row_passes(case):
    inp = clc._inputs(case)
    assert torch.bincount(inp[3]).max() >= 2 or case[0] == 3       # (owners with several occurrences on the width grid)
    want = clcrec_restate.step(*inp, case[5], case[6], clc.REG)
    _clc_untouched_are_zero(case, inp, _clc_run_twice(case, inp, want))


@pytest.mark.parametrize("d", [4, 256])
def test_clcrec_at_the_negatives_cap(d):
    from coldrec_amd import ops
    case = (2, ops.clcrec_max_neg(), d, 3, 50, 0.5, 0.5, 0.5)
    inp = clc._inputs(case)
    want = clcrec_restate.step(*inp, case[5], case[6], clc.REG)
    _clc_untouched_are_zero(case, inp, _clc_run_twice(case, inp, want))


def clc_slot_chunk_inputs(c, B=64, G=8, d=32, nu=10, ni=40):
    """Item 0 at exactly c of the B (1 + G) flat rows (a seeded choice of positions), the other rows on items 1 .. ni - 1."""
    case = (B, G, d, nu, ni, 0.5, 0.5, 0.5)
    U, V, _, users, items, rand_index = clc._inputs(case, seed=c)
    g = torch.Generator().manual_seed(7000 + c)
    M = B * (1 + G)
    flat = torch.randint(1, ni, (M,), generator=g)
    flat[torch.randperm(M, generator=g)[:c]] = 0
    items = flat.view(B, 1 + G)
    E = torch.randn(torch.unique(flat).numel(), d, generator=g) * 0.5
    return case, (U, V, E, users, items, rand_index)


@pytest.mark.parametrize("which", range(5), ids=["chunk-1", "chunk", "chunk+1", "2chunk", "2chunk+1"])
def test_clcrec_slot_split_into_chunks(which):
    from coldrec_amd import ops
    chunk = int(_lib().crh_clcrec_chunk_rows())
    c = [chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1][which]
    case, inp = clc_slot_chunk_inputs(c)
    items, rand_index = inp[4], inp[5]
    hot = (items == 0)
    assert int(hot.sum()) == c and hot[:, 0].any() and hot[:, 1:].any()           # positives and negatives
    mixed = torch.bincount(rand_index, minlength=items.numel()).view_as(items) > 0
    assert (hot & mixed).any() and (hot & ~mixed).any()                            # mixed and unmixed rows
    plan = ops.clcrec_plan(inp[3].to(DEV), items.to(DEV), case[3], case[4])
    assert int(plan["slot_item"][0]) == 0
    assert int(plan["chunk_ptr"][1] - plan["chunk_ptr"][0]) == [1, 1, 2, 2, 3][which] == -(-c // chunk)
    want = clcrec_restate.step(*inp, case[5], case[6], clc.REG)
    _clc_untouched_are_zero(case, inp, _clc_run_twice(case, inp, want))


def clc_user_run_inputs(n, G=3, d=32, nu=6, ni=30):
    """User 0 in exactly n of the B = n + 7 records (a seeded choice), the other records on users 1 .. nu - 1."""
    case = (n + 7, G, d, nu, ni, 0.5, 0.5, 0.5)
    U, V, E, _, items, rand_index = clc._inputs(case, seed=n)
    g = torch.Generator().manual_seed(7100 + n)
    users = torch.randint(1, nu, (n + 7,), generator=g)
    users[torch.randperm(n + 7, generator=g)[:n]] = 0
    return case, (U, V, E, users, items, rand_index)


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129])
def test_clcrec_user_with_many_records(n):
    case, inp = clc_user_run_inputs(n)
    assert int((inp[3] == 0).sum()) == n
    want = clcrec_restate.step(*inp, case[5], case[6], clc.REG)
    _clc_untouched_are_zero(case, inp, _clc_run_twice(case, inp, want))


#                    U     V    feat   T
CLC_LOGIT_SCALES = [(3.0, 0.3, 0.5, 0.1), (3.0, 1.0, 1.0, 0.05)]


def clc_big_logit_inputs(su, sv, sf, T):
    """tests/test_clcrec_gpu.py's inputs (tables of scale 0.3, feat 0.5) rescaled to (su, sv, sf)."""
    case = (40, 16, 64, 30, 60, T, 0.5, 0.5)
    U, V, E, users, items, rand_index = clc._inputs(case)
    return case, (U * (su / 0.3), V * (sv / 0.3), E * (sf / 0.5), users, items, rand_index)


def clc_second_scores(inp, T):
    """The restatement's s2 (B, 1 + G) in float64."""
    U, V, E, users, items, rand_index = (t.double() if t.is_floating_point() else t for t in inp)
    slot = torch.unique(items.reshape(-1), return_inverse=True)[1]
    x = V[items.reshape(-1)].clone()
    x[rand_index] = E[slot][rand_index]
    return ((U[users].repeat_interleave(items.shape[1], 0) * x).sum(1) / T).view(items.shape)


@pytest.mark.parametrize("scales", CLC_LOGIT_SCALES, ids=["U3-V0.3-F0.5-T0.1", "U3-V1-F1-T0.05"])
def test_clcrec_large_logits(scales):
    case, inp = clc_big_logit_inputs(*scales)
    s2 = clc_second_scores(inp, scales[3])
    far = int(((s2.max(1).values - s2[:, 0]) > 69).sum())
    print(f"{far} of {s2.shape[0]} records have max_g s2 - s2_0 > 69")
    assert far >= 1                                        # exp(s0 - m) flushes below 1e-30: the softmax's second branch
    want = clcrec_restate.step(*inp, case[5], case[6], clc.REG)
    assert np.isfinite(want[0]).all() and all(np.isfinite(w).all() for w in want[1:])
    got = clc._fused(case, inp)
    assert torch.isfinite(got[0]).all() and all(torch.isfinite(g).all() for g in got[1:])
    clc._compare("large logits", got, want)
    assert _bit_equal(got, clc._fused(case, inp))


def _compare_split(tag, got, want, apart):
    """tests/test_clcrec_gpu.py's _compare with the rows ``apart[name]`` of a gradient compared on their own (error over
    their own maximum) and the other rows with them left out; every row is in one of the two parts."""
    loss, grads = got[0], [g.cpu().numpy().astype(np.float64) for g in got[1:]]
    assert torch.isfinite(loss).all() and all(np.isfinite(g).all() for g in grads), f"{tag}: not finite"
    assert np.isfinite(want[0]).all() and all(np.isfinite(w).all() for w in want[1:])
    rel = np.abs(loss.numpy().astype(np.float64) - want[0]) / np.abs(want[0])
    errs = []
    for name, g, w in zip(("dU", "dV", "dE"), grads, want[1:]):
        rows = np.zeros(w.shape[0], bool)
        rows[np.asarray(apart.get(name, []), dtype=np.int64)] = True
        for part in (rows, ~rows):
            if part.any():
                top = np.abs(w[part]).max()
                errs.append(np.abs(g[part] - w[part]).max() / top if top > 0 else np.abs(g[part]).max())
        assert np.array_equal(g[(w == 0).all(1)], w[(w == 0).all(1)]), f"{tag}: {name} is not zero at an untouched row"
    print(f"{tag}: loss rel {rel.max():.2e}, gradient err / max per part {' '.join('%.2e' % e for e in errs)}")
    assert rel.max() <= 1e-5
    assert max(errs) <= 1e-4


def clc_zero_row_inputs(which):
    """B = 24, G = 6, d = 32 over 10 users and 25 items; ``which`` = 'feat': the feat row of item 4's slot is zero;
    'item': V[4] is zero, item 4 the positive of records 0 and 5 and a negative of records 1 and 5; 'user': U[2] is zero,
    user 2 in records 0, 3 and 4; 'tiny-feat' / 'tiny-item': that row with the norm 8e-13, below the clamp.
    Returns (case, inputs, zero_rows for the restatement, rows compared apart)."""
    case = (24, 6, 32, 10, 25, 0.5, 0.3, 0.5)
    U, V, E, users, items, rand_index = clc._inputs(case, seed=9)
    items[0, 0], items[5, 0], items[1, 2], items[5, 3] = 4, 4, 4, 4
    users[0], users[3], users[4] = 2, 2, 2
    slot_item = torch.unique(items.reshape(-1))
    g = torch.Generator().manual_seed(7200)
    E = torch.randn(slot_item.numel(), 32, generator=g) * 0.5
    k = int((slot_item == 4).nonzero()[0])
    tiny = torch.nn.functional.normalize(torch.randn(32, generator=g), dim=0) * 8e-13
    if which in ("feat", "tiny-feat"):
        E[k] = 0 if which == "feat" else tiny
        return case, (U, V, E, users, items, rand_index), None, {"dE": [k]}
    if which in ("item", "tiny-item"):
        V[4] = 0 if which == "item" else tiny
        return case, (U, V, E, users, items, rand_index), ([], [4]) if which == "item" else None, {"dV": [4]}
    U[2] = 0
    return case, (U, V, E, users, items, rand_index), ([2], []), {}


@pytest.mark.parametrize("which", ["feat", "item", "user", "tiny-feat", "tiny-item"])
def test_clcrec_zero_norm_rows(which):
    case, inp, zero_rows, apart = clc_zero_row_inputs(which)
    want = clcrec_restate.step(*inp, case[5], case[6], clc.REG, zero_rows=zero_rows)
    if zero_rows is not None:                                    # without the keyword autograd's sqrt at 0 gives NaN there only
        plain = clcrec_restate.step(*inp, case[5], case[6], clc.REG)
        bad = np.isnan(plain[2 if which == "item" else 1]).any(1)
        assert bad.sum() == 1 and bad[4 if which == "item" else 2]
    for name, rows in apart.items():                       # the clamp's 1 / eps: the row sets a scale of its own
        w = want[1 + ("dU", "dV", "dE").index(name)]
        assert np.abs(w[rows]).max() > 1e6 * np.abs(np.delete(w, rows, 0)).max()
    got = clc._fused(case, inp)
    _compare_split(f"zero {which} row", got, want, apart)
    assert _bit_equal(got, clc._fused(case, inp))


# ======================================================================================================= CCFCRec
#                   B  P  N  S  d  nu ni  tau  lambda1
CCF_WIDTH_CASES = [(9, 2, 3, 2, d, 4, 6, 0.1, 0.6) for d in WIDTHS]
CCF_CAP_CASES = [(2, 1, 4000, 94, d, 5, 500, 0.1, 0.6) for d in (4, 256)]
CCF_USER_COUNTS = lambda chunk: [chunk - 1, chunk, chunk + 1, 2 * chunk + 1]
CCF_ITEM_COUNTS = lambda chunk: [chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1]


def ccf_user_chunk_inputs(c):
    """2 users, P = N = S = 1, d = 32: user 0 at exactly c of the 2B occurrences users ++ neg_users, B = (c + 9) // 2."""
    B = (c + 9) // 2
    case = (B, 1, 1, 1, 32, 2, 30, 0.1, 0.6)
    inp = list(ccf._inputs(case, seed=c))
    g = torch.Generator().manual_seed(7300 + c)
    both = torch.ones(2 * B, dtype=torch.long)
    both[torch.randperm(2 * B, generator=g)[:c]] = 0
    inp[3], inp[5] = both[:B].clone(), both[B:].clone()
    return case, tuple(inp)


def ccf_item_chunk_inputs(c):
    """R = 4 (P = N = S = 1), d = 32: item 0 at exactly c of the B R flat rows, B = (c + 11) // 4, the rest on 1 .. 29."""
    B = (c + 11) // 4
    case = (B, 1, 1, 1, 32, 5, 30, 0.1, 0.6)
    inp = list(ccf._inputs(case, seed=c))
    g = torch.Generator().manual_seed(7400 + c)
    flat = torch.randint(1, 30, (4 * B,), generator=g)
    flat[torch.randperm(4 * B, generator=g)[:c]] = 0
    flat = flat.view(B, 4)
    inp[4], inp[6], inp[7], inp[8] = flat[:, 0].clone(), flat[:, 1:2].clone(), flat[:, 2:3].clone().view(B, 1, 1), \
        flat[:, 3:4].clone()
    return case, tuple(inp)


def ccf_edge_cases(chunk=256):
    """Every new CCFCRec case as (id, case, inputs): what the GPU tests run and the CPU measurement measures."""
    out = [("width-" + ccf.IDS(c), c, ccf._inputs(c)) for c in CCF_WIDTH_CASES]
    out += [("cap-" + ccf.IDS(c), c, ccf._inputs(c)) for c in CCF_CAP_CASES]
    out += [("user%d" % c,) + ccf_user_chunk_inputs(c) for c in CCF_USER_COUNTS(chunk)]
    out += [("item%d" % c,) + ccf_item_chunk_inputs(c) for c in CCF_ITEM_COUNTS(chunk)]
    return out


def _ccf_check(tag, case, inp):
    want = ccfcrec_restate.step(*inp, case[7], case[8])
    got = ccf._fused(case, inp)
    loss, gu, gv, gq = got
    arrs = (loss.numpy(), gu.cpu().numpy(), gv.cpu().numpy(), gq.cpu().numpy())
    rel, errs = ccf.distances(arrs, want)
    print(f"{tag}: loss rel {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    for name, g, w in (("dU", arrs[1], want[1]), ("dV", arrs[2], want[2]), ("dQ", arrs[3], want[3])):
        assert not g[(w == 0).all(1)].any(), f"{tag}: {name} is not zero where the restatement's row is"
    um, im = torch.ones(case[5], dtype=torch.bool), torch.ones(case[6], dtype=torch.bool)
    um[inp[3]] = False
    um[inp[5]] = False
    for t in (inp[4], inp[6], inp[7], inp[8]):
        im[t.reshape(-1)] = False
    assert (gu.cpu()[um] == 0).all() and (gv.cpu()[im] == 0).all()                # rows no record touches: exactly zero
    assert rel <= CCF_LOSS_BAR
    assert max(errs) <= CCF_GRAD_BAR
    assert _bit_equal(got, ccf._fused(case, inp)), "two identical calls differ in their bits"


@pytest.mark.parametrize("case", CCF_WIDTH_CASES, ids=ccf.IDS)
def test_ccfcrec_widths(case):
    inp = ccf._inputs(case)
    assert torch.bincount(torch.cat([inp[3], inp[5]])).max() >= 2
    _ccf_check(ccf.IDS(case), case, inp)


@pytest.mark.parametrize("d", [4, 256])
def test_ccfcrec_at_the_rows_cap(d):
    from coldrec_amd import ops
    cap = ops.ccfcrec_max_rows()
    S = 94
    case = (2, 1, cap - 2 - S, S, d, 5, 500, 0.1, 0.6)
    assert ops.ccfcrec_rows(*case[1:4]) == cap and case in CCF_CAP_CASES
    _ccf_check(ccf.IDS(case), case, ccf._inputs(case))


@pytest.mark.parametrize("which", range(4), ids=["chunk-1", "chunk", "chunk+1", "2chunk+1"])
def test_ccfcrec_user_split_into_chunks(which):
    from coldrec_amd import ops
    chunk = int(_lib().crh_ccfcrec_chunk_rows())
    c = CCF_USER_COUNTS(chunk)[which]
    case, inp = ccf_user_chunk_inputs(c)
    B = case[0]
    assert int((inp[3] == 0).sum()) + int((inp[5] == 0).sum()) == c
    assert (inp[3] == 0).any() and (inp[5] == 0).any()                            # on the u_b side and on the k_b side
    plan = ops.ccfcrec_plan(*(t.to(DEV) for t in inp[3:]), 2, case[6])
    assert plan["n_users"] == 2 and plan["n_user_chunks"] == -(-c // chunk) + -(-(2 * B - c) // chunk)
    assert int(plan["user_chunk_ptr"][1]) == [1, 1, 2, 3][which]
    _ccf_check("user with %d occurrences" % c, case, inp)


@pytest.mark.parametrize("which", range(5), ids=["chunk-1", "chunk", "chunk+1", "2chunk", "2chunk+1"])
def test_ccfcrec_item_split_into_chunks(which):
    from coldrec_amd import ops
    chunk = int(_lib().crh_ccfcrec_chunk_rows())
    c = CCF_ITEM_COUNTS(chunk)[which]
    case, inp = ccf_item_chunk_inputs(c)
    flat = torch.cat([inp[4].view(-1, 1), inp[6], inp[7].view(-1, 1), inp[8]], 1)
    assert int((flat == 0).sum()) == c and (flat[:, 0] == 0).any() and (flat[:, 1:] == 0).any()       # some at r = 0
    plan = ops.ccfcrec_plan(*(t.to(DEV) for t in inp[3:]), case[5], case[6])
    assert int(plan["item_ids"][0]) == 0 and int(plan["item_chunk_ptr"][1]) == [1, 1, 2, 2, 3][which] == -(-c // chunk)
    _ccf_check("item with %d occurrences" % c, case, inp)


# ========================================================================================================== ALDI
ALD_TREE_CASES = [(B, d, 11, 30, 0.3, ald.COEF) for d in (8, 64) for B in (15, 16, 17, 33, 48, 49, 64, 65, 80, 81)]
ALD_SAT_CASE = (65, 64, 40, 90, 1.0, ald.COEF)
ALD_SAT_TEACHER, ALD_SAT_STUDENT = 1.5, 1.3


def ald_saturated_inputs():
    U, V, users, pos, neg, gu, gp, gn, w = ald._inputs(ALD_SAT_CASE, seed=1)
    s, g = ALD_SAT_TEACHER, ALD_SAT_STUDENT
    return U * s, V * s, users, pos, neg, gu * g, gp * g, gn * g, w


def ald_edge_cases():
    """Every new ALDI case as (id, case, inputs)."""
    return [(ald.IDS(c), c, ald._inputs(c)) for c in ALD_TREE_CASES] + [("saturated", ALD_SAT_CASE, ald_saturated_inputs())]


def _ald_check(tag, case, inp):
    want = aldi_restate.step(*inp, *case[5])
    got = ald._fused(case, inp)
    assert torch.isfinite(got[0]).all() and all(torch.isfinite(g).all() for g in got[1:]), f"{tag}: not finite"
    arrs = (got[0].numpy(),) + tuple(g.cpu().numpy() for g in got[1:])
    rel, errs = ald.distances(arrs, want)
    print(f"{tag}: loss err / total {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert rel <= ALD_LOSS_BAR
    assert max(errs) <= ALD_GRAD_BAR
    assert _bit_equal(got, ald._fused(case, inp)), "two identical calls differ in their bits"


@pytest.mark.parametrize("case", ALD_TREE_CASES, ids=ald.IDS)
def test_aldi_chunk_tree(case):
    _ald_check(ald.IDS(case), case, ald._inputs(case))


def ald_saturation_figures(inp):
    """(tp - tn, sp - sn) per record in float64."""
    U, V, users, pos, neg, gu, gp, gn, _ = (t.double() if t.is_floating_point() else t for t in inp)
    t = (U[users] * (V[pos] - V[neg])).sum(1)
    x = (gu * gp).sum(1) - (gu * gn).sum(1)
    return t.numpy(), x.numpy()


def test_aldi_saturated_teacher():
    inp = ald_saturated_inputs()
    t, x = ald_saturation_figures(inp)
    print(f"tp - tn: {int((np.abs(t) > 17).sum())} of {t.size} beyond 17, {int((t > 40).sum())} above 40, "
          f"{int((t < -40).sum())} below -40; sp - sn in [{x.min():.1f}, {x.max():.1f}]")
    assert (np.abs(t) > 17).sum() >= t.size // 4 and (t > 40).any() and (t < -40).any()
    assert (t > 17).sum() >= 4 and (t < -17).sum() >= 4 and x.min() <= -30 and x.max() >= 30
    assert ((t > 17) & (x >= 0)).any() and ((t > 17) & (x < 0)).any()              # both forms of the slope
    assert aldi_restate.min_rate_gap(*inp[:8]) >= 1e-5                             # L_rate's signs agree in every precision
    _ald_check("saturated", ALD_SAT_CASE, inp)


# ======================================================================================================== fuzzer
FUZZ_CASES, FUZZ_SEED = 60, 2025


def test_loss_fuzzer_short_run():
    """tests/fuzz/fuzz_loss_ops.py --only clcrec,ccfcrec,aldi --cases 60 --seed 2025 in a child process: 60 random cases
    over the three kernels (--only keeps the fuzzer's later kinds out of the draw: the same 60 cases as before them).
    Measured on the MI355X: 3.1 s for the whole child, the interpreter's start and the library's load included."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_loss_ops.py"), "--only", "clcrec,ccfcrec,aldi",
           "--cases", str(FUZZ_CASES), "--seed", str(FUZZ_SEED)]
    t0 = time.time()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    print(f"fuzzer: {time.time() - t0:.1f} s; {out.stdout.strip().splitlines()[-1:]}")
    assert out.returncode == 0 and "fuzz ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
