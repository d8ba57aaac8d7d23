"""GPU: the owner pass that gar.hip, mtpr.hip and vbpr.hip share (csrc/loss_common.h: lg_owner_chunk_kernel,
lg_owner_finish_kernel, lg_owner_pass) pinned on its own, at the owner sizes and widths of tests/owner_cases.py -- owners of
1 .. 513 occurrences (every window and chunk edge of the chunk kernel, ragged windows after the first among them) at the
thirteen widths that reach all seven lane-group instantiations, full and with lanes that hold no column.

Sum tree.  ``ops.vbpr(..., want_h=True, want_hsum=True)`` without h_adv returns the per-occurrence rows (grad_h) and their
owner sums (grad_hsum); the rows the record kernel hands the pass are those of grad_h (user mode: two * c for both; item
mode: one * c against one * (c + 0)), so grad_hsum must equal oracle/owner_model.py applied to the returned grad_h, BIT FOR
BIT (np.array_equal: signed zeros may differ, nothing else; no tolerance).  That is lg_owner_chunk_kernel<LPR, false>, which
MTPR's and VBPR's table passes run too, and the LgFinishSum finish.  The scores spread over +-30 and more, so coefficients
from 1 down to below 1e-13 of the largest meet in one sum: a lost or doubled occurrence with a small coefficient, or a
changed association, changes bits where it would pass a tolerance.  On the MI355X all 26 cases are bit-equal; the kernel's
sums lie 7.9e-7 of their maximum from the float64 sums of the same rows at worst (d = 132, item mode; 4e-8 .. 6e-7 elsewhere),
the plain left-to-right chain of the host 1.0e-6; the model's rows differ from that chain's at 20 of the 24 item owners and 10
of the 12 users up to d = 128 (all but the owners of 1 and 2) and, at LPR = 64, where one lane group walks a chunk in
order, at the owners of 320 and 513 (a second chunk of more than one occurrence).

Counts.  GAR's finish (LgFinishNorms) weighs an item's row by n_first rinv[1] + (n_all - n_first) rinv[2].  The cases of
tests/owner_cases.py (reg = B = 2746; the positive block's norm over twice the negative's; per-item counts of positives at 0,
1, 63, 64, 65, 255, 256, 257, n - 1 and n on owners of one, two and three chunks) make that part the gradient.  Bars, by the
project's rule 8x the worst distance of the float32 torch formula (CPU) from the float64 one at these same cases, both
modes (tests/test_gar.py prints the figures again, holds them to a factor of 2 and shows that each mutated restatement
lies at least 4x above the bar):
    loss terms, error / total  worst 1.05e-5 (d = 256)  -> COUNT_LOSS_BAR = 8.4e-5
    gradients, error / maximum worst 2.15e-5 (d = 256, d V; float32 torch's norm of a 2746 x 256 block)
                                                        -> COUNT_GRAD_BAR = 1.72e-4
    mutations, least over the widths and modes: one occurrence of a three-chunk owner miscounted 1.57e-3, every
    occurrence counted as a positive 0.24, counts swapped 0.80, R's part dropped on the user side 0.97.
On the MI355X the kernel measures 1.5e-7 (loss terms, d = 20) and 1.7e-7 (gradients, d = 256, user, d G)
at worst over these cases: the bars are float32 torch's, a thousand times the kernel's distance, and a single miscounted
occurrence still lies nine bars away.

LgFinishReg at the same sizes: VBPR's three variants and MTPR's two modes at the profile batch against their float64
restatements, at their files' bars -- VBPR's LOSS_BAR and, as every owner's row is what is left of up to 513 rows that
largely cancel, its "chunks" bar (float32 torch lies 3.4e-6 from float64 here at worst, 4.59e-6 at the "chunks" case);
MTPR's LOSS_BAR and GRAD_BAR (float32 torch 1.2e-6 here, 1.42e-6 at its cases).  On the MI355X the kernels measure 1.1e-7 /
3.0e-6 (VBPR: loss terms / gradients, the latter d Q at d = 256 with h_adv; 1e-7 .. 1.7e-6 elsewhere) and 9.8e-8 / 9.0e-7
(MTPR) at worst.

Mutation check (local breaks of lg_owner_chunk_kernel, run on the MI355X against this file and against the three kernels'
own files): see DESIGN.md, "Owner pass".
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from oracle import owner_model as om
from tests import gar_restate
from tests import mtpr_restate
from tests import owner_cases as oc
from tests import test_gar_gpu as gg
from tests import test_mtpr_gpu as mt
from tests import test_vbpr_gpu as vb
from tests import vbpr_restate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNT_F32_LOSS_WORST, COUNT_F32_GRAD_WORST = 1.05e-5, 2.15e-5    # float32 torch against float64 torch at the count cases
COUNT_LOSS_BAR, COUNT_GRAD_BAR = 8 * COUNT_F32_LOSS_WORST, 8 * COUNT_F32_GRAD_WORST
MUTATION_MARGIN = 4                                              # every mutated restatement: >= 4 bars away
MODES = [False, True]
MODE_IDS = lambda m: "user" if m else "item"
WIDTH_IDS = lambda d: "d%d" % d


def test_the_cases_are_built_for_the_librarys_chunk():
    from coldrec_amd import ops
    assert ops.vbpr_chunk_rows() == ops.mtpr_chunk_rows() == ops.gar_chunk_rows() == oc.CHUNK
    assert {om.lpr_for(d) for d in oc.WIDTHS} == {1, 2, 4, 8, 16, 32, 64}


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("d", oc.WIDTHS, ids=WIDTH_IDS)
def test_hsum_is_the_host_model_bit_for_bit(d, cold_user):
    from coldrec_amd import ops
    inp = oc.vbpr_inputs(d, cold_user, wide=True)
    coef = torch.sigmoid(-oc.vbpr_scores(inp, cold_user))
    assert float(coef.min()) < 1e-6 * float(coef.max())              # coefficients far below the largest
    P, Q, A, h, _, users, pos, neg = (None if t is None else t.to(DEV) for t in inp)
    plan = ops.vbpr_plan(users, pos, neg)
    side = "user" if cold_user else "item"
    assert set(oc.SIZES) <= set(oc.owner_sizes(plan, side))           # every size of the profile, from the plan
    out = ops.vbpr(P, Q, A, h, plan, vbpr_restate.WD1, cold_user=cold_user, want_user=False, want_item=False,
                   want_aux=False, want_h=True, want_hsum=True)
    torch.cuda.synchronize()
    rows, hsum = out[4].cpu().numpy(), out[6].cpu().numpy()
    assert rows.shape == ((1 if cold_user else 2) * oc.B, d) and np.isfinite(rows).all()
    top = np.abs(rows).max(1)                                         # (a record with pos == neg has a zero row in user mode)
    assert (top > 0).mean() > 0.9 and top[top > 0].min() < 1e-6 * top.max()      # ... and so are the rows that meet in the sums
    side_of = lambda k: plan[f"{side}_{k}"].cpu().numpy()
    args = (side_of("ptr"), side_of("occ"), side_of("chunk_ptr"), side_of("chunk_own"))
    model = om.owner_sums(*args, d, rows, ops.vbpr_chunk_rows())
    chain = om.chain_sums(args[0], args[1], rows)
    exact = vbpr_restate.owner_sums(torch.from_numpy(rows).double(), inp[5] if cold_user else torch.cat(inp[6:])).numpy()
    dist = lambda a: float(np.abs(a.astype(np.float64) - exact).max() / np.abs(exact).max())
    print(f"d{d} {side}: kernel {dist(hsum):.2e}, plain chain {dist(chain):.2e} of the maximum from the float64 sums; "
          f"{int((model != chain).any(1).sum())} of {len(model)} owners' model rows are not the chain's")
    assert (model != chain).any()                                     # the comparison pins more than a chain would
    assert hsum.shape == model.shape and np.array_equal(hsum, model)


@pytest.mark.parametrize("variant", vb.VARIANTS, ids=vb.VARIANT_IDS)
@pytest.mark.parametrize("d", oc.WIDTHS, ids=WIDTH_IDS)
def test_vbpr_tables_and_hsum_at_the_profile(d, variant):
    cold_user, adv = variant
    inp = oc.vbpr_inputs(d, cold_user, adv)
    got = vb._fused(inp, vb.WD1, cold_user)
    assert got[6] is not None and (got[5] is not None) == adv
    want = vbpr_restate.step(*inp, vb.WD1, cold_user, vb.LMD)
    vb._compare(f"d{d} {vb.VARIANT_IDS(variant)}", got, want, vb.LOSS_BAR, vb.CHUNKS_GRAD_BAR)


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("d", oc.MTPR_WIDTHS, ids=WIDTH_IDS)
def test_mtpr_tables_at_the_profile(d, cold_user):
    inp = oc.mtpr_inputs(d, cold_user)
    got = mt._fused(inp, mt.WD1, cold_user)
    mt._compare(f"d{d} {MODE_IDS(cold_user)}", got, mtpr_restate.step(*inp, mt.WD1, cold_user), mt.LOSS_BAR, mt.GRAD_BAR)


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("d", oc.WIDTHS, ids=WIDTH_IDS)
def test_gar_counts_decide_the_gradient(d, cold_user):
    """Bars: COUNT_LOSS_BAR / COUNT_GRAD_BAR above (from the float32 torch formula on the CPU, not from the kernel)."""
    from coldrec_amd import ops
    inp, coef = oc.gar_count_inputs(d)
    plan = ops.gar_plan(inp[2], inp[3], inp[4])
    n = inp[2].shape[0]
    first = om.first_counts(plan["item_ptr"], plan["item_occ"], n).tolist()
    own, user_sizes = oc.gar_owners()
    assert sorted(zip(oc.owner_sizes(plan, "item"), first)) == sorted(own) and n < 3000
    assert sorted(oc.owner_sizes(plan, "user")) == sorted(user_sizes)
    got = gg._fused(inp, coef, cold_user)
    gg._compare(f"d{d} {MODE_IDS(cold_user)}", got, gar_restate.step(*inp, *coef, cold_user), COUNT_LOSS_BAR, COUNT_GRAD_BAR)


# ======================================================================================================== fuzzer
FUZZ_CASES, FUZZ_SEED = 60, 2026


def test_loss_fuzzer_short_run_of_the_three_kinds():
    """tests/fuzz/fuzz_loss_ops.py --only gar,mtpr,vbpr --cases 60 --seed 2026 in a child process: 60 random cases over the
    three kernels that end in the owner pass (17 gar, 19 mtpr, 24 vbpr at this seed).  Measured on the MI355X: 3.0 s for the
    whole child, the interpreter's start and the library's load included."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_loss_ops.py"), "--only", "gar,mtpr,vbpr",
           "--cases", str(FUZZ_CASES), "--seed", str(FUZZ_SEED)]
    t0 = time.time()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    print(f"fuzzer: {time.time() - t0:.1f} s; {out.stdout.strip().splitlines()[-1:]}")
    assert out.returncode == 0 and "fuzz ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
