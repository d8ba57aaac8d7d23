"""GPU: the fused two-tower BPR loss of VBPR / AMR (csrc/vbpr.hip) against the float64 restatement (tests/vbpr_restate.py,
itself pinned to the reference's runs by tests/test_vbpr.py), in item mode without and with H_adv and in user mode: the
shapes where it can go wrong, the edges, the contracts, the argument errors, the trainers' autograd operator, and whole
VBPR and AMR runs against G26.

Bars of the kernel against the float64 restatement: 8x the worst distance of the float32 torch formula (CPU) from the
float64 one at the same cases, all three variants.  Loss terms are measured as error over the TOTAL loss, gradients
(grad_hsum among them) as error over their maximum.  Measured on the CPU (tests/test_vbpr.py prints them again and holds
them to a factor of 2):
    cases:  loss terms, error / total  worst 1.29e-7 (B2048-d64, user)    -> LOSS_BAR = 1.03e-6
            gradients, error / maximum worst 3.29e-7 (B16417-d4, item, d P) -> GRAD_BAR = 2.63e-6
            ... in the "chunks" case, where every owner's gradient row is what is left of 513 or more rows that largely
            cancel, worst 4.59e-6 (user, d A; 6.4e-7 .. 3.8e-6 in the other variants) -> CHUNKS_GRAD_BAR = 3.67e-5
    edges:  loss terms worst 9.52e-8, gradients worst 7.97e-7 (scores beyond +-30, item with H_adv); the edge bars are 8x
            these or the cases' bars, whichever is larger: 1.03e-6 and 6.38e-6
On the MI355X the kernel measures 8.2e-8 (loss terms, B7-d256) and 1.7e-7 (gradients, B2048-d64) at worst over the
cases, 1.1e-7 and 5.1e-7 in the "chunks" case, 9.5e-8 (H_adv == H) and 5.3e-7 (scores beyond +-30) over the edges.

Whole runs against G26 (VBPR item, VBPR user, AMR item): plain float32 torch on the CPU on one thread (tests/test_vbpr.py)
ends 1.41e-7 / 2.20e-7 / 1.57e-7 of the total from G26's terms and at worst 1.48e-6 / 2.31e-6 / 3.82e-6 of a tensor's
scale from its best and trained P, Q, PQ2, W; AMR's noise norms 1.20e-7 (relative) from G26's.  8x those stay below the
project's run bars, 1e-5 of the total for loss terms (and, relative, for the noise norms) and 2e-4 of a tensor's scale,
which are therefore the bars.
On the MI355X the runs end 2.01e-7 / 1.54e-7 / 2.11e-7 of the total from G26's terms and at worst 1.07e-6 (item, PQ2) /
3.49e-6 (user, PQ2) / 5.23e-6 (AMR, P) from its tensors, AMR's noise norms 3.28e-7; every one of the 750 / 456 / 750
final lists equals the reference's (716 / 437 / 720 users with a determined ranking).  Only the user-cold run has rows
that no batch gathers (the 60 cold users' rows of P); elsewhere that check runs over an empty set.
G26's best tensors, lists and metrics are the reference's evaluation of the best epoch's model: the reference's own
best_* of P, Q, PQ2, W are the live parameters, which after a run whose best epoch is not its last (VBPR item: epoch 1 of
2) hold the last epoch's values beside the best epoch's content rows (tests/golden/make_golden_g26.py).

One training step (tools/vbpr_step_ab.py: B = 2048, d = 64, content width 16), the trainers' fused step against the same
step written as the restatement in float32 on the GPU (torch autograd, torch.optim.Adagrad / Adam), median of 60
individually timed steps after a warm-up, synchronised at the boundaries, on the MI355X:
    VBPR  toy tables (300 x 500)         fused 1.38 ms   torch 1.45 ms   ratio 1.05
    AMR   toy tables                     fused 1.71 ms   torch 2.39 ms   ratio 1.39
    VBPR  MovieLens-sized (6040 x 3706)  fused 1.40 ms   torch 1.30 ms   ratio 0.92
    AMR   MovieLens-sized                fused 1.57 ms   torch 2.08 ms   ratio 1.32
(a run on a second MI355X: 1.28 / 1.30, 1.63 / 1.82, 1.21 / 1.11, 1.51 / 1.81 ms).  With --batch 16384
the eight times stay where they are (fused 1.46, 1.74, 1.30, 1.69 ms; torch 1.50, 2.13, 1.35, 2.23 ms): up to there both
arms are bound by the host's launches (the plan's grouping of the ids among them), not by the GPU.
"""
import argparse
import functools
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import vbpr_restate as R
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference, metrics_vs_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_LOSS_WORST, F32_GRAD_WORST = 1.29e-7, 3.29e-7               # float32 torch against float64 torch at CASES, all variants
F32_CHUNKS_GRAD_WORST = 4.59e-6                                 # ... the gradients of the "chunks" case
LOSS_BAR, GRAD_BAR, CHUNKS_GRAD_BAR = 8 * F32_LOSS_WORST, 8 * F32_GRAD_WORST, 8 * F32_CHUNKS_GRAD_WORST
EDGE_F32_LOSS_WORST, EDGE_F32_GRAD_WORST = 9.52e-8, 7.97e-7     # ... at the edge cases
EDGE_LOSS_BAR, EDGE_GRAD_BAR = max(8 * EDGE_F32_LOSS_WORST, LOSS_BAR), max(8 * EDGE_F32_GRAD_WORST, GRAD_BAR)
RUN_LOSS_BAR, RUN_TABLE_BAR = 1e-5, 2e-4                  # the project's run bars (see above)
RUNS = [("vbpr", "item"), ("vbpr", "user"), ("amr", "item")]
RUN_IDS = lambda r: "-".join(r)
F32_RUN_LOSS = {"vbpr-item": 1.41e-7, "vbpr-user": 2.20e-7, "amr-item": 1.57e-7}      # float32 torch against G26: terms
F32_RUN_TENSORS = {"vbpr-item": 1.48e-6, "vbpr-user": 2.31e-6, "amr-item": 3.82e-6}   # ... the worst best / trained tensor
F32_RUN_NOISE = 1.20e-7                                                               # ... AMR's noise norms

CASES, IDS, WD1, LMD = R.CASES, R.CASE_IDS, R.WD1, R.CASE_LMD
VARIANTS, VARIANT_IDS = R.VARIANTS, R.VARIANT_IDS


def chunk_rows():
    from coldrec_amd import ops
    return ops.vbpr_chunk_rows()


def grad_bar(case):
    return CHUNKS_GRAD_BAR if case[0] == "chunks" else GRAD_BAR


def _inputs(case, cold_user, adv, **kw):
    return R.inputs(case, cold_user, adv, chunk=chunk_rows(), **kw)


WANT_ALL = dict(want_user=True, want_item=True, want_aux=True, want_h=True, want_h_adv=True, want_hsum=True)


def _fused(inp, wd1, cold_user, lmd=LMD, scale=1.0, **kw):
    """(loss4 on the host, grad_user, grad_item, grad_aux, grad_h, grad_h_adv, grad_hsum)."""
    from coldrec_amd import ops
    P, Q, A, h, h_adv, users, pos, neg = (None if t is None else t.to(DEV) for t in inp)
    plan = ops.vbpr_plan(users, pos, neg)
    out = ops.vbpr(P, Q, A, h, plan, wd1, h_adv=h_adv, lmd=lmd, cold_user=cold_user, scale=scale, **{**WANT_ALL, **kw})
    torch.cuda.synchronize()
    return (None if out[0] is None else out[0].cpu(),) + tuple(out[1:])


def _compare(tag, got, want, loss_bar=None, grad_bar=None):
    loss_bar, grad_bar = LOSS_BAR if loss_bar is None else loss_bar, GRAD_BAR if grad_bar is None else grad_bar
    got = (got[0].numpy(),) + tuple(None if g is None else g.cpu().numpy() for g in got[1:])
    assert all(np.isfinite(g).all() for g in got if g is not None)
    rel, errs = R.distances(got, want)
    print(f"{tag}: loss err / total {rel:.2e}, gradient err / max " + " ".join(f"{e:.2e}" for e in errs))
    assert rel <= loss_bar
    assert max(errs) <= grad_bar


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_matches_float64_restatement(case, variant):
    cold_user, adv = variant
    inp = _inputs(case, cold_user, adv)
    if case[0] == "chunks":
        from coldrec_amd import ops
        plan, c = ops.vbpr_plan(*inp[5:]), chunk_rows()
        for side in ("user", "item"):
            sizes = torch.diff(plan[f"{side}_ptr"])
            per = torch.diff(plan[f"{side}_chunk_ptr"])
            assert (per >= 3).all() and int(((sizes % c) == 1).sum()) >= len(sizes) - 1
    _compare(IDS(case), _fused(inp, WD1, cold_user), R.step(*inp, WD1, cold_user, LMD), grad_bar=grad_bar(case))


@pytest.mark.parametrize("edge", R.EDGE_TAGS, ids=lambda e: VARIANT_IDS(e[0]) + "-" + e[2])
def test_edges(edge):
    (cold_user, adv), k, _ = edge
    tag, inp, wd1, lmd = R.edge_cases(cold_user, adv)[k]
    got = _fused(inp, wd1, cold_user, lmd)
    want = R.step(*inp, wd1, cold_user, lmd)
    _compare(tag, got, want, EDGE_LOSS_BAR, EDGE_GRAD_BAR)
    users, pos, neg = inp[5:]
    B = users.shape[0]
    if tag == "pos-is-neg":                       # x = 0 whatever the rows hold, and Q's two contributions cancel
        i = int(pos[5])
        assert i == int(neg[5]) and np.abs(want[2]).max() > 0
        alone = int((pos == i).sum() + (neg == i).sum()) == 2
        if alone:
            assert np.array_equal(got[2][i].cpu().numpy(), 2 * 2 * np.float32(wd1) * inp[1][i].numpy())
    if tag == "pos-and-neg":
        assert int(pos[0]) == int(neg[1]) == 7
    if tag == "one-user":
        assert len(set(users.tolist())) == 1 and np.count_nonzero(np.abs(want[1]).max(axis=1)) == 1
    if tag == "wd0":
        assert float(got[0][2]) == 0.0
    if tag == "h-zero" and not adv and not cold_user:          # the content tower adds nothing to x, and d A = 0 + R_emb's part
        assert np.allclose(got[3].cpu().numpy(), 2 * wd1 * np.bincount(users.numpy(), minlength=50)[:, None] * inp[2].numpy(),
                           rtol=1e-6, atol=0)
    if tag == "scores-beyond-30":
        P, Q, A, h = (t.double() for t in inp[:4])
        base = (P[users] * (Q[pos] - Q[neg])).sum(1)
        x = base + ((h * (A[pos] - A[neg])).sum(1) if cold_user else (A[users] * (h[:B] - h[B:])).sum(1))
        assert float(x.max()) > 30 and float(x.min()) < -30
    if tag == "one-record":
        assert B == 1
    if tag == "adv-is-plain":
        assert float(got[0][1]) == pytest.approx(lmd * float(got[0][0]), rel=1e-6)
        assert torch.allclose(got[5], got[4] * lmd, rtol=1e-6, atol=0)
    if tag == "lmd-zero":                         # L_adv and every adversarial gradient are exactly 0
        assert float(got[0][1]) == 0.0 and not got[5].any()
        plain = _fused(inp[:4] + [None] + inp[5:], wd1, cold_user, lmd)
        for a, b in zip(got[1:5] + got[6:], plain[1:5] + plain[6:]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("case", [CASES[2], CASES[8]], ids=IDS)
def test_determinism_scale_null_gradients_and_hsum(case, variant):
    cold_user, adv = variant
    inp = _inputs(case, cold_user, adv)
    a, b = _fused(inp, WD1, cold_user), _fused(inp, WD1, cold_user)
    live = [k for k in range(1, 7) if a[k] is not None]
    assert live == ([1, 2, 3, 4, 5, 6] if adv else [1, 2, 3, 4, 6])
    assert torch.equal(a[0], b[0]) and all(torch.equal(a[k], b[k]) for k in live)
    half = _fused(inp, WD1, cold_user, scale=0.5)
    assert torch.equal(half[0], a[0]) and all(torch.equal(a[k] * 0.5, half[k]) for k in live)
    names = ["want_user", "want_item", "want_aux", "want_h", "want_h_adv", "want_hsum"]
    for k in live:                                # an unwanted gradient is None; the others keep their bits
        part = _fused(inp, WD1, cold_user, **{names[k - 1]: False})
        assert part[k] is None and torch.equal(part[0], a[0])
        assert all(torch.equal(part[j], a[j]) for j in live if j != k)
    # grad_hsum = the content gradients summed per distinct cold object in the plan's order
    from coldrec_amd import ops
    plan = ops.vbpr_plan(*(t.to(DEV) for t in inp[5:]))
    own = inp[5] if cold_user else torch.cat(inp[6:])
    assert torch.equal(plan["user_ids" if cold_user else "item_ids"].cpu().long(), torch.unique(own))
    rows = a[4].cpu().double() + (a[5].cpu().double() if adv else 0)
    want = R.owner_sums(rows, own)
    assert a[6].shape == want.shape
    assert float((a[6].cpu().double() - want).abs().max()) <= grad_bar(case) * float(want.abs().max())
    # alone, with every other gradient and the loss NULL: the plain term's part of the full call
    only = _fused(inp[:4] + (None,) + inp[5:], WD1, cold_user, want_user=False, want_item=False, want_aux=False, want_h=False,
                  want_loss=False)
    assert all(t is None for t in only[:6])
    plain = _fused(inp[:4] + (None,) + inp[5:], WD1, cold_user)
    assert torch.equal(only[6], plain[6])
    want = R.owner_sums(a[4].cpu().double(), own)                  # ... = the full call's d H summed per owner
    assert float((only[6].cpu().double() - want).abs().max()) <= grad_bar(case) * float(want.abs().max())


@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
def test_untouched_rows_keep_the_callers_sentinel(variant):
    cold_user, adv = variant
    inp = _inputs((63, 64, 50, 400), cold_user, adv)
    full = _fused(inp, WD1, cold_user)
    sent = lambda t: torch.full(t.shape, -7.0, device=DEV)
    gu, gi, ga, gh = (sent(t) for t in inp[:4])
    kw = dict(grad_h_adv=sent(inp[4])) if adv else {}
    out = _fused(inp, WD1, cold_user, grad_user=gu, grad_item=gi, grad_aux=ga, grad_h=gh, **kw)
    tu, ti = torch.zeros(50, dtype=torch.bool), torch.zeros(400, dtype=torch.bool)
    tu[inp[5]] = True
    ti[inp[6]] = True
    ti[inp[7]] = True
    ta = ti if cold_user else tu
    assert (~tu).any() and (~ti).any()
    for g, t, f in ((gu, tu, full[1]), (gi, ti, full[2]), (ga, ta, full[3])):
        assert (g.cpu()[~t] == -7.0).all() and torch.equal(g.cpu()[t], f.cpu()[t]) and not (f.cpu()[~t] != 0).any()
    assert torch.equal(gh, full[4]) and torch.equal(out[6], full[6])
    if adv:
        assert torch.equal(kw["grad_h_adv"], full[5])


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    case = (2, 4, 11, 13)
    P, Q, A, h, h_adv, users, pos, neg = (t.to(DEV).contiguous() for t in _inputs(case, False, True))
    plan = ops.vbpr_plan(users, pos, neg)
    L = _lib.lib()
    p = lambda t: t.data_ptr()

    def call(d=4, batch=2, ws="ok", item_rows=13, user_rows=11, u_rng=None, i_rng=None, shift=0, cold_user=0, adv=True,
             grad_adv=True):
        space = ops.vbpr_workspace(2, 4, False, plan["n_items"], plan["n_users"], DEV)
        out = [torch.full(t.shape, -7.0, device=DEV) for t in (P, Q, A, h, h_adv, h)] + [torch.full((4,), -7.0, device=DEV)]
        u_rng, i_rng = u_rng or plan["user_range"], i_rng or plan["item_range"]
        ws_ptr, ws_bytes = {"ok": (p(space), space.numel()), "null": (0, space.numel()), "short": (p(space), 16)}[ws]
        outs = [p(t) for t in out]
        if not grad_adv:
            outs[4] = None
        rc = L.crh_vbpr_f32(p(P), user_rows, p(Q), item_rows, p(A), p(h) + shift, p(h_adv) if adv else None, p(plan["users"]),
                            p(plan["pos"]), p(plan["neg"]), u_rng[0], u_rng[1], i_rng[0], i_rng[1], p(plan["item_ids"]),
                            p(plan["item_ptr"]), p(plan["item_occ"]), p(plan["item_chunk_ptr"]), p(plan["item_chunk_own"]),
                            plan["n_items"], plan["n_item_chunks"], p(plan["user_ids"]), p(plan["user_ptr"]),
                            p(plan["user_occ"]), p(plan["user_chunk_ptr"]), p(plan["user_chunk_own"]), plan["n_users"],
                            plan["n_user_chunks"], batch, d, cold_user, 0.01, 1.0, 1.0, *outs, ws_ptr, ws_bytes,
                            _lib.current_stream())
        torch.cuda.synchronize()
        assert all((t == -7.0).all() for t in out)                     # nothing ran
        return rc, L.crh_last_error().decode()

    ARG, WS = -1, -3                                                   # CRH_ERR_ARG, CRH_ERR_WS of include/coldrec_hip.h
    for kw, rc, text in ((dict(d=6), ARG, "multiple of 4"), (dict(d=260), ARG, "multiple of 4"),
                         (dict(batch=0), ARG, "batch = 0"), (dict(ws="null"), WS, "workspace"),
                         (dict(ws="short"), WS, "workspace"), (dict(shift=4), ARG, "16-byte aligned"),
                         (dict(cold_user=1), ARG, "item mode"), (dict(adv=False), ARG, "grad_h_adv without h_adv"),
                         (dict(item_rows=plan["item_range"][1]), ARG, "outside the item table"),
                         (dict(user_rows=plan["user_range"][1]), ARG, "outside the user table"),
                         (dict(u_rng=(-1, 3)), ARG, "outside the user table")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and text in msg, (kw, got_rc, msg)
    assert L.crh_vbpr_workspace_bytes(2, 6, 0, 2, 2) == 0 and L.crh_vbpr_workspace_bytes(2, 260, 0, 2, 2) == 0
    assert L.crh_vbpr_workspace_bytes(0, 4, 0, 1, 1) == 0
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match=r"vbpr: width 260 must be a multiple of 4 in \[4, 256\]"):
        ops.vbpr(z(11, 260), z(13, 260), z(11, 260), z(4, 260), plan, WD1)
    with pytest.raises(RuntimeError, match=r"vbpr: width 6 must be a multiple of 4"):
        ops.vbpr(z(11, 6), z(13, 6), z(11, 6), z(4, 6), plan, WD1)
    with pytest.raises(RuntimeError, match="h_adv is item mode's only"):
        ops.vbpr(P, Q, z(13, 4), z(2, 4), plan, WD1, h_adv=z(2, 4), cold_user=True)
    with pytest.raises(RuntimeError, match="item mode takes tables"):
        ops.vbpr(P, Q, A, h, plan, WD1, cold_user=True)
    with pytest.raises(RuntimeError, match="vbpr: ids lie outside the tables"):
        ops.vbpr(P[:plan["user_range"][1]].contiguous(), Q, A[:plan["user_range"][1]].contiguous(), h, plan, WD1)
    with pytest.raises(RuntimeError, match="vbpr: ids lie outside the tables"):
        ops.vbpr(P, Q[:plan["item_range"][1]].contiguous(), A, h, plan, WD1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.vbpr(P.cpu(), Q.cpu(), A.cpu(), h.cpu(), plan, WD1)
    with pytest.raises(RuntimeError, match="contiguous 2-D float32"):
        ops.vbpr(P.double(), Q, A, h, plan, WD1)
    with pytest.raises(RuntimeError, match="grad_hsum must be"):
        ops.vbpr(P, Q, A, h, plan, WD1, grad_hsum=z(plan["n_items"] + 1, 4))
    with pytest.raises(RuntimeError, match="nothing to compute"):
        ops.vbpr(P, Q, A, h, plan, WD1, want_user=False, want_item=False, want_aux=False, want_h=False, want_loss=False)
    with pytest.raises(RuntimeError, match="integer tensors"):
        ops.vbpr_plan(users.float(), pos, neg)


# ---- the trainers' autograd operator ---------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("cdim", [16, 7])
def test_autograd_operator_matches_restatement_through_the_content_projection(cdim, variant):
    """The trainers' autograd operator fed by content @ W (and (content + shift) @ W) against the float64 restatement
    through torch.autograd.grad with grad_out = 0.7: W receives its gradient from both projections; the tables' land in
    the caller's buffers, unscaled."""
    from coldrec_amd import ops
    from coldrec_amd.model.VBPR import _FusedLoss
    cold_user, adv = variant
    P, Q, A, _, _, users, pos, neg = _inputs((96, 32, 40, 90), cold_user, False)
    gen = torch.Generator().manual_seed(5 + cdim)
    content = torch.randn(40 if cold_user else 90, cdim, generator=gen)
    W0 = torch.randn(cdim, 32, generator=gen) * 0.3
    src = users if cold_user else torch.cat([pos, neg])
    shift = torch.randn(src.shape[0], cdim, generator=gen) * 0.1

    def grads(dt, dev, fused):
        W = torch.nn.Parameter(W0.to(dt).to(dev))
        Pd, Qd, Ad = (t.to(dt).to(dev) for t in (P, Q, A))
        rows = content.to(dt).to(dev)[src.to(dev)]
        h = rows @ W
        h_adv = (rows + shift.to(dt).to(dev)) @ W if adv else None
        if fused:
            bufs = [torch.zeros_like(t) for t in (Pd, Qd, Ad)]
            plan = ops.vbpr_plan(users.to(dev), pos.to(dev), neg.to(dev))
            ws = ops.vbpr_workspace(96, 32, cold_user, plan["n_items"], plan["n_users"], dev)
            total, terms = _FusedLoss.apply(h, h_adv, Pd, Qd, Ad, plan, WD1, LMD, cold_user, *bufs, ws, False)
            assert float(total.detach()) == float(terms[3])
            tables = [g.double().cpu().numpy() for g in bufs]
        else:
            Pd, Qd, Ad = Pd.requires_grad_(), Qd.requires_grad_(), Ad.requires_grad_()
            terms = R.loss_terms(Pd, Qd, Ad, h, users, pos, neg, WD1, cold_user, h_adv, LMD)
            total = terms[3]
            tables = [x.numpy() for x in torch.autograd.grad(total, (Pd, Qd, Ad), retain_graph=True)]
        got = torch.autograd.grad(total, (W,), grad_outputs=torch.tensor(0.7, dtype=dt, device=dev))
        return np.array([float(t.detach()) for t in terms]), [x.double().cpu().numpy() for x in got] + tables

    terms, got = grads(torch.float32, DEV, True)
    want_terms, want = grads(torch.float64, "cpu", False)
    rel = np.abs(terms - want_terms).max() / want_terms[3]
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    print(f"autograd: loss err / total {rel:.2e}, gradient err / max {errs}")
    # the float32 content projection and the kernel, each within its bar of the float64 value
    assert rel <= 2 * LOSS_BAR and max(errs) <= 2 * GRAD_BAR
    assert all(np.abs(a).max() > 0 for a in got)


# ---- whole runs against G26 --------------------------------------------------------------------------------------------

def _cfg(data, device=DEV, **kw):
    a = dict(dataset="toy", model="VBPR", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, p_emb=list(R.P_EMB), p_ctx=list(R.P_CTX), eps=R.EPS, lmd=R.LMD)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def content_of(data, cold):
    return np.asarray(data.mapped_user_content if cold == "user" else data.mapped_item_content, np.float32)


def write_loaded(fx, where, which, cold, data):
    """The files a run of the fixture loads, under where/emb: VBPR the backbone's tables, AMR VBPR's five (item_emb_aux,
    which AMR reads for its shape only, rebuilt as content @ W)."""
    (where / "emb").mkdir(exist_ok=True)
    stem = where / "emb"
    if which == "vbpr":
        torch.save(torch.from_numpy(fx["loaded_U"]), stem / f"toy_cold_{cold}_MF_user_emb.pt")
        torch.save(torch.from_numpy(fx["loaded_V"]), stem / f"toy_cold_{cold}_MF_item_emb.pt")
        return
    five = {k: torch.from_numpy(fx["loaded_" + k]) for k in ("user_emb_main", "item_emb_main", "user_emb_aux", "w_value")}
    five["item_emb_aux"] = torch.from_numpy(content_of(data, cold)) @ five["w_value"]
    for k, f in zip(("user_emb_main", "item_emb_main", "user_emb_aux", "item_emb_aux", "w_value"), R.FILES):
        torch.save(five[k], stem / f"toy_cold_{cold}_VBPR_{f}.pt")


@functools.lru_cache(maxsize=None)
def restated_run(which, cold, dtype):
    """The restatement's whole run, computed once per run and dtype and shared (callers leave it unchanged).  On one
    thread: torch's multi-threaded CPU reductions change their order from run to run; one thread gives the same bits."""
    fx = load_golden(f"g26_{which}_{cold}.npz")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return R.run(R.toy_data(cold), dtype, cold == "user", R.start_of(fx, which == "amr"), amr=which == "amr")
    finally:
        torch.set_num_threads(threads)


def _run(where, which, cold, **kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle), with ``where`` --
    whose ./emb holds the fixture's loaded tensors -- as the working directory."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    data = R.toy_data(cold)
    cwd = os.getcwd()
    os.chdir(where)
    try:
        set_seed(2024, True)
        tr = AVAILABLE_MODELS[which.upper()](_cfg(data, model=which.upper(), cold_object=cold, **kw))
        if which == "amr":
            tr.model.noise_log = []
        tr.run()
    finally:
        os.chdir(cwd)
    return tr


def _four(tr):
    m = tr.model
    return [t.detach().cpu().numpy() for t in (m.P.weight, m.Q.weight, m.PQ2.weight, m.W)]


def _best_four(tr, cold):
    return [t.cpu().numpy() for t in (tr.user_emb_main, tr.item_emb_main, tr.item_emb_aux if cold == "user" else tr.user_emb_aux,
                                      tr.w_value)]


@pytest.fixture(scope="module", params=RUNS, ids=RUN_IDS)
def toy_run(request, tmp_path_factory):
    which, cold = request.param
    where = tmp_path_factory.mktemp(f"{which}_{cold}")
    fx = load_golden(f"g26_{which}_{cold}.npz")
    write_loaded(fx, where, which, cold, R.toy_data(cold))
    return which, cold, fx, _run(where, which, cold), where


def test_run_matches_reference_g26(toy_run):
    """Bars: RUN_LOSS_BAR / RUN_TABLE_BAR above."""
    which, cold, fx, tr, _ = toy_run
    amr, cold_user = which == "amr", cold == "user"
    best, trained = _best_four(tr, cold), _four(tr)
    assert tr.batch_losses.shape == (16, 4 if amr else 3) and tr.LOSS_TERMS[-1] == "batch_loss"
    norms = np.array([float(x) for x in tr.model.noise_log], np.float64) if amr else None
    rel, e_best, e_trained, e_noise = R.run_distances(fx, tr.batch_losses, best, trained, norms)
    print(f"{which} {cold}: worst term difference to G26 over the total {rel:.2e}; best P, Q, PQ2, W differ by " +
          " ".join(f"{e:.2e}" for e in e_best) + " of their scale, trained by " + " ".join(f"{e:.2e}" for e in e_trained) +
          (f"; noise norms by {e_noise:.2e}" if amr else ""))
    assert rel <= RUN_LOSS_BAR and max(e_best) <= RUN_TABLE_BAR and max(e_trained) <= RUN_TABLE_BAR
    if amr:
        assert norms.shape == (32,) and e_noise <= RUN_LOSS_BAR
    assert np.allclose(tr.batch_losses[:, -1], tr.batch_losses[:, :-1].sum(1), rtol=1e-6)
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    # the published five and the ranked pair
    content = content_of(tr.data, cold)
    aux = (tr.user_emb_aux if cold_user else tr.item_emb_aux).cpu().numpy()
    assert np.abs(aux - content.astype(np.float64) @ best[3].astype(np.float64)).max() <= 1e-5 * np.abs(aux).max()
    assert torch.equal(tr.user_emb, torch.cat([tr.user_emb_main, tr.user_emb_aux], 1))
    assert torch.equal(tr.item_emb, torch.cat([tr.item_emb_main, tr.item_emb_aux], 1))
    touched = restated_run(which, cold, torch.float32)["touched"]
    first = restated_run(which, cold, torch.float32)["init"]
    for k, name, rows in ((0, "P", ~touched[0]), (1, "Q", ~touched[1]), (2, "PQ2", ~touched[1 if cold_user else 0])):
        print(f"{which} {cold}: {int(rows.sum())} rows of {name} were gathered by no batch")
        assert np.array_equal(trained[k][rows], first[k][rows])      # rows no batch touched: no step moved them
        assert np.abs(trained[k][~rows] - first[k][~rows]).max() > 1e-3
    got_lists = {}
    for t in ("all", "cold", "warm"):
        c, _s, i = tr._topk_arrays(tr._sets("test", t), t)
        assert np.array_equal(c["users_int"].cpu().numpy(), fx[f"{t}_users_int"])
        got_lists[t] = i
    ranked = [t.cpu().numpy() for t in (tr.user_emb, tr.item_emb)]
    same, det, total = lists_vs_reference(R.ranked_of(fx, content, cold_user), ranked, got_lists, min_frac=0.5)
    print(f"{which} {cold}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    results = dict(overall=tr.overall_test_results, cold=tr.cold_test_results, warm=tr.warm_test_results)
    metrics_vs_reference(results, fx, same == total, tr.bestPerformance[1]["NDCG"])
    lines = json.loads(str(fx["loss_lines"]))
    assert len(lines) == 2 and [float(l.split("batch_loss:")[1]) for l in lines] == pytest.approx(
        list(tr.batch_losses[[0, 8], -1]), rel=RUN_LOSS_BAR)


def test_second_run_is_bit_identical(toy_run):
    which, cold, _, a, where = toy_run
    b = _run(where, which, cold)
    assert np.array_equal(a.batch_losses, b.batch_losses)
    assert torch.equal(a.user_emb, b.user_emb) and torch.equal(a.item_emb, b.item_emb)
    for x, y in zip(_four(a), _four(b)):
        assert np.array_equal(x, y)
    if which == "amr":
        assert torch.equal(a.model.noise, b.model.noise) and a.model.noise.abs().max() > 0


def test_cli_chain_vbpr_then_amr(tmp_path, monkeypatch):
    """MF, then our VBPR with --save_emb, then our AMR from those files, through the CLI."""
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "MF", "--make_synthetic", "toy"] + common) is None
    main(["--model", "MF", "--epochs", "1"] + common)
    pay = main(["--model", "VBPR", "--epochs", "2", "--p_emb", "0.05,0.01"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "VBPR" / "history.txt").is_file()
    shapes = {}
    for which in ("VBPR", "AMR"):
        if which == "AMR":
            pay = main(["--model", "AMR", "--epochs", "2", "--p_emb", "0.05,0.01", "--eps", "0.1", "--lmd", "1"] + common)
            assert set(pay) == {"10", "20"}
        for f in R.FILES:
            t = torch.load(tmp_path / "emb" / f"toy_cold_item_{which}_{f}.pt", map_location="cpu")
            assert torch.isfinite(t).all() and t.abs().max() > 0 and t.shape[1] == 64
            assert shapes.setdefault(f, t.shape) == t.shape
    a, b = (torch.load(tmp_path / "emb" / f"toy_cold_item_{w}_W.pt", map_location="cpu") for w in ("VBPR", "AMR"))
    assert not torch.equal(a, b)                   # AMR trained on from VBPR's projection
