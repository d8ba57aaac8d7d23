"""GPU: DUIF's fused projected-BPR step (csrc/duif.hip) against the float64 restatement (tests/duif_restate.py, itself
pinned to the reference's runs by tests/test_duif.py), for cold items and cold users: the shapes where it can go wrong,
the edges, the contracts, the argument errors, the trainer's autograd operator, and whole DUIF runs against G28.

Bars of the kernel against the float64 restatement: 8x the worst distance of the float32 torch formula (CPU) from the
float64 one at the same cases, both modes; the factor 8 is the project's margin for a different but equally valid fp32
summation order.  Loss terms are measured as error over the TOTAL loss, gradients (and H) as error over their maximum.
Measured on the CPU (tests/test_duif.py prints them again and holds them to a factor of 2):
    cases:  loss terms, error / total  worst 1.40e-7 ("chunks", item)           -> LOSS_BAR = 1.12e-6
            gradients and H, error / maximum worst 6.19e-7 (B512-d128-c300, item, H) -> GRAD_BAR = 4.95e-6
            ... in the "chunks" case, where every owner's gradient row is what is left of 513 or more rows that largely
            cancel, worst 1.60e-6 (user, d T; it moves by a tenth from run to run with torch's threads) ->
            CHUNKS_GRAD_BAR = 1.28e-5
    edges:  each edge has its own pair (EDGE_F32_WORST), the worse of the two modes; its bars are 8x these or the cases'
            bars, whichever is larger.  Only two edges exceed the cases' bars: scores beyond +-30 (gradients 1.06e-6 ->
            8.48e-6) and pos == neg in every record (gradients 1.49e-5 -> 1.19e-4: autograd forms g p - g n at the size
            of g p where only the norms' part, a thousandth of it, is left; the kernel forms p - n = 0 first).
On the MI355X the kernel measures 1.88e-7 (loss terms, B7-d256-c7 item) and 6.19e-7 (H, B512-d128-c300 item; gradients
4.81e-7) at worst over the cases, 1.40e-7 and 3.84e-7 in the "chunks" case; over the edges 1.17e-7 (loss terms, first and
last rows, user) and 1.49e-5 (d W, pos == neg, item: the float32 formula's own figure; user mode's d T 5.16e-6; 8.0e-7 at worst at the other
edges).  The
autograd operator through the encoder's loss(): 1.04e-7 and 3.07e-7.

Whole runs against G28 (item, user): plain float32 torch on the CPU on one thread (tests/test_duif.py) ends 8.45e-8 /
8.49e-8 of the total from G28's terms and at worst 1.18e-7 / 6.13e-7 of a tensor's scale from its best and trained free
table and W; all 750 / 456 lists equal the reference's, with 739 / 447 users' rankings determined (item: 222 of 227, 283
of 287, 234 of 236 in the all / cold / warm settings; user: 210 of 214, 29 of 30, 208 of 212 -- the condition of
min_frac = 0.5 holds in every setting).  8x those stay below the project's run bars, 1e-5 of the total for loss terms and
2e-4 of a tensor's scale, which are therefore the bars.
On the MI355X the runs end 1.69e-7 / 1.71e-7 of the total from G28's terms; W and the projected table at worst 5.83e-7 /
1.16e-7 from G28's; the free table 1.50e-4 (item) / 1.77e-5 (user) of its scale, in ONE element each: (239, 24) of the
item run's 19 200 and (101, 15) of the user run's 32 000; every other element lies within 1e-5 of the scale (printed by
the run test).  The float64 restatement on the CPU stands 5.25e-5 / 7.24e-6 from G28 in the same tables, and all of the
item run's distance sits in the same element (239, 24), every other one within 1e-6 absolute.  Supposed, not shown, of
that element: its first gradients nearly cancel, and Adam, which divides an element's summed gradient by its own size,
carries their rounding into its step.  Every one of the 750 / 456 final lists equals the reference's (734 /
447 users with a determined ranking).  No row of either free table goes ungathered, so that check runs over an empty set.
G28's best tensors, lists and metrics are the reference's evaluation of the best epoch's model: the reference's own
best_* of the free table is the live parameter, which after a run whose best epoch is not its last (both runs: epoch 1
of 2) holds the last epoch's values beside the best epoch's projected table (tests/golden/make_golden_g28.py).

One training step including Adam (tools/duif_step_ab.py: B = 2048, d = 64; the three arms interleaved in one process,
median of 60 individually timed steps after a warm-up, synchronised at the boundaries), on the MI355X, ms; (a) this
trainer's fused step, (b) the reference's formulation (the whole content table projected per batch), (c) torch
gathering first; a second run of the process in brackets:
    toy (300 x 500, c = 16)             item  (a) 0.81 (0.85)  (b) 0.94 (1.03)  (c) 0.86 (0.94)
                                        user  (a) 0.78 (0.86)  (b) 0.88 (1.02)  (c) 0.82 (0.94)
    MovieLens-sized (6040 x 3706, 206)  item  (a) 0.77 (0.86)  (b) 0.86 (1.02)  (c) 0.77 (0.93)
                                        user  (a) 0.79 (0.84)  (b) 0.86 (0.95)  (c) 0.78 (0.86)
    CiteULike-sized (5551 x 16980, 300) item  (a) 0.77 (0.81)  (b) 0.92 (0.99)  (c) 0.77 (0.84)
                                        user  (a) 0.79 (0.82)  (b) 0.85 (0.93)  (c) 0.78 (0.84)
    10^6 content rows (c = 128)         item  (a) 0.79 (0.82)  (b) 2.58 (2.64)  (c) 0.79 (0.85)
                                        user  (a) 0.81 (0.82)  (b) 2.44 (2.51)  (c) 0.81 (0.85)
(a) does not grow with the content rows; (b) does: 3.0 - 3.3x of (a) at 10^6 rows, 1.1 - 1.2x below.  Against (c) the
fused step only ties (c / a = 0.99 - 1.11; it lost once, by 1 %, MovieLens-sized user mode, first run): both arms are
bound by the host's launches -- supposed from the times' indifference to c and to d c, not profiled.
"""
import argparse
import json
import os
import types

import numpy as np
import pytest
import torch

from tests import duif_restate as R
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference, metrics_vs_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_LOSS_WORST, F32_GRAD_WORST = 1.40e-7, 6.19e-7               # float32 torch against float64 torch at CASES, both modes
F32_CHUNKS_GRAD_WORST = 1.60e-6                                 # ... the gradients of the "chunks" case
LOSS_BAR, GRAD_BAR, CHUNKS_GRAD_BAR = 8 * F32_LOSS_WORST, 8 * F32_GRAD_WORST, 8 * F32_CHUNKS_GRAD_WORST
# ... at the edge cases, each edge its own: (loss terms, gradients), the worse of the two modes
EDGE_F32_WORST = {"pos-is-neg": (5.57e-8, 1.49e-5), "scores-beyond-30": (1.68e-8, 1.06e-6), "w-zero": (5.41e-8, 2.61e-7),
                  "free-zero": (4.44e-8, 2.90e-7), "first-and-last": (9.35e-8, 2.50e-7), "pos-and-neg": (1.62e-7, 2.40e-7)}
EDGE_BARS = {k: (max(8 * l, LOSS_BAR), max(8 * g, GRAD_BAR)) for k, (l, g) in EDGE_F32_WORST.items()}
RUN_LOSS_BAR, RUN_TABLE_BAR = 1e-5, 2e-4                        # the project's run bars (see above)
F32_RUN_LOSS = {"item": 8.45e-8, "user": 8.49e-8}               # float32 torch against G28: terms
F32_RUN_TENSORS = {"item": 1.18e-7, "user": 6.13e-7}            # ... the worst best / trained tensor

CASES, IDS, MODES, MODE_IDS, REG = R.CASES, R.CASE_IDS, R.MODES, R.MODE_IDS, R.CASE_REG


def chunk_rows():
    from coldrec_amd import ops
    return ops.duif_chunk_rows()


def grad_bar(case):
    return CHUNKS_GRAD_BAR if case[0] == "chunks" else GRAD_BAR


def _inputs(case, cold_user, **kw):
    return R.inputs(case, cold_user, chunk=chunk_rows(), **kw)


def off16(t):
    """t on the device in storage that starts 4 bytes past a 16-byte boundary: a content row starts at any address."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def _fused(inp, reg, cold_user, scale=1.0, **kw):
    """(loss3 on the host, grad_table, grad_w, H)."""
    from coldrec_amd import ops
    T, C, W, users, pos, neg = inp
    T, W, users, pos, neg = (t.to(DEV) for t in (T, W, users, pos, neg))
    plan = ops.duif_plan(users, pos, neg, cold_user)
    out = ops.duif(T, off16(C), W, plan, reg, cold_user=cold_user, scale=scale, **{**dict(want_h=True), **kw})
    torch.cuda.synchronize()
    return (out[0].cpu(),) + tuple(out[1:])


def _compare(tag, got, want, loss_bar=None, grad_bar=None):
    loss_bar, grad_bar = LOSS_BAR if loss_bar is None else loss_bar, GRAD_BAR if grad_bar is None else grad_bar
    got = (got[0].numpy(),) + tuple(None if g is None else g.cpu().numpy() for g in got[1:])
    assert all(np.isfinite(g).all() for g in got if g is not None)
    rel, errs = R.distances(got, want)
    print(f"{tag}: loss err / total {rel:.2e}, d T, d W, H err / max " + " ".join(f"{e:.2e}" for e in errs))
    assert rel <= loss_bar
    assert max(errs) <= grad_bar


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_matches_float64_restatement(case, cold_user):
    from coldrec_amd import ops
    inp = _inputs(case, cold_user)
    B, (d, c) = inp[3].shape[0], case[1:3]
    if case[0] == "chunks":
        plan, ch = ops.duif_plan(*inp[3:], cold_user), chunk_rows()
        sizes, per = torch.diff(plan["own_ptr"]), torch.diff(plan["own_chunk_ptr"])
        assert (per >= 3).all() and int(((sizes % ch) == 1).sum()) >= len(sizes) - 1 and len(sizes) == (5 if cold_user else 3)
    if isinstance(case[0], tuple):
        want = {"1": 1, "2": 2, "chunk+1": ops.duif_part_chunk() + 1}[case[0][1]]
        rows = B if cold_user else 2 * B
        assert ops.duif_parts(rows, d, c) == want
        if want == 1:                                               # the boundary: one more record makes a second partial
            assert ops.duif_parts(rows + (1 if cold_user else 2), d, c) == 2
    _compare(IDS(case) + " " + MODE_IDS(cold_user), _fused(inp, REG, cold_user), R.step(*inp, REG, cold_user),
             grad_bar=grad_bar(case))


@pytest.mark.parametrize("edge", R.EDGE_TAGS, ids=lambda e: MODE_IDS(e[0]) + "-" + e[2])
def test_edges(edge):
    cold_user, k, _ = edge
    tag, inp, reg = R.edge_cases(cold_user)[k]
    got = _fused(inp, reg, cold_user)
    want = R.step(*inp, reg, cold_user)
    EDGE_LOSS_BAR, EDGE_GRAD_BAR = EDGE_BARS[tag]
    _compare(tag, got, want, EDGE_LOSS_BAR, EDGE_GRAD_BAR)
    T, C, W, users, pos, neg = inp
    B = users.shape[0]
    if tag == "pos-is-neg":
        # x = 0 in every record whatever the rows hold; without the norms' part the BPR gradients cancel.  Exactly, where
        # a record cancels in itself: g (p - n) of the record's own row (item mode d T, user mode d H and so d W).  The
        # other two are sums of + g u and - g u over different places of one fixed order, which cancel to rounding.
        assert torch.equal(pos, neg) and float(got[0][0]) == pytest.approx(-np.log(1e-5 + 0.5), rel=1e-6)
        bare = _fused(inp, 0.0, cold_user)
        assert float(bare[0][1]) == 0.0
        exact, rounded = (bare[2], bare[1]) if cold_user else (bare[1], bare[2])
        assert not exact.any()
        # ... to rounding: |g| <= 0.5 / B, so the 2 B terms' magnitudes add up to max|u| (x max|C| in d W) at most, and the
        # error of a float32 sum of them is a few 2^-24 of that: far inside the edges' gradient bar of it
        top = float(got[3].abs().max()) if cold_user else float(T.abs().max()) * float(C.abs().max())
        assert float(rounded.abs().max()) <= EDGE_GRAD_BAR * top
        assert np.abs(want[1]).max() > 0 and np.abs(want[2]).max() > 0                      # the norms' parts remain
    if tag == "scores-beyond-30":
        x = torch.from_numpy(want[3])
        u = T.double()[users] if not cold_user else x
        p, n = (x[:B], x[B:]) if not cold_user else (T.double()[pos], T.double()[neg])
        s = (u * (p - n)).sum(1)
        assert float(s.max()) > 30 and float(s.min()) < -30
    if tag == "w-zero":                               # H and its norms are zero: no NaN, W's gradient is the BPR part alone
        assert not got[3].any() and torch.isfinite(got[2]).all() and torch.isfinite(got[1]).all()
        if cold_user:                                 # u = 0: x = 0 and d T = the norms' part alone
            assert float(got[0][0]) == pytest.approx(-np.log(1e-5 + 0.5), rel=1e-6)
    if tag == "free-zero":
        assert not T.any() and torch.isfinite(got[1]).all() and torch.isfinite(got[2]).all()
        if not cold_user:                             # u = 0: the projected rows' gradient is their norms' part alone
            assert float(got[0][0]) == pytest.approx(-np.log(1e-5 + 0.5), rel=1e-6)
    if tag == "first-and-last":
        nu, ni = R.EDGE_BASE[3:]
        assert {0, nu - 1} <= set(users.tolist()) and {0, ni - 1} <= set(pos.tolist()) and {0, ni - 1} <= set(neg.tolist())
        rows = got[1].cpu()
        assert rows[0].any() and rows[-1].any()
    if tag == "pos-and-neg":
        assert int(pos[0]) == int(neg[1]) == 7


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [CASES[2], CASES[6]], ids=IDS)
def test_determinism_scale_null_gradients_and_projected_rows(case, cold_user):
    inp = _inputs(case, cold_user)
    a, b = _fused(inp, REG, cold_user), _fused(inp, REG, cold_user)
    assert all(torch.equal(x, y) for x, y in zip(a, b))               # all four outputs, bit for bit
    half = _fused(inp, REG, cold_user, scale=0.5)
    assert torch.equal(half[0], a[0]) and torch.equal(half[3], a[3])
    assert torch.equal(a[1] * 0.5, half[1]) and torch.equal(a[2] * 0.5, half[2])
    names = ["want_table", "want_w", "want_h"]
    for k in (1, 2, 3):                               # an unwanted output is None; the others keep their bits
        part = _fused(inp, REG, cold_user, **{names[k - 1]: False})
        assert part[k] is None and all(torch.equal(part[j], a[j]) for j in range(4) if j != k)
    T, C, W, users, pos, neg = inp
    touched = torch.zeros(T.shape[0], dtype=torch.bool)
    for t in ((pos, neg) if cold_user else (users,)):
        touched[t] = True
    assert (~touched).any() and not a[1].cpu()[~touched].any() and a[1].cpu()[touched].abs().sum(1).gt(0).all()
    ids = users if cold_user else torch.cat([pos, neg])
    want = C.double()[ids] @ W.double().T
    assert a[3].shape == want.shape
    assert float((a[3].cpu().double() - want).abs().max()) <= GRAD_BAR * float(want.abs().max())


def test_untouched_rows_keep_the_callers_sentinel():
    inp = _inputs(CASES[2], False)
    full = _fused(inp, REG, False)
    gt = torch.full(inp[0].shape, -7.0, device=DEV)
    gw = torch.full(inp[2].shape, -7.0, device=DEV)
    out = _fused(inp, REG, False, grad_table=gt, grad_w=gw)
    touched = torch.zeros(inp[0].shape[0], dtype=torch.bool)
    touched[inp[3]] = True
    assert out[1] is gt and out[2] is gw and torch.equal(gw, full[2])
    assert (gt.cpu()[~touched] == -7.0).all() and torch.equal(gt.cpu()[touched], full[1].cpu()[touched])


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    case = (2, 4, 5, 11, 13)
    T, C, W, users, pos, neg = (t.to(DEV).contiguous() for t in _inputs(case, False))
    plan = ops.duif_plan(users, pos, neg, False)
    L = _lib.lib()
    p = lambda t: t.data_ptr()

    def call(d=4, c=5, batch=2, ws="ok", table_rows=11, content_rows=13, f_rng=None, c_rng=None, shift=0, wshift=0, reg=0.01,
             scale=1.0, table=True, n_own=None):
        space = ops.duif_workspace(2, 4, 5, False, plan["n_own"], DEV)
        out = [torch.full(s, -7.0, device=DEV) for s in (T.shape, W.shape, (4, 4), (3,))]
        f_rng, c_rng = f_rng or plan["user_range"], c_rng or plan["item_range"]
        ws_ptr, ws_bytes = {"ok": (p(space), space.numel()), "null": (0, space.numel()), "short": (p(space), 16)}[ws]
        rc = L.crh_duif_f32(p(T) + shift if table else None, table_rows, p(C), content_rows, c, p(W) + wshift, p(plan["users"]),
                            p(plan["pos"]), p(plan["neg"]), f_rng[0], f_rng[1], c_rng[0], c_rng[1], p(plan["own_ids"]),
                            p(plan["own_ptr"]), p(plan["own_occ"]), p(plan["own_chunk_ptr"]), p(plan["own_chunk_own"]),
                            plan["n_own"] if n_own is None else n_own, plan["n_own_chunks"], batch, d, 0, reg, scale,
                            *[p(t) for t in out], ws_ptr, ws_bytes, _lib.current_stream())
        torch.cuda.synchronize()
        assert all((t == -7.0).all() for t in out)                     # nothing ran
        return rc, L.crh_last_error().decode()

    ARG, WS = -1, -3                                                   # CRH_ERR_ARG, CRH_ERR_WS of include/coldrec_hip.h
    for kw, rc, text in ((dict(table=False), ARG, "NULL"), (dict(d=6), ARG, "multiple of 4"), (dict(d=260), ARG, "multiple of 4"),
                         (dict(c=0), ARG, "c = 0"), (dict(c=4097), ARG, "c = 4097"), (dict(batch=0), ARG, "batch = 0"),
                         (dict(ws="null"), WS, "workspace"), (dict(ws="short"), WS, "workspace"),
                         (dict(shift=4), ARG, "16-byte aligned"), (dict(wshift=4), ARG, "16-byte aligned"),
                         (dict(reg=float("nan")), ARG, "finite"), (dict(scale=float("inf")), ARG, "finite"),
                         (dict(n_own=3), ARG, "n_own = 3"),
                         (dict(table_rows=plan["user_range"][1]), ARG, "outside the table"),
                         (dict(content_rows=plan["item_range"][1]), ARG, "outside the content"),
                         (dict(f_rng=(-1, 3)), ARG, "outside the table"), (dict(c_rng=(0, 13)), ARG, "outside the content")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and text in msg, (kw, got_rc, msg)
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match=r"duif: width 260 must be a multiple of 4 in \[4, 256\]"):
        ops.duif(z(11, 260), C, z(260, 5), plan, REG)
    with pytest.raises(RuntimeError, match=r"duif: width 6 must be a multiple of 4"):
        ops.duif(z(11, 6), C, z(6, 5), plan, REG)
    with pytest.raises(RuntimeError, match="the projection must be"):
        ops.duif(T, C, z(5, 4), plan, REG)
    with pytest.raises(RuntimeError, match="other cold object"):
        ops.duif(T, C, W, plan, REG, cold_user=True)
    with pytest.raises(RuntimeError, match="duif: ids lie outside the tables"):
        ops.duif(T[:plan["user_range"][1]].contiguous(), C, W, plan, REG)
    with pytest.raises(RuntimeError, match="duif: ids lie outside the tables"):
        ops.duif(T, C[:plan["item_range"][1]].contiguous(), W, plan, REG)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.duif(T.cpu(), C.cpu(), W.cpu(), plan, REG)
    with pytest.raises(RuntimeError, match="contiguous 2-D float32"):
        ops.duif(T.double(), C, W, plan, REG)
    with pytest.raises(RuntimeError, match="gradient buffers must be"):
        ops.duif(T, C, W, plan, REG, grad_w=z(5, 4))
    with pytest.raises(RuntimeError, match="integer tensors"):
        ops.duif_plan(users.float(), pos, neg, False)


# ---- the trainer's autograd operator ---------------------------------------------------------------------------------

def _cfg(data, device=DEV, **kw):
    a = dict(dataset="toy", model="DUIF", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cdim", [16, 7])
def test_autograd_operator_matches_restatement_through_the_trainers_loss(cdim, cold_user):
    """The encoder's loss() on tensors of the test's own, backward with grad_out = 0.7, against the float64 restatement."""
    from coldrec_amd.model.DUIF import DUIF_Encoder
    nu, ni, d, B = 40, 90, 32, 96
    gen = torch.Generator().manual_seed(11 + cdim + int(cold_user))
    content = torch.randn(nu if cold_user else ni, cdim, generator=gen)
    data = types.SimpleNamespace(user_num=nu, item_num=ni, user_content_dim=cdim, item_content_dim=cdim,
                                 mapped_user_content=content.numpy(), mapped_item_content=content.numpy())
    cold = "user" if cold_user else "item"
    m = DUIF_Encoder(_cfg(data, cold_object=cold, reg=REG).args, data, d, DEV).to(DEV)
    users, pos, neg = (torch.randint(n, (B,), generator=gen) for n in (nu, ni, ni))
    T0, W0 = m.table.detach().cpu().clone(), m.projector.weight.detach().cpu().clone()
    total = m.loss(users.to(DEV), pos.to(DEV), neg.to(DEV))
    assert float(total.detach()) == float(m.last_terms[2])
    got = torch.autograd.grad(total, (m.table, m.projector.weight), grad_outputs=torch.tensor(0.7, device=DEV))
    want = R.step(T0, content, W0, users, pos, neg, REG, cold_user)
    rel = np.abs(m.last_terms.cpu().numpy() - want[0]).max() / want[0][2]
    errs = [float(np.abs(g.double().cpu().numpy() - 0.7 * w).max() / np.abs(0.7 * w).max()) for g, w in zip(got, want[1:3])]
    print(f"autograd c = {cdim} {cold}: loss err / total {rel:.2e}, gradient err / max {errs}")
    assert rel <= LOSS_BAR and max(errs) <= GRAD_BAR
    assert set(m.state_dict()) == {"embedding_dict.user_emb", "embedding_dict.item_emb", f"{cold}_projector.weight"}


# ---- whole runs against G28 --------------------------------------------------------------------------------------------

def _run(where, cold, **kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle), with ``where`` as
    the working directory."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    data = R.toy_data(cold)
    cwd = os.getcwd()
    os.chdir(where)
    try:
        set_seed(2024, True)
        tr = AVAILABLE_MODELS["DUIF"](_cfg(data, cold_object=cold, **kw))
        tr.run()
    finally:
        os.chdir(cwd)
    return tr


def _two(tr):
    return [t.detach().cpu().numpy() for t in (tr.model.table, tr.model.projector.weight)]


@pytest.fixture(scope="module", params=["item", "user"])
def toy_run(request, tmp_path_factory):
    cold = request.param
    where = tmp_path_factory.mktemp("duif_" + cold)
    return cold, load_golden(f"g28_duif_{cold}.npz"), _run(where, cold, save_emb=True), where


def test_run_matches_reference_g28(toy_run):
    """Bars: RUN_LOSS_BAR / RUN_TABLE_BAR above."""
    cold, fx, tr, where = toy_run
    cold_user = cold == "user"
    assert tr.batch_losses.shape == (16, 3) and tr.LOSS_TERMS == ("bpr", "reg", "batch_loss")
    assert np.allclose(tr.batch_losses[:, -1], tr.batch_losses[:, :-1].sum(1), rtol=1e-6)
    free, proj = (tr.item_emb, tr.user_emb) if cold_user else (tr.user_emb, tr.item_emb)
    trained = _two(tr)
    # (the best epoch's W is not kept by the trainer; its projected table is, and is compared with G28's below)
    rel, _, e_trained = R.run_distances(fx, cold_user, tr.batch_losses, (), trained)
    dist = lambda t, w: float(np.abs(t.cpu().numpy().astype(np.float64) - w).max() / np.abs(w).max())
    e_best = [dist(free, R.best_of(fx, cold_user)[0]), dist(proj, fx["best_proj"])]
    print(f"DUIF {cold}: worst term difference to G28 over the total {rel:.2e}; best free and projected tables differ by " +
          " ".join(f"{e:.2e}" for e in e_best) + " of their scale, the trained table and W by " +
          " ".join(f"{e:.2e}" for e in e_trained))
    far = np.abs(trained[0].astype(np.float64) - R.trained_of(fx, cold_user)[0]) > 1e-5 * np.abs(R.trained_of(fx, cold_user)[0]).max()
    print(f"DUIF {cold}: {int(far.sum())} of {far.size} elements of the trained table lie more than 1e-5 of its scale from G28's" +
          (f" (first at {tuple(int(x) for x in np.argwhere(far)[0])})" if far.any() else ""))
    assert rel <= RUN_LOSS_BAR and max(e_best) <= RUN_TABLE_BAR and max(e_trained) <= RUN_TABLE_BAR
    assert tr.epochs_ran == int(fx["epochs_ran"]) == 2 and tr.bestPerformance[0] == int(fx["best_epoch"]) == 1
    # the best epoch's tables are copies: the last epoch moved the live table away from them
    assert free.data_ptr() != tr.model.table.data_ptr() and not torch.equal(free, tr.model.table.detach())
    # the cold side's table is drawn and never trained
    frozen = tr.model.embedding_dict["user_emb" if cold_user else "item_emb"].detach().cpu().numpy()
    assert np.array_equal(frozen, R.init_of(fx, cold_user)[0 if cold_user else 1])
    # dense Adam: a row no batch touched still moved by its moments, if it ever had a gradient; one that never had stays
    touched = R.restated_run(cold, torch.float32)["touched"]
    first = R.init_of(fx, cold_user)[1 if cold_user else 0]
    print(f"DUIF {cold}: {int((~touched).sum())} rows of the free table were gathered by no batch")
    assert np.array_equal(trained[0][~touched], first[~touched]) and np.abs(trained[0][touched] - first[touched]).max() > 1e-3
    got_lists = {}
    for t in ("all", "cold", "warm"):
        c, _s, i = tr._topk_arrays(tr._sets("test", t), t)
        assert np.array_equal(c["users_int"].cpu().numpy(), fx[f"{t}_users_int"])
        got_lists[t] = i
    ranked = [t.cpu().numpy() for t in (tr.user_emb, tr.item_emb)]
    same, det, total = lists_vs_reference(R.ranked_of(fx, cold_user), ranked, got_lists, min_frac=0.5)
    print(f"DUIF {cold}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    results = dict(overall=tr.overall_test_results, cold=tr.cold_test_results, warm=tr.warm_test_results)
    metrics_vs_reference(results, fx, same == total, tr.bestPerformance[1]["NDCG"])
    lines = json.loads(str(fx["loss_lines"]))
    assert len(lines) == 2 and [float(l.split("batch_loss:")[1]) for l in lines] == pytest.approx(
        list(tr.batch_losses[[0, 8], -1]), rel=RUN_LOSS_BAR)
    # --save_emb wrote the published pair, which a later trainer loads as a backbone's tables
    from coldrec_amd.model.FusedLossTrainer import load_backbone_tables
    cwd = os.getcwd()
    os.chdir(where)
    try:
        args = argparse.Namespace(dataset="toy", cold_object=cold, backbone="DUIF")
        loaded = load_backbone_tables("test", args, tr.data, 64)
    finally:
        os.chdir(cwd)
    assert torch.equal(loaded[0], tr.user_emb.cpu()) and torch.equal(loaded[1], tr.item_emb.cpu())


def test_second_run_is_bit_identical(toy_run):
    cold, _, a, where = toy_run
    b = _run(where, cold)
    assert np.array_equal(a.batch_losses, b.batch_losses)
    assert torch.equal(a.user_emb, b.user_emb) and torch.equal(a.item_emb, b.item_emb)
    for x, y in zip(_two(a), _two(b)):
        assert np.array_equal(x, y)


def test_cli_run(tmp_path, monkeypatch):
    """One run of main.py --model DUIF on a synthetic toy dataset."""
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "user", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "DUIF", "--make_synthetic", "toy"] + common) is None
    pay = main(["--model", "DUIF", "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "DUIF" / "history.txt").is_file()
    for side in ("user", "item"):
        t = torch.load(tmp_path / "emb" / f"toy_cold_user_DUIF_{side}_emb.pt", map_location="cpu")
        assert torch.isfinite(t).all() and t.abs().max() > 0 and t.shape[1] == 64
