"""GPU: the fused MTPR loss (csrc/mtpr.hip) and the touched-rows Adagrad (csrc/adagrad.hip) against the float64
restatement (tests/mtpr_restate.py, itself pinned to the reference's runs by tests/test_mtpr.py), in item mode and in user
mode: the shapes where they can go wrong, the edges, the determinism contract, the argument errors, the trainer's
autograd operator, and whole runs against G25.

Bars of the kernel against the float64 restatement: 8x the worst distance of the float32 torch formula (CPU) from the
float64 one at the same cases, both modes.  Loss terms are measured as error over the TOTAL loss, gradients as error over
their maximum.  Measured on the CPU (tests/test_mtpr.py prints them again and holds them to a factor of 2):
    cases:  loss terms, error / total  worst 1.40e-7 (B65-d124, item)     -> LOSS_BAR = 1.12e-6
            gradients, error / maximum worst 1.42e-6 (B1-d4, item, d Q; 2.9e-7 .. 1.1e-6 elsewhere)
                                                                          -> GRAD_BAR = 1.14e-5
    edges:  loss terms worst 1.55e-7, gradients worst 4.19e-6 (scores beyond +-30, item: a dot product's rounding is
            multiplied by the slope of a term far from its tail); the edge bars are 8x these or the cases' bars, whichever
            is larger: 1.24e-6 and 3.35e-5
    Adagrad: float32 torch.optim.Adagrad against the float64 restatement at ADAGRAD_CASES, error over the maximum of p
            and of the accumulator: worst 5.14e-8                         -> ADAGRAD_BAR = 4.1e-7
On the MI355X the kernel measures 8.5e-8 (loss terms, B2048-d64, user) and 9.6e-7 (gradients, B1-d4, item) at worst over
the cases, 1.1e-7 (H = 0, user) and 1.9e-6 (scores beyond +-30, item) over the edges; adagrad_rows 5.8e-8 in one step
and 7.8e-8 after three.

Whole runs against G25: plain float32 torch on the CPU on one thread (tests/test_mtpr.py) ends 2.13e-7 (item) / 1.48e-7
(user) of the total from G25's terms, 3.13e-6 / 1.45e-6 (item: users / items) and 1.07e-6 / 2.42e-6 (user) of the best
tables' scale from its best tables, and at worst 1.60e-5 / 1.28e-5 of a tensor's scale from its five trained tensors
(with more threads torch's CPU reductions change order from run to run and that figure moves between 4e-6 and 3e-5).
8x those stay below the project's run bars, 1e-5 of the total for loss terms and 2e-4 of a table's scale, which are
therefore the bars.
On the MI355X the runs end 2.13e-7 (item) / 1.48e-7 (user) of the total from G25's terms, 2.57e-6 / 1.31e-6 (item) and
1.36e-6 / 4.13e-6 (user) from its best tables and at worst 1.15e-5 (item, P) / 2.69e-5 (user, Q) from its trained
tensors; every one of the 750 / 456 final lists equals the reference's (712 / 434 users with a determined ranking).
In the item-cold run every row of both tables is gathered by some batch, so the check of the rows no batch touched runs
over an empty set there; in the user-cold run it covers the 60 cold users' rows of P.
"""
import argparse
import functools
import json
import types

import numpy as np
import pytest
import torch

from tests import mtpr_restate as R
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference, metrics_vs_reference

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_LOSS_WORST, F32_GRAD_WORST = 1.40e-7, 1.42e-6               # float32 torch against float64 torch at CASES, both modes
LOSS_BAR, GRAD_BAR = 8 * F32_LOSS_WORST, 8 * F32_GRAD_WORST
EDGE_F32_LOSS_WORST, EDGE_F32_GRAD_WORST = 1.55e-7, 4.19e-6     # ... at the edge cases
EDGE_LOSS_BAR, EDGE_GRAD_BAR = max(8 * EDGE_F32_LOSS_WORST, LOSS_BAR), max(8 * EDGE_F32_GRAD_WORST, GRAD_BAR)
F32_ADAGRAD_WORST = 5.14e-8                               # float32 torch.optim.Adagrad against float64 at ADAGRAD_CASES
ADAGRAD_BAR = 8 * F32_ADAGRAD_WORST
RUN_LOSS_BAR, RUN_TABLE_BAR = 1e-5, 2e-4                  # the project's run bars (see above)
F32_RUN_LOSS = dict(item=2.13e-7, user=1.48e-7)           # float32 torch against G25, measured: terms / the total
F32_RUN_BEST = dict(item=(3.13e-6, 1.45e-6), user=(1.07e-6, 2.42e-6))     # ... best user_emb / item_emb over their scale
F32_RUN_TRAINED = dict(item=1.60e-5, user=1.28e-5)        # ... the worst of the trained P, Q, W, weu, wei

MODES = [False, True]
MODE_IDS = lambda m: "user" if m else "item"
CASES, IDS, WD1 = R.CASES, R.CASE_IDS, R.WD1


def chunk_rows():
    from coldrec_amd import ops
    return ops.mtpr_chunk_rows()


def _inputs(case, cold_user, **kw):
    return R.inputs(case, cold_user, chunk=chunk_rows(), **kw)


def _fused(inp, wd1, cold_user, scale=1.0, want=(True,) * 5, **kw):
    from coldrec_amd import ops
    P, Q, h, weu, wei, users, pos, neg = (t.to(DEV) for t in inp)
    plan = ops.mtpr_plan(users, pos, neg)
    out = ops.mtpr(P, Q, h, weu, wei, plan, wd1, cold_user=cold_user, scale=scale, want_user=want[0], want_item=want[1],
                   want_h=want[2], want_weu=want[3], want_wei=want[4], **kw)
    torch.cuda.synchronize()
    return (out[0].cpu(),) + tuple(out[1:])


def _compare(tag, got, want, loss_bar=None, grad_bar=None):
    loss_bar, grad_bar = LOSS_BAR if loss_bar is None else loss_bar, GRAD_BAR if grad_bar is None else grad_bar
    got = (got[0].numpy(),) + tuple(g.cpu().numpy() for g in got[1:])
    assert all(np.isfinite(g).all() for g in got)
    rel, errs = R.distances(got, want)
    print(f"{tag}: loss err / total {rel:.2e}, gradient err / max " + " ".join(f"{e:.2e}" for e in errs))
    assert rel <= loss_bar
    assert max(errs) <= grad_bar


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_matches_float64_restatement(case, cold_user):
    inp = _inputs(case, cold_user)
    if case[0] == "chunks":
        from coldrec_amd import ops
        plan, c = ops.mtpr_plan(*inp[5:]), chunk_rows()
        for side in ("user", "item"):
            sizes = torch.diff(plan[f"{side}_ptr"])
            per = torch.diff(plan[f"{side}_chunk_ptr"])
            assert (per >= 3).all() and int(((sizes % c) == 1).sum()) >= len(sizes) - 1
    _compare(IDS(case), _fused(inp, WD1, cold_user), R.step(*inp, WD1, cold_user))


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("k", range(8), ids=[e[0] for e in R.edge_cases(False)])
def test_edges(k, cold_user):
    tag, inp, wd1 = R.edge_cases(cold_user)[k]
    got = _fused(inp, wd1, cold_user)
    want = R.step(*inp, wd1, cold_user)
    _compare(tag, got, want, EDGE_LOSS_BAR, EDGE_GRAD_BAR)
    users, pos, neg = inp[5:]
    if tag == "pos-is-neg":                       # every t of that record pairs a score with itself or its twin
        assert int(pos[5]) == int(neg[5]) and np.abs(want[2][int(pos[5])]).max() > 0
    if tag == "pos-and-neg":
        assert int(pos[0]) == int(neg[1]) == 7
    if tag == "one-user":
        assert len(set(users.tolist())) == 1 and np.count_nonzero(np.abs(want[1]).max(axis=1)) == 1
    if tag == "wd0":
        assert float(got[0][4]) == 0.0
    if tag == "h-zero" and not cold_user:         # z = 0: L_f = B log 2
        assert float(got[0][1]) == pytest.approx(65 * np.log(2.0), rel=1e-6)
    if tag == "weu-zero":                         # all scores 0: every term B log 2, the tables and wei get nothing
        assert np.allclose(got[0][:4].numpy(), 65 * np.log(2.0), rtol=1e-6)
        assert not got[1].any() and not got[2].any() and not got[5].any() and got[4].abs().max() > 0
    if tag == "scores-beyond-30":
        s = torch.stack(R.scores(*(t.double() for t in inp[:5]), users, pos, neg, cold_user))
        t = torch.stack([s[0] - s[1], s[2] - s[3], s[0] - s[3], s[2] - s[1]])
        assert float(t.max()) > 30 and float(t.min()) < -30


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [CASES[2], CASES[7]], ids=IDS)
def test_determinism_scale_and_null_gradients(case, cold_user):
    inp = _inputs(case, cold_user)
    a, b = _fused(inp, WD1, cold_user), _fused(inp, WD1, cold_user)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    half = _fused(inp, WD1, cold_user, scale=0.5)
    assert torch.equal(half[0], a[0])
    for x, y in zip(a[1:], half[1:]):
        assert torch.equal(x * 0.5, y)
    for k in range(5):
        want = [True] * 5
        want[k] = False
        part = _fused(inp, WD1, cold_user, want=tuple(want))
        assert part[1 + k] is None and torch.equal(part[0], a[0])
        for j in range(5):
            if j != k:
                assert torch.equal(part[1 + j], a[1 + j])


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
def test_untouched_rows_keep_the_callers_sentinel(cold_user):
    case = (63, 64, 50, 400)
    inp = _inputs(case, cold_user)
    full = _fused(inp, WD1, cold_user)
    sent = lambda t: torch.full(t.shape, -7.0, device=DEV)
    gu, gi, gh, gwu, gwi = (sent(t) for t in inp[:5])
    _fused(inp, WD1, cold_user, grad_user=gu, grad_item=gi, grad_h=gh, grad_weu=gwu, grad_wei=gwi)
    tu, ti = torch.zeros(50, dtype=torch.bool), torch.zeros(400, dtype=torch.bool)
    tu[inp[5]] = True
    ti[inp[6]] = True
    ti[inp[7]] = True
    assert (~tu).any() and (~ti).any()
    assert (gu.cpu()[~tu] == -7.0).all() and (gi.cpu()[~ti] == -7.0).all()
    assert torch.equal(gu.cpu()[tu], full[1].cpu()[tu]) and torch.equal(gi.cpu()[ti], full[2].cpu()[ti])
    assert torch.equal(gh, full[3]) and torch.equal(gwu, full[4]) and torch.equal(gwi, full[5])
    assert not (full[1].cpu()[~tu] != 0).any() and not (full[2].cpu()[~ti] != 0).any()
    # a buffer that is neither passed nor wanted cannot be written; the others keep the full call's bits
    gu.fill_(-7.0)
    out = _fused(inp, WD1, cold_user, grad_user=gu, grad_h=gh, want=(True, False, True, True, True))
    assert out[2] is None and torch.equal(gu.cpu()[tu], full[1].cpu()[tu]) and torch.equal(gh, full[3])


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    case = (2, 4, 11, 13)
    P, Q, h, weu, wei, users, pos, neg = (t.to(DEV).contiguous() for t in _inputs(case, False))
    plan = ops.mtpr_plan(users, pos, neg)
    L = _lib.lib()
    p = lambda t: t.data_ptr()

    def call(d=4, batch=2, ws="ok", item_rows=13, user_rows=11, u_rng=None, i_rng=None, shift=0):
        space = ops.mtpr_workspace(2, 4, False, plan["n_items"], plan["n_users"], DEV)
        out = [torch.full(t.shape, -7.0, device=DEV) for t in (P, Q, h, weu, wei)] + [torch.full((6,), -7.0, device=DEV)]
        u_rng, i_rng = u_rng or plan["user_range"], i_rng or plan["item_range"]
        ws_ptr, ws_bytes = {"ok": (p(space), space.numel()), "null": (0, space.numel()), "short": (p(space), 16)}[ws]
        rc = L.crh_mtpr_f32(p(P), user_rows, p(Q), item_rows, p(h) + shift, p(weu), p(wei), p(plan["users"]), p(plan["pos"]),
                            p(plan["neg"]), u_rng[0], u_rng[1], i_rng[0], i_rng[1], p(plan["item_ids"]), p(plan["item_ptr"]),
                            p(plan["item_occ"]), p(plan["item_chunk_ptr"]), p(plan["item_chunk_own"]), plan["n_items"],
                            plan["n_item_chunks"], p(plan["user_ids"]), p(plan["user_ptr"]), p(plan["user_occ"]),
                            p(plan["user_chunk_ptr"]), p(plan["user_chunk_own"]), plan["n_users"], plan["n_user_chunks"],
                            batch, d, 0, 0.01, 1.0, *(p(t) for t in out), ws_ptr, ws_bytes, _lib.current_stream())
        torch.cuda.synchronize()
        assert all((t == -7.0).all() for t in out)                     # nothing ran
        return rc, L.crh_last_error().decode()

    ARG, WS = -1, -3                                                   # CRH_ERR_ARG, CRH_ERR_WS of include/coldrec_hip.h
    for kw, rc, text in ((dict(d=6), ARG, "multiple of 4"), (dict(d=132), ARG, "multiple of 4"),
                         (dict(batch=0), ARG, "batch = 0"), (dict(ws="null"), WS, "workspace"),
                         (dict(ws="short"), WS, "workspace"), (dict(shift=4), ARG, "16-byte aligned"),
                         (dict(item_rows=plan["item_range"][1]), ARG, "outside the item table"),
                         (dict(user_rows=plan["user_range"][1]), ARG, "outside the user table"),
                         (dict(u_rng=(-1, 3)), ARG, "outside the user table")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and text in msg, (kw, got_rc, msg)
    assert L.crh_mtpr_workspace_bytes(2, 6, 0, 2, 2) == 0 and L.crh_mtpr_workspace_bytes(0, 4, 0, 1, 1) == 0
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match=r"mtpr: width 132 must be a multiple of 4 in \[4, 128\]"):
        ops.mtpr(z(11, 264), z(13, 132), z(4, 132), z(264, 132), z(264, 132), plan, WD1)
    with pytest.raises(RuntimeError, match="item mode takes tables"):
        ops.mtpr(P, Q, h, weu, wei, plan, WD1, cold_user=True)
    with pytest.raises(RuntimeError, match="mtpr: ids lie outside the tables"):
        ops.mtpr(P[:plan["user_range"][1]].contiguous(), Q, h, weu, wei, plan, WD1)
    with pytest.raises(RuntimeError, match="mtpr: ids lie outside the tables"):
        ops.mtpr(P, Q[:plan["item_range"][1]].contiguous(), h, weu, wei, plan, WD1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.mtpr(P.cpu(), Q.cpu(), h.cpu(), weu.cpu(), wei.cpu(), plan, WD1)
    with pytest.raises(RuntimeError, match="contiguous 2-D float32"):
        ops.mtpr(P.double(), Q, h, weu, wei, plan, WD1)
    with pytest.raises(RuntimeError, match="integer tensors"):
        ops.mtpr_plan(users.float(), pos, neg)
    with pytest.raises(RuntimeError, match="outside the item table"):
        ops.mtpr_plan(users, pos, neg, n_users=11, n_items=int(max(pos.max(), neg.max())))
    with pytest.raises(RuntimeError, match="adagrad_rows: width 6"):
        ops.adagrad_rows(z(4, 6), z(4, 6), z(4, 6), torch.zeros(1, dtype=torch.int32, device=DEV), 0.05)
    with pytest.raises(RuntimeError, match="int32 vector"):
        ops.adagrad_rows(z(4, 8), z(4, 8), z(4, 8), torch.zeros(1, dtype=torch.int64, device=DEV), 0.05)


# ---- the touched-rows Adagrad ------------------------------------------------------------------------------------------

def adagrad_distance(got_p, got_s, want_p, want_s):
    return max(float((got_p.double() - want_p).abs().max() / want_p.abs().max()),
               float((got_s.double() - want_s).abs().max() / max(float(want_s.abs().max()), 1e-30)))


@pytest.mark.parametrize("case", R.ADAGRAD_CASES, ids=lambda c: "d%d-%s" % (c[0], "first" if c[1] else "later"))
def test_adagrad_rows_matches_float64_restatement(case):
    from coldrec_amd import ops
    p, g, s, ids = R.adagrad_inputs(*case)
    want_p, want_s = R.adagrad(p.double(), g.double(), s.double(), ids, R.ADAGRAD_LR)
    pd, gd, sd = p.to(DEV), g.to(DEV), s.to(DEV)
    ops.adagrad_rows(pd, gd, sd, ids.to(DEV), R.ADAGRAD_LR)
    pd, gd, sd = pd.cpu(), gd.cpu(), sd.cpu()
    err = adagrad_distance(pd, sd, want_p, want_s)
    print(f"adagrad_rows d{case[0]}: error over the maximum {err:.2e}")
    assert err <= ADAGRAD_BAR
    rest = torch.ones(p.shape[0], dtype=torch.bool)
    rest[ids.long()] = False
    assert rest.any()                              # the rows outside ids keep their bits in p, s and g
    assert torch.equal(pd[rest], p[rest]) and torch.equal(sd[rest], s[rest]) and torch.equal(gd[rest], g[rest])
    zero = ids[:3].long()                          # zero-gradient rows keep their bits
    assert not g[zero].any() and torch.equal(pd[zero], p[zero]) and torch.equal(sd[zero], s[zero])
    assert not gd[ids.long()].any() and g[ids[3:].long()].abs().min() > 0          # consumed rows are cleared
    p2, g2, s2 = p.to(DEV), g.to(DEV), s.to(DEV)
    ops.adagrad_rows(p2, g2, s2, ids.to(DEV), R.ADAGRAD_LR, zero_grad=False)
    assert torch.equal(p2.cpu(), pd) and torch.equal(s2.cpu(), sd) and torch.equal(g2.cpu(), g)


def test_adagrad_rows_follows_torch_adagrad_over_three_steps():
    """Three consecutive steps over changing row subsets against torch.optim.Adagrad on the CPU stepping the whole table
    with the dense gradient (zero outside the subset)."""
    from coldrec_amd import ops
    gen = torch.Generator().manual_seed(77)
    p0 = torch.randn(40, 64, generator=gen) * 0.1
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.Adagrad([ref], lr=R.ADAGRAD_LR)
    pd, sd, gd = p0.to(DEV), torch.zeros(40, 64, device=DEV), torch.zeros(40, 64, device=DEV)
    for _ in range(3):
        ids = torch.randperm(40, generator=gen)[:17]
        dense = torch.zeros(40, 64)
        dense[ids] = torch.randn(17, 64, generator=gen)
        ref.grad = dense.clone()
        opt.step()
        gd.copy_(dense)
        ops.adagrad_rows(pd, gd, sd, ids.to(torch.int32).to(DEV), R.ADAGRAD_LR)
        assert not gd.any()
    err = adagrad_distance(pd.cpu(), sd.cpu(), ref.detach().double(), opt.state[ref]["sum"].double())
    print(f"adagrad_rows, three steps against torch.optim.Adagrad: error over the maximum {err:.2e}")
    assert err <= ADAGRAD_BAR


# ---- the trainer's autograd operator ---------------------------------------------------------------------------------

@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("cdim", [16, 7])
def test_autograd_operator_matches_restatement_through_the_content_projection(cdim, cold_user):
    """The trainer's autograd operator fed by content @ W against the float64 restatement through torch.autograd.grad with
    grad_out = 0.7: W, weu and wei receive their gradients; the tables' land in the caller's buffers, unscaled."""
    from coldrec_amd import ops
    from coldrec_amd.model.MTPR import _FusedLoss
    P, Q, _, weu, wei, users, pos, neg = _inputs((96, 32, 40, 90), cold_user)
    gen = torch.Generator().manual_seed(5 + cdim)
    content = torch.randn(40 if cold_user else 90, cdim, generator=gen)
    W0 = torch.randn(cdim, 32, generator=gen) * 0.3
    src = users if cold_user else torch.cat([pos, neg])

    def grads(dt, dev, fused):
        W, wu, wi = (torch.nn.Parameter(t.to(dt).to(dev)) for t in (W0, weu, wei))
        Pd, Qd = P.to(dt).to(dev), Q.to(dt).to(dev)
        h = content.to(dt).to(dev)[src.to(dev)] @ W
        if fused:
            gu, gi = torch.zeros_like(Pd), torch.zeros_like(Qd)
            plan = ops.mtpr_plan(users.to(dev), pos.to(dev), neg.to(dev))
            ws = ops.mtpr_workspace(96, 32, cold_user, plan["n_items"], plan["n_users"], dev)
            total, terms = _FusedLoss.apply(h, wu, wi, Pd, Qd, plan, WD1, cold_user, gu, gi, ws)
            assert float(total.detach()) == float(terms[5])
            tables = [gu.double().cpu().numpy(), gi.double().cpu().numpy()]
        else:
            Pd, Qd = Pd.requires_grad_(), Qd.requires_grad_()
            terms = R.loss_terms(Pd, Qd, h, wu, wi, users, pos, neg, WD1, cold_user)
            total = terms[5]
            tables = [x.numpy() for x in torch.autograd.grad(total, (Pd, Qd), retain_graph=True)]
        got = torch.autograd.grad(total, (W, wu, wi), grad_outputs=torch.tensor(0.7, dtype=dt, device=dev))
        return np.array([float(t.detach()) for t in terms]), [x.double().cpu().numpy() for x in got] + tables

    terms, got = grads(torch.float32, DEV, True)
    want_terms, want = grads(torch.float64, "cpu", False)
    rel = np.abs(terms - want_terms).max() / want_terms[5]
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    print(f"autograd: loss err / total {rel:.2e}, gradient err / max {errs}")
    # the float32 content projection and the kernel, each within its bar of the float64 value
    assert rel <= 2 * LOSS_BAR and max(errs) <= 2 * GRAD_BAR
    assert all(np.abs(a).max() > 0 for a in got)


# ---- whole runs against G25 --------------------------------------------------------------------------------------------

def _cfg(data, device=DEV, **kw):
    a = dict(dataset="toy", model="MTPR", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, p_emb=[0.05, 0.0], p_ctx=[0.05, 0.01], p_proj=[0.05, 0.01])
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


@functools.lru_cache(maxsize=None)
def restated_run(cold, dtype):
    """The restatement's whole run, computed once per cold object and dtype and shared (callers leave it unchanged).  On
    one thread: torch's multi-threaded CPU reductions change their order from run to run, and over the 16 steps that moves
    the float32 run's distance to G25 between 4e-6 and 3e-5 of a table's scale; one thread gives the same bits every time."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return R.run(R.toy_data(cold), dtype, cold == "user")
    finally:
        torch.set_num_threads(threads)


def _run(cold, **kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle)."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    set_seed(2024, True)
    tr = AVAILABLE_MODELS["MTPR"](_cfg(R.toy_data(cold), cold_object=cold, **kw))
    tr.run()
    return tr


def _trained(tr):
    m = tr.model
    return [t.detach().cpu().numpy() for t in (m.P.weight, m.Q.weight, m.W, m.weu, m.wei)]


@pytest.fixture(scope="module", params=["item", "user"])
def toy_run(request):
    cold = request.param
    return cold, load_golden(f"g25_mtpr_{cold}.npz"), _run(cold)


def test_run_matches_reference_g25(toy_run):
    """Bars: RUN_LOSS_BAR / RUN_TABLE_BAR above."""
    cold, fx, tr = toy_run
    best = [t.cpu().numpy() for t in (tr.user_emb, tr.item_emb)]
    trained = _trained(tr)
    assert tr.batch_losses.shape == (16, 6)
    rel, e_best, e_trained = R.run_distances(fx, tr.batch_losses, best, trained)
    print(f"MTPR {cold}: worst term difference to G25 over the total {rel:.2e}; best tables differ by {e_best[0]:.2e} / "
          f"{e_best[1]:.2e} of their scale, trained P, Q, W, weu, wei by " + " ".join(f"{e:.2e}" for e in e_trained))
    assert rel <= RUN_LOSS_BAR and max(e_best) <= RUN_TABLE_BAR and max(e_trained) <= RUN_TABLE_BAR
    assert np.allclose(tr.batch_losses[:, 5], tr.batch_losses[:, :5].sum(1), rtol=1e-6)
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    touched = restated_run(cold, torch.float32)["touched"]
    for k, name in enumerate(("P", "Q")):          # rows no batch touched: no step moved them
        rows = ~touched[k]
        print(f"MTPR {cold}: {int(rows.sum())} rows of {name} were gathered by no batch")
        assert np.array_equal(trained[k][rows], fx["init_" + name][rows])
        assert np.abs(trained[k][touched[k]] - fx["init_" + name][touched[k]]).max() > 1e-3
    got_lists = {}
    for t in ("all", "cold", "warm"):
        c, _s, i = tr._topk_arrays(tr._sets("test", t), t)
        assert np.array_equal(c["users_int"].cpu().numpy(), fx[f"{t}_users_int"])
        got_lists[t] = i
    same, det, total = lists_vs_reference(fx, best, got_lists, min_frac=0.5)
    print(f"MTPR {cold}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    results = dict(overall=tr.overall_test_results, cold=tr.cold_test_results, warm=tr.warm_test_results)
    metrics_vs_reference(results, fx, same == total, tr.bestPerformance[1]["NDCG"])
    lines = json.loads(str(fx["loss_lines"]))
    assert len(lines) == 2 and [float(l.split("batch_loss:")[1]) for l in lines] == pytest.approx(
        list(tr.batch_losses[[0, 8], 5]), rel=RUN_LOSS_BAR)


def test_second_run_is_bit_identical(toy_run):
    cold, _, a = toy_run
    b = _run(cold)
    assert np.array_equal(a.batch_losses, b.batch_losses)
    assert torch.equal(a.user_emb, b.user_emb) and torch.equal(a.item_emb, b.item_emb)
    for x, y in zip(_trained(a), _trained(b)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("cold", ["item", "user"])
def test_cli_trains_end_to_end(cold, tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", cold, "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "MF", "--make_synthetic", "toy"] + common) is None
    pay = main(["--model", "MTPR", "--epochs", "2", "--p_emb", "0.05,0", "--p_ctx", "[0.05, 0.01]"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "MTPR" / "history.txt").is_file()
    out = {s: torch.load(tmp_path / "emb" / f"toy_cold_{cold}_MTPR_{s}_emb.pt", map_location="cpu") for s in ("user", "item")}
    assert out["user"].shape[1] == out["item"].shape[1] == 64
    for s in ("user", "item"):
        assert torch.isfinite(out[s]).all() and out[s].abs().max() > 0
