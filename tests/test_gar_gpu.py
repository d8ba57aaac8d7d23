"""GPU: the fused GAR loss (csrc/gar.hip) against the float64 restatement (tests/gar_restate.py, itself pinned to the
reference's runs by tests/test_gar.py), in item mode and in user mode: the shapes where it can go wrong, its edges, its
determinism contract, the argument errors, the trainer's autograd operator, and whole runs against G24.

Bars of the kernel against the float64 restatement: 8x the worst distance of the float32 torch formula (CPU) from the
float64 one at the same cases, both modes.  Loss terms are measured as error over the TOTAL loss, gradients as error over
their maximum.  Measured on the CPU (tests/test_gar.py prints them again and holds them to a factor of 2):
    cases:  loss terms, error / total  worst 1.91e-7 (B2048-d64, item)   -> LOSS_BAR = 1.53e-6
            gradients, error / maximum worst 7.78e-7 (the chunk case, item, d V: 513 and more occurrences per row; 1.6e-7
            .. 3.6e-7 elsewhere)                                          -> GRAD_BAR = 6.22e-6
    edges:  loss terms worst 1.33e-7 (pos-is-neg), gradients worst 2.51e-6 (scores beyond +-30, item)
            (the edge bars are 8x these or the cases' bars, whichever is larger; the worst edge is the one with scores
            beyond +-30, where a dot product's rounding is multiplied by bpr's slope)
On the MI355X the kernel measures 1.69e-7 (loss terms, B300-d256) and 6.13e-7 (gradients, B2-d4) at worst over the cases,
2.02e-7 and 2.34e-6 over the edges (both at scores beyond +-30).

Whole runs against G24: plain float32 torch on the CPU (tests/test_gar.py) ends 8.81e-8 (item) / 8.91e-8 (user) of the
total from G24's loss terms and 1.51e-5 / 1.46e-6 (item: users / items) and 2.35e-7 / 2.34e-7 (user) of the tables'
scale from its final tables.  8x those stay below the project's run bars, 1e-5 and 2e-4, which are therefore the bars.
On the MI355X the runs end 1.76e-7 (item) / 1.87e-7 (user) of the total from G24's loss terms and 1.74e-5 / 1.14e-6 (item)
and 3.02e-7 / 2.98e-6 (user) of the tables' scale from its tables; every one of the 750 / 456 final lists equals the
reference's (725 / 446 users with a determined ranking).  On both fixtures every row outside the cold set is gathered by
some batch, so the check of the rows no batch touched runs over an empty set there; it is kept for other data.
"""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import gar_restate
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_LOSS_WORST, F32_GRAD_WORST = 1.91e-7, 7.78e-7         # float32 torch against float64 torch at CASES, both modes
LOSS_BAR, GRAD_BAR = 8 * F32_LOSS_WORST, 8 * F32_GRAD_WORST
EDGE_F32_LOSS_WORST, EDGE_F32_GRAD_WORST = 1.33e-7, 2.51e-6      # ... at the edge cases
EDGE_LOSS_BAR, EDGE_GRAD_BAR = max(8 * EDGE_F32_LOSS_WORST, LOSS_BAR), max(8 * EDGE_F32_GRAD_WORST, GRAD_BAR)
RUN_LOSS_BAR, RUN_TABLE_BAR = 1e-5, 2e-4                  # the project's run bars (see above)
F32_RUN_LOSS = dict(item=8.81e-8, user=8.91e-8)           # float32 torch against G24, measured
F32_RUN_TABLES = dict(item=(1.51e-5, 1.46e-6), user=(2.35e-7, 2.34e-7))

COEF = (0.05, 0.1, 1e-4)                                  # alpha, beta, reg: the trainer's defaults
MODES = [False, True]
MODE_IDS = lambda m: "user" if m else "item"


def chunk_rows():
    from coldrec_amd import _lib
    return int(_lib.lib().crh_gar_chunk_rows())


# B, d, nu, ni; "chunks": B = 3 (2 chunk + 1) records dealt out so that each of the 3 users holds 2 chunk + 1 of them, four
# of the 5 items 2 chunk + 1 of the 2B occurrences and the fifth the remaining 4 chunk + 2 (2B is even, so the five counts
# cannot all be one more than a whole number of chunks): every owner holds several chunks, all but one a ragged one of 1
CASES = [(1, 4, 11, 11), (2, 4, 11, 13), (37, 20, 11, 30), (63, 64, 50, 400), (65, 252, 300, 500), (300, 256, 11, 500),
         ("chunks", 132, 3, 5), (2048, 64, 300, 500)]
IDS = lambda c: "B%s-d%d" % c[:2]


def _inputs(case, seed=0, scale=0.3):
    """(U, V, users, pos, neg, G) on the CPU; ids drawn with repeats."""
    B, d, nu, ni = case
    g = torch.Generator().manual_seed(2400 + seed + d + 7 * (B if B != "chunks" else 513))
    if B == "chunks":
        c = chunk_rows()
        B = 3 * (2 * c + 1)
        users = torch.arange(3).repeat_interleave(2 * c + 1)[torch.randperm(B, generator=g)]
        occ = torch.cat([torch.arange(4).repeat_interleave(2 * c + 1), torch.full((4 * c + 2,), 4)])
        occ = occ[torch.randperm(2 * B, generator=g)]
        pos, neg = occ[:B].clone(), occ[B:].clone()
    else:
        users = torch.randint(nu, (B,), generator=g)
        pos, neg = torch.randint(ni, (B,), generator=g), torch.randint(ni, (B,), generator=g)
    U, V = torch.randn(nu, d, generator=g) * scale, torch.randn(ni, d, generator=g) * scale
    G = torch.tanh(torch.randn(B, d, generator=g) * scale)
    return U, V, users, pos, neg, G


def edge_cases():
    """(tag, inputs, (alpha, beta, reg)) of the edges; every one runs in both modes."""
    out = []
    base = (37, 20, 11, 30)
    inp = list(_inputs(base, seed=1))
    inp[4] = inp[4].clone()
    inp[4][5] = inp[3][5]                                             # a record with pos == neg
    out.append(("pos-is-neg", inp, COEF))
    inp = list(_inputs(base, seed=2))
    inp[3], inp[4] = inp[3].clone(), inp[4].clone()
    inp[3][0], inp[4][0], inp[3][1], inp[4][1] = 7, 8, 9, 7           # item 7: a positive in record 0, a negative in 1
    out.append(("pos-and-neg", inp, COEF))
    for a, b in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0)):
        out.append((f"alpha{a:g}-beta{b:g}", list(_inputs(base, seed=3)), (a, b, 1e-4)))
    out.append(("reg0", list(_inputs(base, seed=4)), (0.05, 0.1, 0.0)))
    inp = list(_inputs((65, 64, 50, 400), seed=5))
    inp[5] = torch.zeros_like(inp[5])                                 # G = 0: a block of zero norm
    out.append(("gen-zero", inp, (0.05, 0.1, 1e-2)))
    out.append(("scores-beyond-30", list(_inputs((65, 64, 50, 400), seed=6, scale=2.0)), COEF))
    inp = list(_inputs((63, 64, 50, 400), seed=7))
    for k in (2, 3, 4):
        inp[k] = inp[k].clone()
    inp[2][0], inp[2][1], inp[3][0], inp[3][1], inp[4][2], inp[4][3] = 0, 49, 0, 399, 0, 399
    out.append(("first-and-last-rows", inp, COEF))
    return out


def _fused(inp, coef, cold_user, scale=1.0, want=(True, True, True), **kw):
    from coldrec_amd import ops
    U, V, users, pos, neg, G = (t.to(DEV) for t in inp)
    plan = ops.gar_plan(users, pos, neg)
    loss, du, di, dg = ops.gar(U, V, G, plan, *coef, cold_user=cold_user, scale=scale, want_user=want[0],
                               want_item=want[1], want_gen=want[2], **kw)
    torch.cuda.synchronize()
    return loss.cpu(), du, di, dg


def distances(got, want):
    """(worst error of the four loss terms over the total, [error / maximum of d U, d V, d G]) of numpy tuples."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]).max() / abs(want[0][3])
    errs = []
    for g, w in zip(got[1:], want[1:]):
        top = np.abs(w).max()
        errs.append(np.abs(np.asarray(g, np.float64) - w).max() / top if top > 0 else np.abs(g).max())
    return rel, errs


def _compare(tag, got, want, loss_bar=LOSS_BAR, grad_bar=GRAD_BAR):
    got = (got[0].numpy(),) + tuple(g.cpu().numpy() for g in got[1:])
    assert all(np.isfinite(g).all() for g in got)
    rel, errs = distances(got, want)
    print(f"{tag}: loss err / total {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert rel <= loss_bar
    assert max(errs) <= grad_bar


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_matches_float64_restatement(case, cold_user):
    inp = _inputs(case)
    if case[0] == "chunks":
        from coldrec_amd import ops
        plan, c = ops.gar_plan(inp[2], inp[3], inp[4]), chunk_rows()
        for side in ("user", "item"):
            sizes = torch.diff(plan[f"{side}_ptr"])
            per = torch.diff(plan[f"{side}_chunk_ptr"])
            assert (per >= 3).all() and int(((sizes % c) == 1).sum()) >= len(sizes) - 1
    _compare(IDS(case), _fused(inp, COEF, cold_user), gar_restate.step(*inp, *COEF, cold_user))


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("edge", edge_cases(), ids=lambda e: e[0])
def test_edges(edge, cold_user):
    tag, inp, coef = edge
    got = _fused(inp, coef, cold_user)
    want = gar_restate.step(*inp, *coef, cold_user)
    _compare(tag, got, want, EDGE_LOSS_BAR, EDGE_GRAD_BAR)
    if tag == "pos-is-neg":                       # x3 = 0 in that record and both contributions land on the one row
        assert int(inp[3][5]) == int(inp[4][5]) and np.abs(want[2][int(inp[3][5])]).max() > 0
    if tag == "pos-and-neg":
        assert int(inp[3][0]) == int(inp[4][1]) == 7
    if tag == "gen-zero":
        assert float(got[0][2]) > 0 and not inp[5].any()              # R keeps the other three blocks' norms
    if tag == "scores-beyond-30":                 # where bpr sits on its floor, -log(1e-5) = 11.51, or at 0
        U, V = inp[0].double(), inp[1].double()
        x3 = (U[inp[2]] * (V[inp[3]] - V[inp[4]])).sum(1)
        assert float(x3.max()) > 30 and float(x3.min()) < -30


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("case", [CASES[2], CASES[6]], ids=IDS)
def test_determinism_scale_and_null_gradients(case, cold_user):
    inp = _inputs(case)
    a, b = _fused(inp, COEF, cold_user), _fused(inp, COEF, cold_user)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    half = _fused(inp, COEF, cold_user, scale=0.5)
    assert torch.equal(half[0], a[0])
    for x, y in zip(a[1:], half[1:]):
        assert torch.equal(x * 0.5, y)
    for k in range(3):
        want = [True, True, True]
        want[k] = False
        part = _fused(inp, COEF, cold_user, want=tuple(want))
        assert part[1 + k] is None and torch.equal(part[0], a[0])
        for j in range(3):
            if j != k:
                assert torch.equal(part[1 + j], a[1 + j])


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
def test_untouched_rows_keep_the_callers_sentinel(cold_user):
    case = (63, 64, 50, 400)
    inp = _inputs(case)
    full = _fused(inp, COEF, cold_user)
    gu, gi = torch.full((50, 64), -7.0, device=DEV), torch.full((400, 64), -7.0, device=DEV)
    gg = torch.full((63, 64), -7.0, device=DEV)
    _fused(inp, COEF, cold_user, grad_user=gu, grad_item=gi, grad_gen=gg)
    tu, ti = torch.zeros(50, dtype=torch.bool), torch.zeros(400, dtype=torch.bool)
    tu[inp[2]] = True
    ti[inp[3]] = True
    ti[inp[4]] = True
    assert (~tu).any() and (~ti).any()
    assert (gu.cpu()[~tu] == -7.0).all() and (gi.cpu()[~ti] == -7.0).all()
    assert torch.equal(gu.cpu()[tu], full[1].cpu()[tu]) and torch.equal(gi.cpu()[ti], full[2].cpu()[ti])
    assert torch.equal(gg, full[3]) and not (full[1].cpu()[~tu] != 0).any() and not (full[2].cpu()[~ti] != 0).any()
    # a buffer that is neither passed nor wanted cannot be written; the others keep the full call's bits
    gu.fill_(-7.0)
    out = _fused(inp, COEF, cold_user, grad_user=gu, grad_gen=gg, want=(True, False, True))
    assert out[2] is None and torch.equal(gu.cpu()[tu], full[1].cpu()[tu]) and torch.equal(gg, full[3])


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    case = (2, 4, 11, 13)
    U, V, users, pos, neg, G = (t.to(DEV).contiguous() for t in _inputs(case))
    plan = ops.gar_plan(users, pos, neg)
    L = _lib.lib()
    p = lambda t: t.data_ptr()

    def call(d=4, batch=2, ws="ok", item_rows=13, user_rows=11, u_rng=None, i_rng=None, shift=0):
        space = ops.gar_workspace(2, 4, plan["n_items"], plan["n_users"], DEV)
        out = [torch.full((11, 4), -7.0, device=DEV), torch.full((13, 4), -7.0, device=DEV),
               torch.full((2, 4), -7.0, device=DEV), torch.full((4,), -7.0, device=DEV)]
        u_rng, i_rng = u_rng or plan["user_range"], i_rng or plan["item_range"]
        ws_ptr, ws_bytes = {"ok": (p(space), space.numel()), "null": (0, space.numel()), "short": (p(space), 16)}[ws]
        rc = L.crh_gar_f32(p(U), user_rows, p(V), item_rows, p(G) + shift, p(plan["users"]), p(plan["pos"]), p(plan["neg"]),
                           u_rng[0], u_rng[1], i_rng[0], i_rng[1], p(plan["item_ids"]), p(plan["item_ptr"]),
                           p(plan["item_occ"]), p(plan["item_chunk_ptr"]), p(plan["item_chunk_own"]), plan["n_items"],
                           plan["n_item_chunks"], p(plan["user_ids"]), p(plan["user_ptr"]), p(plan["user_occ"]),
                           p(plan["user_chunk_ptr"]), p(plan["user_chunk_own"]), plan["n_users"], plan["n_user_chunks"],
                           batch, d, 0, 0.05, 0.1, 1e-4, 1.0, p(out[0]), p(out[1]), p(out[2]), p(out[3]), ws_ptr, ws_bytes,
                           _lib.current_stream())
        torch.cuda.synchronize()
        assert all((t == -7.0).all() for t in out)                     # nothing ran
        return rc, L.crh_last_error().decode()

    ARG, WS = -1, -3                                                   # CRH_ERR_ARG, CRH_ERR_WS of include/coldrec_hip.h
    for kw, rc, text in ((dict(d=6), ARG, "multiple of 4"), (dict(d=260), ARG, "multiple of 4"),
                         (dict(batch=0), ARG, "batch = 0"), (dict(ws="null"), WS, "workspace"),
                         (dict(ws="short"), WS, "workspace"), (dict(shift=4), ARG, "16-byte aligned"),
                         (dict(item_rows=plan["item_range"][1]), ARG, "outside the item table"),
                         (dict(user_rows=plan["user_range"][1]), ARG, "outside the user table"),
                         (dict(u_rng=(-1, 3)), ARG, "outside the user table")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and text in msg, (kw, got_rc, msg)
    assert L.crh_gar_workspace_bytes(2, 6, 2, 2) == 0 and L.crh_gar_workspace_bytes(0, 4, 1, 1) == 0
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match=r"gar: width 6 must be a multiple of 4 in \[4, 256\]"):
        ops.gar(z(11, 6), z(13, 6), z(2, 6), plan, *COEF)
    with pytest.raises(RuntimeError, match="gar: ids lie outside the tables"):
        ops.gar(U[:plan["user_range"][1]].contiguous(), V, G, plan, *COEF)
    with pytest.raises(RuntimeError, match="gar: ids lie outside the tables"):
        ops.gar(U, V[:plan["item_range"][1]].contiguous(), G, plan, *COEF)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.gar(U.cpu(), V.cpu(), G.cpu(), plan, *COEF)
    with pytest.raises(RuntimeError, match="contiguous 2-D float32"):
        ops.gar(U.double(), V, G, plan, *COEF)
    with pytest.raises(RuntimeError, match="integer tensors"):
        ops.gar_plan(users.float(), pos, neg)
    with pytest.raises(RuntimeError, match="outside the item table"):
        ops.gar_plan(users, pos, neg, n_users=11, n_items=int(max(pos.max(), neg.max())))


@pytest.mark.parametrize("cold_user", MODES, ids=MODE_IDS)
def test_autograd_operator_matches_restatement_through_the_generator(cold_user):
    """The trainer's autograd operator, fed by a small generator, against the float64 restatement through
    torch.autograd.grad with grad_out = 0.7: the generator's parameters and both tables receive their gradients."""
    from coldrec_amd import ops
    from coldrec_amd.model.GAR import _FusedLoss
    U, V, users, pos, neg, _ = _inputs((96, 32, 40, 90))
    torch.manual_seed(5)
    content = torch.randn(40 if cold_user else 90, 12)
    gen = gar_restate.generator(12, 32)
    src = users if cold_user else pos

    def grads(dt, dev, fused):
        g = gar_restate.generator(12, 32).to(dt).to(dev)
        g.load_state_dict({k: v.to(dt) for k, v in gen.state_dict().items()})
        Up, Vp = (torch.nn.Parameter(t.to(dt).to(dev)) for t in (U, V))
        params = list(g.parameters()) + [Up, Vp]
        out = g(content.to(dt).to(dev)[src.to(dev)])
        if fused:
            total, terms = _FusedLoss.apply(out, Up, Vp, ops.gar_plan(users.to(dev), pos.to(dev), neg.to(dev)), COEF, cold_user)
            assert float(total.detach()) == float(terms[3])
        else:
            terms = gar_restate.loss_terms(Up, Vp, users, pos, neg, out, *COEF, cold_user)
            total = terms[3]
        got = torch.autograd.grad(total, params, grad_outputs=torch.tensor(0.7, dtype=dt, device=dev))
        return np.array([float(t.detach()) for t in terms]), [x.double().cpu().numpy() for x in got]

    terms, got = grads(torch.float32, DEV, True)
    want_terms, want = grads(torch.float64, "cpu", False)
    rel = np.abs(terms - want_terms).max() / want_terms[3]
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    print(f"autograd: loss err / total {rel:.2e}, gradient err / max {errs}")
    # the float32 generator and the kernel, each within its bar of the float64 value
    assert rel <= 2 * LOSS_BAR and max(errs) <= 2 * GRAD_BAR
    assert all(np.abs(a).max() > 0 for a in got)


# ---- whole runs against G24 --------------------------------------------------------------------------------------------

def _cfg(data, device=DEV, **kw):
    a = dict(dataset="toy", model="GAR", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, alpha=0.05, beta=0.1)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def write_loaded(fx, where, cold):
    (where / "emb").mkdir(exist_ok=True)
    torch.save(torch.from_numpy(fx["loaded_U"]), where / "emb" / f"toy_cold_{cold}_MF_user_emb.pt")
    torch.save(torch.from_numpy(fx["loaded_V"]), where / "emb" / f"toy_cold_{cold}_MF_item_emb.pt")


def run_distances(fx, losses, tables):
    """(worst |loss term - G24's| / G24's total over the steps, [|table - G24's| / G24's scale of the two tables]);
    ``losses`` (steps, 3) = [L_gen, L_rec, total]."""
    want = fx["losses"]
    assert losses.shape == want.shape
    rel = (np.abs(losses - want) / np.abs(want[:, 2:3])).max()
    errs = [float(np.abs(np.asarray(t, np.float64) - fx[k]).max() / np.abs(fx[k]).max())
            for t, k in zip(tables, ("user_emb", "item_emb"))]
    return rel, errs


def lists_vs_reference(fx, tables, got_lists=None, min_frac=0.5):
    """The determined-ranking criterion of tests/test_e2e_gpu.py and tests/test_aldi_gpu.py for one user and one item
    table whose rows differ from the reference's by very different amounts (trained rows, generated rows).  Every score
    may move by its own bound: D[u, j] = the fp32 dot-product error bound + the change the measured differences of user
    row u and of item row j can cause.  A user's ranking is DETERMINED when, walking the reference's fp64 order, each of
    the k leading scores less its bound stays above every later score plus its bound; those users' lists must be
    identical.  ``got_lists[t]`` = our (n, k) ids per setting, or None to rank ``tables`` here in float64.  Returns
    (same, determined, users)."""
    ref = [np.asarray(fx[k], np.float64) for k in ("user_emb", "item_emb")]
    got = [np.asarray(t, np.float64) for t in tables]
    d = ref[1].shape[1]
    e_u, e_v = (np.abs(g - r).max(axis=1) for g, r in zip(got, ref))
    gam = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    a_v = np.abs(ref[1])
    same = det = total = 0
    for t in ("all", "cold", "warm"):
        want_i, want_s, users = fx[f"{t}_idx"], fx[f"{t}_score"], fx[f"{t}_users_int"]
        k = want_i.shape[1]
        rp, rc = fx[f"{t}_rated_rowptr"], fx[f"{t}_rated_col"]

        def masked(S, fill):
            for r in range(len(users)):
                S[r, rc[rp[r]:rp[r + 1]]] = fill
            if fx[f"{t}_cand"].size:
                S[:, fx[f"{t}_cand"]] = fill
            return S

        S = masked(ref[0][users] @ ref[1].T, -1e9)
        a_u, eu = np.abs(ref[0][users]), e_u[users][:, None]
        D = masked(gam * (a_u @ a_v.T) + eu * a_v.sum(1)[None, :] + a_u.sum(1)[:, None] * e_v[None, :] + d * eu * e_v[None, :],
                   0.0)                                                            # ties among masked entries are by design
        order = np.argsort(-S, axis=1, kind="stable")
        low, high = np.take_along_axis(S - D, order, 1), np.take_along_axis(S + D, order, 1)
        later = np.maximum.accumulate(high[:, ::-1], axis=1)[:, ::-1]              # max of high over positions >= r
        lead = np.take_along_axis(S, order, 1)[:, :k] > -1e8
        determined = (~lead | (low[:, :k] > later[:, 1:k + 1])).all(axis=1)
        mine = got_lists[t] if got_lists is not None else \
            np.argsort(-masked(got[0][users] @ got[1].T, -1e9), axis=1, kind="stable")[:, :k]
        real = want_s > -1e8                                                       # masked fill-ins: order unspecified
        equal = np.array([np.array_equal(mine[r][real[r]], want_i[r][real[r]]) for r in range(len(users))])
        assert equal[determined].all(), (t, "users with a determined ranking whose list differs from the reference's:",
                                         np.nonzero(determined & ~equal)[0][:10])
        print(f"  {t}: {int(equal.sum())} of {len(users)} lists identical, {int(determined.sum())} determined")
        same, det, total = same + int(equal.sum()), det + int(determined.sum()), total + len(users)
    assert det >= min_frac * total, f"only {det} of {total} rankings are determined at table errors {e_u.max():.2e} {e_v.max():.2e}"
    return same, det, total


def metrics_vs_reference(results, fx, lists_identical, best_ndcg=None, loose=2e-4):
    """tests/test_e2e_gpu.py's _metrics_vs_reference on G24's arrays: 5-dp metrics equal to the reference's when every
    list is (1e-5 = one unit of the rounding), within 2e-4 otherwise."""
    tol = 1.5e-5 if lists_identical else loose
    for name in ("overall", "cold", "warm"):
        np.testing.assert_allclose(np.array(results[name]), fx[f"test_{name}"], atol=tol, rtol=0)
    if best_ndcg is not None:
        np.testing.assert_allclose(best_ndcg, json.loads(str(fx["best_metrics"]))["NDCG"], atol=loose, rtol=0)


def _run(where, cold, **kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle), with ``where`` --
    whose ./emb holds the fixture's loaded tables -- as the working directory."""
    import os
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    data = gar_restate.toy_data(cold)
    cwd = os.getcwd()
    os.chdir(where)
    try:
        set_seed(2024, True)
        tr = AVAILABLE_MODELS["GAR"](_cfg(data, cold_object=cold, **kw))
        tr.run()
    finally:
        os.chdir(cwd)
    return tr


@pytest.fixture(scope="module", params=["item", "user"])
def toy_run(request, tmp_path_factory):
    cold = request.param
    where = tmp_path_factory.mktemp("gar_" + cold)
    fx = load_golden(f"g24_gar_{cold}.npz")
    write_loaded(fx, where, cold)
    return cold, fx, _run(where, cold), where


def test_run_matches_reference_g24(toy_run):
    """Bars: RUN_LOSS_BAR / RUN_TABLE_BAR above."""
    cold, fx, tr, _ = toy_run
    tables = [t.cpu().numpy() for t in (tr.user_emb, tr.item_emb)]
    assert tr.batch_losses.shape == (16, 4)
    rel, errs = run_distances(fx, tr.batch_losses[:, [0, 1, 3]], tables)
    print(f"GAR {cold}: worst loss-term difference to G24 over the total {rel:.2e}; final tables differ by "
          f"{errs[0]:.2e} / {errs[1]:.2e} of their scale")
    assert rel <= RUN_LOSS_BAR and max(errs) <= RUN_TABLE_BAR
    assert np.allclose(tr.batch_losses[:, 3], tr.batch_losses[:, :3].sum(1), rtol=1e-6)
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    # rows outside the cold set that no batch gathered: moved only by what Adam does with zero gradients -- against the
    # float32 restatement's run, not the loaded bits
    r = gar_restate.run(gar_restate.toy_data(cold), fx["loaded_U"], fx["loaded_V"], torch.float32, cold == "user")
    snap = r["snaps"][int(fx["best_epoch"]) - 1]
    is_cold = [np.zeros(t.shape[0], bool) for t in tables]
    is_cold[0 if cold == "user" else 1][np.asarray(tr.data.mapped_cold_user_idx if cold == "user"
                                                   else tr.data.mapped_cold_item_idx)] = True
    for k in range(2):
        rows = ~r["touched"][k] & ~is_cold[k]
        print(f"GAR {cold}: {int(rows.sum())} rows of table {k} outside the cold set were gathered by no batch")
        assert np.array_equal(tables[k][rows], snap[k][rows].astype(np.float32))
    moved = np.abs(tables[0] - fx["loaded_U"]).max(), np.abs(tables[1] - fx["loaded_V"]).max()
    assert min(moved) > 1e-3                                                     # both tables were trained
    got_lists = {}
    for t in ("all", "cold", "warm"):
        c, _s, i = tr._topk_arrays(tr._sets("test", t), t)
        assert np.array_equal(c["users_int"].cpu().numpy(), fx[f"{t}_users_int"])
        got_lists[t] = i
    same, det, total = lists_vs_reference(fx, tables, got_lists, min_frac=0.5)
    print(f"GAR {cold}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    results = dict(overall=tr.overall_test_results, cold=tr.cold_test_results, warm=tr.warm_test_results)
    metrics_vs_reference(results, fx, same == total, tr.bestPerformance[1]["NDCG"])
    lines = json.loads(str(fx["loss_lines"]))
    assert len(lines) == 2 and [float(l.split("batch_loss:")[1]) for l in lines] == pytest.approx(
        list(tr.batch_losses[[0, 8], 3]), rel=RUN_LOSS_BAR)


def test_second_run_is_bit_identical(toy_run):
    cold, _, a, where = toy_run
    b = _run(where, cold)
    assert np.array_equal(a.batch_losses, b.batch_losses)
    assert torch.equal(a.user_emb, b.user_emb) and torch.equal(a.item_emb, b.item_emb)


@pytest.mark.parametrize("cold", ["item", "user"])
def test_cli_trains_end_to_end(cold, tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", cold, "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "MF", "--make_synthetic", "toy"] + common) is None
    main(["--model", "MF", "--epochs", "1"] + common)
    loaded = {s: torch.load(tmp_path / "emb" / f"toy_cold_{cold}_MF_{s}_emb.pt", map_location="cpu").detach()
              for s in ("user", "item")}
    pay = main(["--model", "GAR", "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "GAR" / "history.txt").is_file()
    out = {s: torch.load(tmp_path / "emb" / f"toy_cold_{cold}_GAR_{s}_emb.pt", map_location="cpu") for s in ("user", "item")}
    for s in ("user", "item"):
        assert out[s].shape == loaded[s].shape and torch.isfinite(out[s]).all() and not torch.equal(out[s], loaded[s])
