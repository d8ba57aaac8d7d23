"""The screened ranking's certificate against a host model of its bound (run with -m gpu on an MI355X).

Every other screen test runs inputs whose gap between the 20th and the 28th score is 20 .. 100 times B_u, so none of them sees
the size of the bound.  Here the inputs (tests/screen_cases.py) put the gap inside the range B_u sweeps over the users of one
call, on grids where the approximate and the exact score are exact: the number of uncertified users is the position at which
B_u crosses the gap, and oracle/screen_model.py (validated on the CPU by tests/test_screen_certificate.py) says where that is.
Every case asserts: the screened call (CRH_SCORE_SCREEN=2) equals the exact route (CRH_SCORE_SCREEN=0) bit for bit for every
user, sampled users equal the C oracle, and ``ops.score_topk_uncertified()`` equals the model's count -- users whose model
margin is inside the guard band |e_k - (A_last + B_u)| < 1e-4 B_u may fall either way (the kernel and the model evaluate one
fp64 formula in different operation orders; the CPU module caps the band at 2 % of a sweep).

What a wrong bound would do, by the model (400 x 5 003, k = 20, uncertified users; the GPU count must equal the first column):
    sweep   sound   without |u| R   without |u - u^| N^   without g_d |u| N   without g' |u^| N^
    a       192     192             192                   126                 0
    b       197     0               197                   161                 0
    c       198     198             0                     172                 0
    d       198     198             0                     190                 0
and with the maxima R, N, N^ taken over a bitmap-masked row as well: 396 .. 400 (tests/test_screen_certificate.py prints each)."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops
from oracle import oracle_np as orc
from oracle import screen_model as sm
from tests import screen_cases as sc

pytestmark = pytest.mark.gpu

K = sc.K
GUARD = 1.0e-4


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _run(monkeypatch, mode, case, k, users=None, compact=1, order=1):
    dev = _dev()
    U, V, rated, bitmap_ids, item_base = case["U"], case["V"], case["rated"], case["bitmap_ids"], case["item_base"]
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    monkeypatch.setenv("CRH_SCORE_SCREEN_COMPACT", str(compact))
    monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", str(order))
    n_users = U.shape[0] if users is None else len(users)
    rp, rc = ops.rated_csr(rated, dev) if rated is not None else (None, None)
    bm = ops.make_bitmap(item_base + V.shape[0], bitmap_ids, dev) if bitmap_ids is not None else None
    route = ops.score_topk_route(n_users, V.shape[0], V.shape[1], k, has_bitmap=bm is not None)
    plan = ops.score_topk_screen_plan(n_users, V.shape[0], V.shape[1], k, has_bitmap=bm is not None) if route["screened"] else None
    ut = None if users is None else torch.from_numpy(np.asarray(users, np.int32)).to(dev)
    s, i = ops.score_topk(torch.from_numpy(U).to(dev), ut, torch.from_numpy(V).to(dev), k, rp, rc, bm, item_base=item_base)
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if route["screened"] else None
    return s.cpu().numpy(), i.cpu().numpy(), route, plan, unc


_exact_cache = {}
_case_cache = {}
_model_cache = {}


def _case(name, build):
    if name not in _case_cache:
        _case_cache[name] = build()
    return _case_cache[name]


def _model(name, case, k, users):
    if name not in _model_cache:
        _model_cache[name] = sc.model(case, k=k, users=users)
    return _model_cache[name]


def _exact(monkeypatch, name, case, k, users, n_sample):
    """The exact route's answer of a case (cached under `name`), checked against the oracle on sampled users when first computed."""
    if name not in _exact_cache:
        s0, i0, r0, _, _ = _run(monkeypatch, 0, case, k, users)
        assert not r0["screened"]
        n_users = s0.shape[0]
        pick = np.unique(np.concatenate([np.random.default_rng(0).integers(0, n_users, n_sample), [0, n_users - 1]]))
        rows = pick if users is None else np.asarray(users)[pick]
        rowptr = col = None
        if case["rated"] is not None:
            rr = [case["rated"][j] for j in pick]
            rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
            col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
        bm = orc.make_bitmap(case["item_base"] + case["V"].shape[0], case["bitmap_ids"]) if case["bitmap_ids"] is not None else None
        ws, wi = orc.score_topk(case["U"], rows.astype(np.int64), case["V"], k, rowptr, col, bm, item_base=case["item_base"])
        assert np.array_equal(i0[pick], wi)
        assert np.array_equal(s0[pick].view(np.uint32), ws.view(np.uint32))
        s0.setflags(write=False)
        i0.setflags(write=False)
        _exact_cache[name] = (s0, i0)
    return _exact_cache[name]


def _check(monkeypatch, name, case, k=K, users=None, compact=1, order=1, n_sample=12):
    """Screened == exact for every user, exact == oracle on sampled users, uncertified count == the model's outside the guard band.
    Returns (uncertified, model result, plan, route, screened ids)."""
    res = _model(name, case, k, users)
    lo, inside = sm.guarded_count(res, GUARD)
    assert inside <= 0.02 * len(res["cert"]), inside         # (the cap of tests/test_screen_certificate.py, for every case here)
    s0, i0 = _exact(monkeypatch, name, case, k, users, n_sample)
    s2, i2, r2, plan, unc = _run(monkeypatch, 2, case, k, users, compact, order)
    assert r2["screened"], r2
    assert plan["compact"] == (case["bitmap_ids"] is not None and compact == 1), plan
    print("%s (compact %d, order %d): %d of %d users uncertified; model %d outside a guard band of %d"
          % (name, compact, order, unc, s2.shape[0], lo, inside))
    assert np.array_equal(i2, i0), np.argwhere((i2 != i0).any(1))[:5]
    assert np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
    assert lo <= unc <= lo + inside, (unc, lo, inside)
    return unc, res, plan, r2, i2


# ---- the four sweeps at 400 users x 5 003 items
@pytest.mark.parametrize("kind", "abcd")
def test_sweep(monkeypatch, kind):
    name = "sweep-%s" % kind
    unc, res, _, _, _ = _check(monkeypatch, name, _case(name, lambda: sc.sweep(kind)))
    assert 100 < unc < 300           # (the crossing is inside the sweep: tests/test_screen_certificate.py)


@pytest.mark.parametrize("compact,order", [(1, 1), (1, 0), (0, 0)])
@pytest.mark.parametrize("mask", ["R", "N"])
@pytest.mark.parametrize("kind", "abcd")
def test_sweep_bitmap_masks_the_row_of_a_maximum(monkeypatch, kind, mask, compact, order):
    """A bitmap masks the row that would set R (sweep b: R comes from the next row; the others: R = 0 although a masked row is off
    the grid) or N and N^, with a fifth of the background.  With that row counted in, 396 .. 400 users would be uncertified."""
    name = "sweep-%s/mask-%s" % (kind, mask)
    case = _case(name, lambda: sc.sweep(kind, mask=mask))
    if compact and order:
        monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
        monkeypatch.setenv("CRH_SCORE_SCREEN_COMPACT", "1")
        monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", "1")
        assert ops.score_topk_screen_ordered(case["U"].shape[0], case["V"].shape[0], 128, K, has_bitmap=True)
    unc, _, _, _, _ = _check(monkeypatch, name, case, compact=compact, order=order)
    assert 100 < unc < 300


@pytest.mark.parametrize("kind", "abcd")
def test_sweep_rated(monkeypatch, kind):
    """User j rates the plant of rank 21 + j % 8: the 29th plant ends its list, every rank behind the rated one shifts by one."""
    name = "sweep-%s/rated" % kind
    case = _case(name, lambda: sc.sweep(kind, rated=True))
    unc, res, _, _, got = _check(monkeypatch, name, case)
    for j in (0, 1, 7, 8, 398):
        assert case["rated"][j][0] not in res["cand"][j] and case["plant_ids"][28] in res["cand"][j]
    if kind != "d":                  # (sweep d: the nine lower plants tie in the approximate score; A_last does not move)
        plain = sm.guarded_count(_model("sweep-%s" % kind, _case("sweep-%s" % kind, lambda: sc.sweep(kind)), K, None), GUARD)[0]
        assert plain - unc >= 5      # A_last fell by 6 * 2^-18


# ---- one sweep at 70 001 items: the screen ranks a seeded prefix of 8 192 items first (screen_prefix: shards of >= 65 536 items).
# score_topk_route describes the exact route the screen replaces; that one is seeded here as well, with a longer prefix
@pytest.mark.parametrize("where", ["plants in the prefix", "ballast in the prefix", "ballast in the prefix, r1 masked"])
def test_sweep_seeded_prefix(monkeypatch, where):
    n_items, P, main0 = 70_001, 8192, 16_384

    def build():
        rng = np.random.default_rng(70)
        if where == "plants in the prefix":
            plants, ballast = rng.choice(P, sc.N_PLANTS, replace=False), main0 + rng.choice(n_items - main0, 4, replace=False)
        else:
            plants, ballast = main0 + rng.choice(n_items - main0, sc.N_PLANTS, replace=False), rng.choice(P, 4, replace=False)
        return sc.sweep("b", n_items=n_items, plant_ids=plants, ballast_ids=ballast, mask="R" if "masked" in where else None)
    name = "prefix/" + where
    unc, _, _, route, _ = _check(monkeypatch, name, _case(name, build))
    assert route["seeded"] and P <= route["prefix_items"] < main0, route
    assert 100 < unc < 300


# ---- few users: the fp16 pass is cut (44 cuts of the 91 811 items behind the seeded prefix).  The plants sit in the first cuts of
# an off-grid shard, the rows that set R and N in the last ones
def test_sweep_cuts_off_grid_base(monkeypatch):
    n_users, n_items, base = 40, 100_003, 1_000_003

    def build():
        rng = np.random.default_rng(44)
        plants = 10_000 + rng.choice(10_000, sc.N_PLANTS, replace=False)
        ballast = n_items - 1 - rng.choice(10_000, 4, replace=False)
        return sc.sweep("b", n_users=n_users, n_items=n_items, plant_ids=plants, ballast_ids=ballast, item_base=base)
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    assert ops.score_topk_screen_plan(n_users, n_items, 128, K, has_bitmap=False)["cuts"] > 8
    unc, _, plan, _, _ = _check(monkeypatch, "cuts", _case("cuts", build), n_sample=4)
    assert plan["cuts"] > 8          # (more than 8 cuts of the main range: ids 10 000 .. 20 000 and the last 10 000 never share one)
    assert 10 < unc < 30


# ---- scale invariance: powers of two change no rounding, so the same users certify
@pytest.mark.parametrize("eu,ev", [(40, -30), (-40, 20)])
def test_scale_invariance(monkeypatch, eu, ev):
    base = _case("sweep-a", lambda: sc.sweep("a"))
    name = "scaled/%d/%d" % (eu, ev)
    case = _case(name, lambda: dict(base, U=np.ldexp(base["U"], eu), V=np.ldexp(base["V"], ev)))
    assert np.array_equal(np.ldexp(case["U"], -eu), base["U"]) and np.array_equal(np.ldexp(case["V"], -ev), base["V"])
    unc, res, _, _, _ = _check(monkeypatch, name, case)
    plain = _model("sweep-a", base, K, None)
    assert np.array_equal(res["cert"], plain["cert"])
    assert unc == int((~plain["cert"]).sum())            # (sweep a's guard band is empty)


# ---- users through an index vector with repeats: the sweep permuted, the user scale from the selected rows only
def test_users_index_vector(monkeypatch):
    base = _case("sweep-a", lambda: sc.sweep("a"))
    n = base["U"].shape[0]
    rng = np.random.default_rng(5)
    users = np.concatenate([rng.permutation(n), rng.integers(0, n, 23)]).astype(np.int32)
    huge = np.full((1, 128), 2.0 ** 30, np.float32)      # not selected: as a scale setter it would flush every knob
    case = _case("users", lambda: dict(base, U=np.concatenate([base["U"][:100], huge, base["U"][100:]])))
    users = users + (users >= 100)
    unc, res, _, _, _ = _check(monkeypatch, "users", case, users=users)
    plain = _model("sweep-a", base, K, None)
    assert np.array_equal(res["cert"], plain["cert"][users - (users > 100)])
    assert unc == int((~res["cert"]).sum())


# ---- the two refusal cases: only a sound bound gives the right answer
@pytest.mark.parametrize("side", ["item", "user"])
def test_refusal(monkeypatch, side):
    name = "refusal/" + side
    case = _case(name, sc.refusal_item_side if side == "item" else sc.refusal_user_side)
    unc, res, _, _, got = _check(monkeypatch, name, case, n_sample=5)          # (five users: the oracle checks them all)
    u = case["victim_user"]
    assert not res["cert"][u] and unc == 1
    assert got[u, 0] == case["victim"]
    assert case["victim"] not in res["cand"][u]          # the fp16 pass did not deliver it: the fallback did


# ---- k = 1 and k = 20 on sweep a
@pytest.mark.parametrize("k", [1, 20])
def test_k(monkeypatch, k):
    base = _case("sweep-a", lambda: sc.sweep("a"))
    unc, res, _, _, _ = _check(monkeypatch, "sweep-a" if k == K else "sweep-a/k1", base, k=k)
    if k == 1:                       # e_1 is the best plant, 19/64 + g above A_last: every user certifies
        assert unc == 0
    else:
        assert unc == int((~res["cert"]).sum()) and 100 < unc < 300
