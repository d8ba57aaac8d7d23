"""The margin rule of the screened route's fp16 pass on the GPU (run with -m gpu on an MI355X).

Once a list's tail is an item, the pass takes max(tail, L[k-1] - M) for the user's threshold, M > 2 B_u: rows that can never reach
the exact top k enter no list.  The rule may move neither an output nor the number of uncertified users.  As in
tests/test_screen_event_gpu.py (whose grids, helpers and checks are used as they are) the tables sit on exact grids, where
oracle/screen_model.py says how many users certify, and every case asserts: the screened call equals the exact route bit for bit,
sampled users equal the C oracle, the uncertified count equals the model's, a second run gives the same -- and here also: the call
with CRH_SCORE_SCREEN_MARGIN=0 (M = +inf, the thresholds are the tails) in the same process gives the same bits and the same count.

The sweeps of tests/screen_cases.py put the eight lower plants about one B_u below the 20th, where the rule never cuts (a_k - M lies
below the tail).  The "wide" cases here put them THREE bounds of the middle user below it and let |u| run from 1 to 8, so that one
call holds users with A < a_k - 2 B_u (the rule supplies their threshold; they certify), users with A >= a_k - 2 B_u that certify,
and users that do not certify -- the model says which, and the test asserts that every kind is present.
"""
import numpy as np
import pytest

from oracle import screen_model as sm
from tests import screen_cases as sc
from tests import test_screen_event_gpu as ev

pytestmark = pytest.mark.gpu

K = sc.K
OFF_GRID_BASE = 1_000_003


def _check(monkeypatch, name, form, case, k=K, users=None, cuts=None):
    """ev._check with the rule on (twice), then the same call with the rule off: equal bits, equal count."""
    monkeypatch.setenv("CRH_SCORE_SCREEN_MARGIN", "1")
    ids, unc, res = ev._check(monkeypatch, name, form, case, k=k, users=users, cuts=cuts)
    has_bm, compact, order = ev.FORMS[form]
    (s0, i0), _ = ev._reference(monkeypatch, name, case, k, users, has_bm)
    monkeypatch.setenv("CRH_SCORE_SCREEN_MARGIN", "0")
    s_off, i_off, r_off, _, unc_off = ev._run(monkeypatch, 2, case, k, users, compact, order, has_bm)
    assert r_off["screened"]
    print("%s / %s: rule on %d uncertified, rule off %d" % (name, form, unc, unc_off))
    assert np.array_equal(i_off, i0) and np.array_equal(s_off.view(np.uint32), s0.view(np.uint32))
    assert unc_off == unc, (unc_off, unc)
    return ids, unc, res


def _kinds(res, k=K):
    """(users whose final tail lies below a_k - 2 B_u, certified users) of a model result."""
    a_k, A = res["a_cand"][:, k - 1], res["a_cand"][:, sm.KP - 1]
    return (A < a_k - 2.0 * res["B"]), res["cert"]


def _wide(n_users, n_items, mask, plant_ids=None, ballast_ids=None, item_base=0, scale=1.0, rated=False):
    """Sweep a with the lower plants three bounds of a middle user below the 20th and |u| from 1 to 8 (knob j / 16 on the grid)."""
    c = sc.sweep("a", n_users=n_users, n_items=n_items, mask=mask, plant_ids=plant_ids, ballast_ids=ballast_ids, item_base=item_base,
                 rated=rated)
    g = float(np.ceil(3.0 * c["g"] / sc.DELTA) * sc.DELTA)
    V = sc._items("a", n_items, g, c["plant_ids"], c["ballast"], 7)
    U = c["U"].copy()
    U[:, 2] = np.floor(np.arange(n_users) * (127.0 / max(1, n_users - 1))) / 16.0
    return dict(c, U=U, V=(V * np.float32(scale)).astype(np.float32), g=g * scale)


def _assert_all_kinds(res, k=K):
    thin, cert = _kinds(res, k)
    assert (thin & cert).any() and (~thin & cert).any() and (~cert).any(), (int(thin.sum()), int(cert.sum()))
    assert not (thin & ~cert).any()                  # A < a_k - 2 B_u certifies (the proof's second case)


# ---- unseeded lists (400 x 5 003): they start empty, the rule stays off until a tail is an item; every stream form
@pytest.mark.parametrize("form", list(ev.FORMS))
def test_unseeded_forms(monkeypatch, form):
    mask = "N" if ev.FORMS[form][0] else None
    name = "margin wide %s" % mask
    c = ev._case(name, lambda: _wide(400, 5003, mask))
    _, unc, res = _check(monkeypatch, name, form, c)
    _assert_all_kinds(res)
    assert 0 < unc < 400


@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
def test_unseeded_sweep_a(monkeypatch, form):
    """The sweep of the other screen tests: a_k - M lies below every tail, the rule supplies no threshold at all."""
    name, c = ev._sweep_a(form)
    _, unc, res = _check(monkeypatch, name, form, c)
    assert not _kinds(res)[0].any() and 100 < unc < 300


# ---- seeded lists behind the 8 192-row prefix, off-grid base: the full-list form of the event; the plants lie in the main range
def _seeded(n_users, n_items, mask, rated=False):
    rng = np.random.default_rng(66)
    P = 8192
    plants = P + rng.choice(n_items - P, sc.N_PLANTS, replace=False)
    ballast = np.setdiff1d(P + rng.choice(n_items - P, 8, replace=False), plants)[:4]
    return _wide(n_users, n_items, mask, plant_ids=plants, ballast_ids=ballast, item_base=OFF_GRID_BASE, rated=rated)


@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap", "bitmap, not compacted"])
def test_seeded_full_lists(monkeypatch, form):
    mask = "N" if ev.FORMS[form][0] else None
    name = "margin seeded %s" % mask
    c = ev._case(name, lambda: _seeded(150, 65765, mask))
    _, unc, res = _check(monkeypatch, name, form, c, cuts=True)
    _assert_all_kinds(res)
    assert 0 < unc < 150


@pytest.mark.parametrize("form", ["compacted, id order", "no bitmap"])
def test_seeded_cuts_rated(monkeypatch, form):
    """40 users x 100 003 items: more cuts; every user rates one of the lower plants (a candidate that enters at -1e9)."""
    mask = "N" if ev.FORMS[form][0] else None
    name = "margin cuts %s" % mask
    c = ev._case(name, lambda: _seeded(40, 100_003, mask, rated=True))
    _, _, res = _check(monkeypatch, name, form, c, cuts=True)
    _assert_all_kinds(res)


def test_seeds_ending_in_masked_entries(monkeypatch):
    """A bitmap leaves 20 live rows in the prefix: every seed list is full, its last eight entries are masked rows at -1e9 and its
    threshold -inf.  The rule must stay off until items of the main range have pushed them out, then engage."""
    name = "margin masked seeds"

    def build():
        c = _seeded(150, 65765, "N")
        keep = np.random.default_rng(3).choice(8192, 20, replace=False)
        cold = np.union1d(c["bitmap_ids"], np.setdiff1d(np.arange(8192), keep) + OFF_GRID_BASE)
        return dict(c, bitmap_ids=cold)
    c = ev._case(name, build)
    for form in ("compacted, ordered", "bitmap, not compacted"):
        _, _, res = _check(monkeypatch, name, form, c, cuts=True)
        _assert_all_kinds(res)


# ---- 11, 27, 28 and 29 live rows: lists that never fill, fill exactly, and see one row more
@pytest.mark.parametrize("n_live", [11, 27, 28, 29])
def test_live_row_counts(monkeypatch, n_live):
    c = ev._signed(n_live, 6400)
    for form in ("compacted, ordered", "compacted, id order"):
        _, unc, _ = _check(monkeypatch, "signed %d" % n_live, form, c)
        assert n_live >= 28 or unc == 200
    _check(monkeypatch, "signed whole %d" % n_live, "no bitmap", dict(c, V=c["V"][:n_live], bitmap_ids=None))


# ---- k = 1: L[k-1] is the list's head
@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
def test_k1(monkeypatch, form):
    mask = "N" if ev.FORMS[form][0] else None
    name = "margin wide %s" % mask
    c = ev._case(name, lambda: _wide(400, 5003, mask))
    _, unc, res = _check(monkeypatch, name + " k1", form, c, k=1)
    assert unc == 0 and _kinds(res, 1)[0].all()      # the best plant is 19/64 above the 20th, far above every bound and the tail
    name = "margin seeded %s" % mask
    c = ev._case(name, lambda: _seeded(150, 65765, mask))
    _, unc, _ = _check(monkeypatch, name + " k1", form, c, k=1, cuts=True)
    assert unc == 0


# ---- a table scaled by 2^40 and by 2^-40: M is scaled by the exact powers of two of the table scales
@pytest.mark.parametrize("e", [40, -40])
def test_scaled_table(monkeypatch, e):
    name = "margin scaled %d" % e
    c = ev._case(name, lambda: _wide(400, 5003, None, scale=2.0 ** e))
    _, unc, res = _check(monkeypatch, name, "no bitmap", c)
    _assert_all_kinds(res)
    one = _wide(400, 5003, None)
    assert np.array_equal(sm.certify(one["U"], one["V"], K)["cert"], res["cert"])          # a power of two moves nobody


# ---- one non-finite user row: its norms are +inf, so is the call's largest bound, and M = +inf switches the rule off for the call
def test_nonfinite_user_row(monkeypatch):
    name = "margin nonfinite"

    def build():
        c = _seeded(150, 65765, None)
        U = c["U"].copy()
        U[77, 3] = np.inf
        return dict(c, U=U)
    c = ev._case(name, build)
    finite = np.setdiff1d(np.arange(150), [77])
    res = sm.certify(c["U"], c["V"], K, users=finite, item_base=c["item_base"])
    lo, inside = sm.guarded_count(res, ev.GUARD)
    s0, i0, r0, _, _ = ev._run(monkeypatch, 0, c, K, None, 1, 1, False)
    assert not r0["screened"]
    first = None
    for margin in ("1", "0", "1"):
        monkeypatch.setenv("CRH_SCORE_SCREEN_MARGIN", margin)
        s2, i2, r2, _, unc = ev._run(monkeypatch, 2, c, K, None, 1, 1, False)
        assert r2["screened"]
        print("%s, CRH_SCORE_SCREEN_MARGIN=%s: %d uncertified; model %d of the finite users, %d in the guard band" % (name, margin, unc, lo, inside))
        assert np.array_equal(i2, i0) and np.array_equal(s2.view(np.uint32), s0.view(np.uint32))     # exact through the fallback
        assert lo + 1 <= unc <= lo + 1 + inside, (unc, lo, inside)      # the model's count of the finite users, and user 77
        assert first is None or first == unc
        first = unc


# ---- the margin refusal: an input on which only M > 2 B_u gives the right answer (after the item-side refusal of
# tests/screen_cases.py).  User 0 is 1 in all 128 dimensions.  The victim row is 1 + 0.49 * 2^-10 everywhere: approximate score 128,
# exact score 128 + 62.7 ulps (ulp = 2^-10), the best of the table.  Twenty decoys hold H = 105 .. 114 components 0.49 ulps BELOW
# 1 + 2^-10 and ones elsewhere: approximate 128 + H ulps, exact 128 + 0.51 H <= 128 + 58.2 ulps -- below the victim.  B_u is
# 95.8 ulps, so the victim's approximate score lies 105 ulps, between B_u and 2 B_u, below a_k.  Eight rows with a zero component
# score 127 + t ulps: the list is wide, A < a_k - 3 B_u, and the user certifies.  The decoys and the eight come first in the stream, the
# victim last: with M > 2 B_u it is a candidate (a_k - M < 128) and ends as the user's best item; with M halved (about B_u) the
# threshold is 128 + 9 ulps, the row never enters a list, and the call either returns a certified list without it or -- through
# stage 2's clause -- refuses a user the model certifies.
def refusal_margin(n_items=3001, seed=13):
    rng = np.random.default_rng(seed)
    V = sc._refusal_background(rng, n_items)
    V[:, 64:] = V[:, :64]                                               # background scores <= 64 against the user of ones
    ulp = 2.0 ** -10
    decoys, lows, pads, victim = np.arange(40, 60), np.arange(100, 108), np.arange(200, 220), 2900
    for r, row in enumerate(decoys):
        V[row] = 1.0
        V[row, :105 + (19 - r) // 2] = np.float32(1.0 + 0.51 * ulp)
    for t, row in enumerate(lows):
        V[row] = 1.0
        V[row, 127] = 0.0
        V[row, :t] = 1.0 + ulp
    V[victim] = np.float32(1.0 + 0.49 * ulp)
    V[pads] = 0.0
    V[pads, 0] = 3.0 - np.arange(20) / 64.0
    U = np.zeros((5, 128), np.float32)
    U[0] = 1.0
    U[1:, 0] = 1.0
    return dict(kind="margin", U=U, V=V.astype(np.float32), bitmap_ids=None, rated=None, item_base=0, victim=victim, victim_user=0)


def test_margin_refusal(monkeypatch):
    name = "margin refusal"
    c = ev._case(name, refusal_margin)
    res = sm.certify(c["U"], c["V"], K, check_exact=False)
    B, a = res["B"][0], res["a_cand"][0]
    gap = a[K - 1] - 128.0
    assert list(res["cand"][0]).index(c["victim"]) == K and a[K] == 128.0          # the 21st approximate score ...
    assert B < gap < 2.0 * B and a[sm.KP - 1] < a[K - 1] - 3.0 * B                  # ... between B_u and 2 B_u below a_k; a wide list
    assert res["cert"][0] and res["top"][0][0] == c["victim"]                       # certified, and the victim is the best item
    monkeypatch.setenv("CRH_SCORE_SCREEN_MARGIN", "1")
    s0, i0, r0, _, _ = ev._run(monkeypatch, 0, c, K, None, 1, 1, False)
    assert not r0["screened"] and i0[0, 0] == c["victim"]
    for rep in range(2):
        s2, i2, r2, _, unc = ev._run(monkeypatch, 2, c, K, None, 1, 1, False)
        assert r2["screened"]
        print("%s: %d uncertified, model %d" % (name, unc, int((~res["cert"]).sum())))
        assert i2[0, 0] == c["victim"]
        assert np.array_equal(i2, i0) and np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
        assert unc == int((~res["cert"]).sum())
