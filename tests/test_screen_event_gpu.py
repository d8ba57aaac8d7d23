"""The slow-path event of the screened route's fp16 pass (run with -m gpu on an MI355X).

Round 17 shortened what the 16x16 event executes: the kernel is compiled for K' = 28 (list addresses, the tail entry's lane and the
fill tests are immediates), the per-lane `slot >= n_users` test is gone (padding columns and dead waves are kept out by their +inf
thresholds alone), the clamped rows of a cut's last tile are told by one 32-bit scalar per event, and the hit mask of a user block
is one asm statement.  None of that may change an insert.

As in the other screen tests a wrong list does not corrupt the call's output -- the exact rescoring and the certificate see to
that -- it moves A_last and with it the number of uncertified users.  So the tables sit on the exact grids of
tests/screen_cases.py, where the approximate scores are exact numbers and oracle/screen_model.py says how many users certify,
and every case asserts: the screened call (CRH_SCORE_SCREEN=2) equals the exact route (CRH_SCORE_SCREEN=0) bit for bit for every
user, sampled users equal the C oracle, the uncertified count equals the model's (users inside the guard band of
tests/test_screen_certificate_gpu.py may fall either way), and a second screened run gives equal bits and an equal count.

Shapes: a few hundred users x 5 000 .. 9 000 items -- no seeded prefix, so the lists start empty and the `n < K'` inserts run --
and one seeded case of 65 765 items (prefix 8 192, the main range in cuts).

What the cases cannot see: WHICH of two candidates of equal approximate score sits at a list's tail.  The tail's score is
A_last either way, and a certified user's tail is not among its k best.  The tie cases run both tie branches of crh_better
under the compile-time K' (an insert of a lower id over an equal tail, a refusal of a higher one) and assert the above."""
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
FORMS = {                      # name: (bitmap, CRH_SCORE_SCREEN_COMPACT, CRH_SCORE_SCREEN_ORDER); the first two are the 16x16 launches
    "compacted, ordered": (True, 1, 1),        # of the headline: the compacted one (under a bitmap) and the one without a bitmap
    "no bitmap": (False, 1, 1),
    "compacted, id order": (True, 1, 0),
    "bitmap, not compacted": (True, 0, 0),
}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _run(monkeypatch, mode, case, k, users, compact, order, bitmap):
    dev = _dev()
    U, V, rated, item_base = case["U"], case["V"], case["rated"], case["item_base"]
    bitmap_ids = case["bitmap_ids"] if bitmap else None
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


_cases, _exact_cache, _model_cache = {}, {}, {}


def _case(name, build):
    if name not in _cases:
        _cases[name] = build()
    return _cases[name]


def _reference(monkeypatch, name, case, k, users, bitmap, n_sample=6):
    """(exact route's scores and ids, model result) of a case with or without its bitmap: computed once, read-only.  The exact
    route is checked against the C oracle on sampled users when first computed."""
    key = (name, k, bitmap)
    if key not in _exact_cache:
        s0, i0, r0, _, _ = _run(monkeypatch, 0, case, k, users, 1, 1, bitmap)
        assert not r0["screened"]
        n_users = s0.shape[0]
        pick = np.unique(np.concatenate([np.random.default_rng(0).integers(0, n_users, n_sample), [0, n_users - 1]]))
        rows = pick if users is None else np.asarray(users)[pick]
        rowptr = col = None
        if case["rated"] is not None:
            rr = [case["rated"][j] for j in pick]
            rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
            col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
        bm = orc.make_bitmap(case["item_base"] + case["V"].shape[0], case["bitmap_ids"]) if bitmap else None
        ws, wi = orc.score_topk(case["U"], rows.astype(np.int64), case["V"], k, rowptr, col, bm, item_base=case["item_base"])
        assert np.array_equal(i0[pick], wi)
        assert np.array_equal(s0[pick].view(np.uint32), ws.view(np.uint32))
        s0.setflags(write=False)
        i0.setflags(write=False)
        _exact_cache[key] = (s0, i0)
        _model_cache[key] = sm.certify(case["U"], case["V"], k, users=users, bitmap_ids=case["bitmap_ids"] if bitmap else None,
                                       rated=case["rated"], item_base=case["item_base"])
    return _exact_cache[key], _model_cache[key]


def _check(monkeypatch, name, form, case, k=K, users=None, cuts=None):
    """One case in one stream form, twice.  Returns (screened ids, uncertified count, model result)."""
    has_bm, compact, order = FORMS[form]
    assert not has_bm or case["bitmap_ids"] is not None, "the case has no bitmap"
    (s0, i0), res = _reference(monkeypatch, name, case, k, users, has_bm)
    lo, inside = sm.guarded_count(res, GUARD)
    assert inside <= 1 + 0.02 * len(res["cert"]), inside
    got = None
    for rep in range(2):
        s2, i2, r2, plan, unc = _run(monkeypatch, 2, case, k, users, compact, order, has_bm)
        assert r2["screened"], r2
        assert plan["compact"] == (has_bm and compact == 1), plan
        assert cuts is None or (plan["cuts"] > 1) == cuts, plan
        print("%s / %s: %d of %d users uncertified; model %d outside a guard band of %d" % (name, form, unc, s2.shape[0], lo, inside))
        assert np.array_equal(i2, i0), np.argwhere((i2 != i0).any(1))[:5]
        assert np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
        assert lo <= unc <= lo + inside, (unc, lo, inside)
        if got is not None:
            assert np.array_equal(got[0].view(np.uint32), s2.view(np.uint32)) and np.array_equal(got[1], i2) and got[2] == unc
        got = (s2, i2, unc)
    return got[1], got[2], res


def _hash192(gi):
    """rated_hash192 of score_topk_dma.hip: the bit of the 192-bit membership filter that id gi sets."""
    return ((((int(gi) * 2654435761) & 0xFFFFFFFF) >> 16) * 192) >> 16


# ---- planted tiles.  Sweep a (every user ranks the items alike; its 29 plants sit in tile 1, so every user of every wave has 28 or
# 29 candidates in ONE tile: second, third ... candidates of one user, all 16 columns of all 8 blocks) plus rows that score for
# chosen users only: such a row is zero but for 2 .. 3 in a dimension where only those users hold a one.  Tiles are those of the
# stream in id order (the forms "no bitmap", "compacted, id order" -- the bitmap masks whole tiles of background, so rows keep
# their place in their tile -- and "bitmap, not compacted"); the ordered form streams the same rows in another order.
#   dim  users     tile  rows
#   3    7         60    9                     one candidate: one block, one lane, one row, a full list
#   4    21        70    3, 21 / 71: 6, 2      two candidates of one user in one tile (ascending and descending scores)
#   5    33, 35    80    12                    two users of one 16-column block
#   6    5, 100    90    30                    two blocks
#   7    130       100   0 .. 31               all 32 rows of one user, scores rising: 32 inserts into a list of 28
#   13   200       110   0 .. 25 / 111: 16, 17, 4, 20   ties: rows 16 and 17 (2.0) enter behind the 26 rows of tile 110 and fill the
#                        list, its tail is row 17; row 4 -- the event walks lane groups, so it comes later -- ties with the tail
#                        at a LOWER id and enters, row 20 ties with the new tail (row 16) at a HIGHER id and does not
#   14   203       120 +  one unrated row that sets the same filter bit as the plant user 203 rates (its filter says "maybe": the
#                        search runs, finds nothing, the row enters)
# With `rated` every user j rates the plant of rank 21 + j % 8: a candidate above the threshold that the filter and the search
# turn into a masked score.
N_ITEMS_P, N_USERS_P = 7008, 300
MASKED_TILES = [3, 10, 65, 95, 105, 150]


def _planted(rated):
    def build():
        plants = np.arange(33, 33 + sc.N_PLANTS)
        c = sc.sweep("a", n_users=N_USERS_P, n_items=N_ITEMS_P, plant_ids=plants, ballast_ids=np.array([100, 101, 102, 103]), rated=rated)
        U, V = c["U"].copy(), c["V"].copy()

        def put(dim, users, rows, scores):
            U[np.asarray(users), dim] = 1.0
            V[np.asarray(rows)] = 0.0
            V[np.asarray(rows), dim] = np.asarray(scores, np.float32)
        put(3, [7], [60 * 32 + 9], [2.0])
        put(4, [21], [70 * 32 + 3, 70 * 32 + 21, 71 * 32 + 6, 71 * 32 + 2], [2.0, 2.25, 2.25, 2.0])
        put(5, [33, 35], [80 * 32 + 12], [2.0])
        put(6, [5, 100], [90 * 32 + 30], [2.0])
        put(7, [130], 100 * 32 + np.arange(32), 2.0 + np.arange(32) / 64.0)
        put(13, [200], np.concatenate([110 * 32 + np.arange(26), 111 * 32 + np.array([16, 17, 4, 20])]),
            np.concatenate([3.0 - np.arange(26) / 64.0, [2.0, 2.0, 2.0, 2.0]]))
        coll = None
        if rated:
            want = _hash192(c["rated"][203][0])
            coll = next(i for i in range(120 * 32, N_ITEMS_P) if _hash192(i) == want and i // 32 not in MASKED_TILES)
            put(14, [203], [coll], [2.0])
        cold = np.concatenate([32 * t + np.arange(32) for t in MASKED_TILES])
        return dict(c, U=U, V=V, bitmap_ids=cold, coll=coll)
    return _case("planted rated" if rated else "planted", build)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("rated", [False, True])
def test_planted_tiles(monkeypatch, form, rated):
    c = _planted(rated)
    got, _, res = _check(monkeypatch, "planted rated" if rated else "planted", form, c)
    assert got[7, 0] == 60 * 32 + 9 and got[33, 0] == got[35, 0] == 80 * 32 + 12 and got[5, 0] == got[100, 0] == 90 * 32 + 30
    assert list(got[21, :4]) == [70 * 32 + 21, 71 * 32 + 6, 70 * 32 + 3, 71 * 32 + 2]
    assert list(got[130]) == list(100 * 32 + 31 - np.arange(K))
    assert list(got[200]) == list(110 * 32 + np.arange(K))
    # the model's K' lists of the tie user end in rows 4 and 16 of tile 111 (approximate 2.0, the lower ids of the four)
    assert list(res["cand"][200, 26:]) == [111 * 32 + 4, 111 * 32 + 16]
    if rated:
        assert got[203, 0] == c["coll"] and _hash192(c["coll"]) == _hash192(c["rated"][203][0])
        for j in (0, 7, 203):
            assert c["rated"][j][0] not in got[j] and c["rated"][j][0] not in res["cand"][j]


# ---- padding columns and dead waves.  The event has no test of its own that keeps a padding column or a dead wave out: their
# thresholds are +inf.  Slices of one sweep of 600 users, centred on the user at which B_u crosses the gap (so that a slice holds
# both kinds): 1, 15, 17 users (one block and a bit), 127, 129 (waves 2 and 3 of the workgroup dead), 511, 513 and 600 (the
# second workgroup: one column, or 88, and three dead waves).  The sweep under a bitmap is built with one, the other without.
@pytest.mark.parametrize("n_users", [1, 15, 17, 127, 129, 511, 513, 600])
def test_padding_and_dead_waves(monkeypatch, n_users):
    first = max(0, min(300 - n_users // 2, 600 - n_users))
    for form, mask in (("compacted, ordered", "N"), ("no bitmap", None)):
        base = _case("waves %s" % mask, lambda: sc.sweep("a", n_users=600, n_items=5003, mask=mask))
        c = dict(base, U=base["U"][first:first + n_users])
        _, unc, _ = _check(monkeypatch, "waves %d %s" % (n_users, mask), form, c)
        assert n_users < 100 or 0 < unc < n_users         # (the crossing, user 302 or 312, is inside the wider slices)


# ---- the ragged last tile.  Users 0 .. 99 score every row NEGATIVE (u_0 = -1 against v_0 > 0), users 100 .. 199 positive: the
# zero rows behind the last live row of a clamped tail tile would beat every threshold of the first hundred.  Live counts
# 32 m + 1 and 32 m + 31 under a bitmap (the compacted stream's row count), 28 and 11 live rows (K' and fewer: the lists never
# fill and the users cannot certify), and the same counts as the table's own length without a bitmap.
def _signed(n_live, n_items):
    def build():
        rng = np.random.default_rng(9000 + n_live)
        V = np.zeros((n_items, 128), np.float32)
        V[:, 0] = rng.integers(8, 65, n_items) * 2.0 ** -6              # 1/8 .. 1
        V[:, 1] = rng.integers(-32, 33, n_items) * 2.0 ** -6
        V[:, 16:] = rng.integers(-4, 5, (n_items, 112)) * 2.0 ** -6
        U = np.zeros((200, 128), np.float32)
        U[:100, 0], U[100:, 0] = -1.0, 1.0
        U[:, 1] = 2.0 ** -8
        U[:, 2] = (512.0 + np.arange(200)) * 2.0 ** -10                  # a knob: |u| differs, no score does
        cold = np.sort(rng.choice(n_items, n_items - n_live, replace=False))
        return dict(U=U, V=V, bitmap_ids=cold, rated=None, item_base=0)
    return _case("signed %d of %d" % (n_live, n_items), build)


@pytest.mark.parametrize("n_live", [32 * 160 + 1, 32 * 160 + 31, 32 * 1 + 1, 28, 11])
def test_ragged_last_tile(monkeypatch, n_live):
    c = _signed(n_live, 6400)
    for form in ("compacted, ordered", "compacted, id order"):
        got, unc, _ = _check(monkeypatch, "signed %d" % n_live, form, c)
        # (behind the live rows a short answer is filled up with masked ones, as the exact route fills it)
        assert np.isin(got[:, :min(K, n_live)], np.setdiff1d(np.arange(6400), c["bitmap_ids"])).all()
        assert n_live >= 28 or unc == 200                # (a list that is not full certifies nobody)
    # the same row counts as the whole table, every row streamed: the not-compacted 16x16 launch and its tail test
    _check(monkeypatch, "signed whole %d" % n_live, "no bitmap", dict(c, V=c["V"][:n_live], bitmap_ids=None))


# ---- k = 1 and a users vector with repeats, on sweep a under a bitmap and without one
def _sweep_a(form):
    """Sweep a of tests/screen_cases.py, built under a bitmap for the forms that have one."""
    mask = "N" if FORMS[form][0] else None
    return "sweep a %s" % mask, _case("sweep a %s" % mask, lambda: sc.sweep("a", mask=mask))


@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
def test_k1(monkeypatch, form):
    name, c = _sweep_a(form)
    _, unc, _ = _check(monkeypatch, name + " k1", form, c, k=1)
    assert unc == 0                  # e_1 is the best plant, 19/64 + g above A_last


@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
def test_users_vector_with_repeats(monkeypatch, form):
    name, c = _sweep_a(form)
    n = c["U"].shape[0]
    rng = np.random.default_rng(5)
    users = np.concatenate([rng.permutation(n), rng.integers(0, n, 23), [7, 7, 7]]).astype(np.int32)
    _, unc, res = _check(monkeypatch, name + " users", form, c, users=users)
    assert unc == int((~res["cert"]).sum()) and 100 < unc < 300


# ---- seeded thresholds and cuts: 65 765 items (prefix 8 192; 150 users, so the main range is cut).  "main": the plants lie in
# the main range, spread over the cuts, and enter full, seeded lists; "prefix": they lie in the prefix and no row of the main
# range beats a threshold.
@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
@pytest.mark.parametrize("where", ["main", "prefix"])
def test_seeded_and_cut(monkeypatch, where, form):
    n_items, P = 65765, 8192

    def build():
        rng = np.random.default_rng(65)
        plants = P + rng.choice(n_items - P, sc.N_PLANTS, replace=False) if where == "main" else rng.choice(P, sc.N_PLANTS, replace=False)
        ballast = np.setdiff1d(P + rng.choice(n_items - P, 8, replace=False), plants)[:4]
        return sc.sweep("a", n_users=150, n_items=n_items, plant_ids=plants, ballast_ids=ballast, mask="N" if FORMS[form][0] else None,
                        item_base=1_000_003)
    name = "seeded %s %s" % (where, FORMS[form][0])
    _, unc, _ = _check(monkeypatch, name, form, _case(name, build), cuts=True)
    assert 30 < unc < 120            # (the crossing is inside the sweep)
