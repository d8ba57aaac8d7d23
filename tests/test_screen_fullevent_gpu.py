"""The full-list event of the screened route's fp16 pass (run with -m gpu on an MI355X).

Round 18 gave the 16x16 event a second form for waves whose lists are all full when the seeds have been copied (one wave-uniform
flag, worked out in the kernel's prologue): it neither reads nor writes a list's fill, and a hit block with one hit lane and one row
runs its candidate with no loop.  With the flag clear -- an unseeded call, K' read at run time -- the event of round 17 runs.  None
of that may change an insert.

The library seeds its lists from 65 536 items upwards (prefix 8 192), so the full-list form runs only in the cases of 65 765 items
below (off-grid base, the main range in cuts); the cases of a few thousand items run the other branch of the flag and are the ones
that turn red when the flag is forced to true.  All tables sit on the exact grids of tests/screen_cases.py, and every case asserts
what tests/test_screen_event_gpu.py asserts, through its helpers (one cache of cases and references for both files): the screened
call equals the exact route bit for bit, sampled users equal the C oracle, the uncertified count equals oracle/screen_model.py's,
and a second run gives the same.  A candidate that is lost, or entered where it must not, shows in the output of a certified user
(the planted users below certify: their e_k - A_last is at least 1/64) or moves A_last and the count.

What no case can see, here as there: WHICH of several candidates of equal approximate score sit at a list's tail.  Whatever the
tie rule, a list holds everything above its last score and some of the items that tie with it; A_last is the same, and an item
that ties with A_last is never among the k best of a certified user (its exact score is at most A_last + B_u < e_k).  So a
mutation of the id rule alone stays green (profiles/r18_event_mutations.log); the tie cases run both branches and assert the above."""
import numpy as np
import pytest

from tests import screen_cases as sc
from tests import test_screen_event_gpu as ev

pytestmark = pytest.mark.gpu

K = sc.K
FORMS4 = list(ev.FORMS)
N_ITEMS_S, P, BASE = 65765, 8192, 1_000_003          # the seeded shape: prefix P, ids from an off-grid base
MASKED_TILES = [3, 10, 65, 95, 105, 150]             # whole tiles of background (of the main range): rows keep their place in their tile


def _row(tile, rows):
    """Local ids of rows of tile `tile` of the main range, as the stream in id order cuts it."""
    return P + 32 * tile + np.asarray(rows)


# ---- planted tiles behind a seed prefix.  Sweep a: every user ranks the items alike, the 29 plants sit in tile 1 of the main range
# (28 or 29 candidates of every user in one tile: the loop path), plus rows that score for chosen users only (a private dimension):
#   dim  users     rows (tile of the main range: rows)          what it runs
#   3    7         60: 9                                         one candidate: the straight-line path
#   4    21        70: 2, 3                                      two rows of one lane (g = 0, r = 2 and 3)
#   5    22        72: 3, 21                                     two lanes of one user (g = 0 and g = 1)
#   6    33, 35    80: 12                                        two lanes (two users) of one 16-column block
#   7    5, 100    90: 30                                        two blocks
#   10   130       100: 0 .. 31                                  all 32 rows of one user, scores rising: 32 inserts
#   13   40        26 prefix rows 3 - i/64; 110: 16, 17, 4, 20   ties with the tail: rows 16, 17 (2.0) enter, the tail is row 17; row 4 (a
#                                                                later lane group) ties at a LOWER id and enters, row 20 ties with the
#                                                                new tail (row 16) at a HIGHER id and does not
#   14   41        10 prefix rows 3 - i/64; 112: 7               a candidate equal to a middle entry (3 - 5/64), placed behind it
#   15   42        28 prefix rows 2.5 - i/64; 115: 0, 4          row 0 (2.75) enters and lifts the tail to 2.5 - 26/64; row 4 (2.5 - 27/64 + 1/128,
#                                                                above the threshold the hit mask was taken with) is strictly below it
#   11   43        5 +: one unrated row                       sets the filter bit of the plant user 43 rates: the search runs, finds nothing
# With `rated` user j rates the plant of rank 20 + j % 8: a candidate above the threshold that must not displace a real entry.
def _planted_seeded(rated):
    def build():
        c = sc.sweep("a", n_users=300, n_items=N_ITEMS_S, plant_ids=_row(1, 1 + np.arange(sc.N_PLANTS)), ballast_ids=_row(4, np.arange(4)),
                     rated=rated, item_base=BASE)
        U, V = c["U"].copy(), c["V"].copy()

        def put(dim, users, rows, scores):
            U[np.asarray(users), dim] = 1.0
            V[np.asarray(rows)] = 0.0
            V[np.asarray(rows), dim] = np.asarray(scores, np.float32)
        put(3, [7], _row(60, [9]), [2.0])
        put(4, [21], _row(70, [2, 3]), [2.0, 2.25])
        put(5, [22], _row(72, [3, 21]), [2.0, 2.25])
        put(6, [33, 35], _row(80, [12]), [2.0])
        put(7, [5, 100], _row(90, [30]), [2.0])
        put(10, [130], _row(100, np.arange(32)), 2.0 + np.arange(32) / 64.0)
        put(13, [40], np.concatenate([1000 + np.arange(26), _row(110, [16, 17, 4, 20])]), np.concatenate([3.0 - np.arange(26) / 64.0, [2.0] * 4]))
        put(14, [41], np.concatenate([3000 + np.arange(10), _row(112, [7])]), np.concatenate([3.0 - np.arange(10) / 64.0, [3.0 - 5 / 64.0]]))
        put(15, [42], np.concatenate([2000 + np.arange(28), _row(115, [0, 4])]),
            np.concatenate([2.5 - np.arange(28) / 64.0, [2.75, 2.5 - 27 / 64.0 + 1 / 128.0]]))
        coll = None
        if rated:
            want = ev._hash192(c["rated"][43][0])
            # (close behind the plants: the filter of a cut holds the rated ids of that cut's range only)
            taken = MASKED_TILES + [4, 60, 70, 72, 80, 90, 100, 110, 112, 115]
            coll = next(i for i in range(P + 5 * 32, N_ITEMS_S) if ev._hash192(i + BASE) == want and (i - P) // 32 not in taken)
            put(11, [43], [coll], [2.0])
        cold = np.concatenate([_row(t, np.arange(32)) for t in MASKED_TILES]) + BASE
        return dict(c, U=U, V=V, bitmap_ids=cold, coll=coll)
    return ev._case("seeded planted rated" if rated else "seeded planted", build)


@pytest.mark.parametrize("form", FORMS4)
@pytest.mark.parametrize("rated", [False, True])
def test_seeded_planted_tiles(monkeypatch, form, rated):
    c = _planted_seeded(rated)
    got, _, res = ev._check(monkeypatch, "seeded planted rated" if rated else "seeded planted", form, c, cuts=True)
    g = lambda tile, rows: list(BASE + _row(tile, rows))
    assert res["cert"][[5, 7, 21, 22, 33, 35, 40, 41, 42, 100, 130]].all()          # (so their outputs are the screen's own)
    assert got[7, 0] == g(60, [9])[0] and got[33, 0] == got[35, 0] == g(80, [12])[0] and got[5, 0] == got[100, 0] == g(90, [30])[0]
    assert list(got[21, :2]) == g(70, [3, 2]) and list(got[22, :2]) == g(72, [21, 3])
    assert list(got[130]) == g(100, 31 - np.arange(K))
    assert list(got[40]) == list(BASE + 1000 + np.arange(K)) and list(res["cand"][40, 26:]) == g(110, [4, 16])
    assert list(got[41, :11]) == list(BASE + 3000 + np.arange(6)) + g(112, [7]) + list(BASE + 3006 + np.arange(4))
    assert list(got[42]) == g(115, [0]) + list(BASE + 2000 + np.arange(K - 1)) and g(115, [4])[0] not in res["cand"][42]
    if rated:
        assert res["cert"][43] and got[43, 0] == c["coll"] + BASE and ev._hash192(c["coll"] + BASE) == ev._hash192(c["rated"][43][0])
        for j in (0, 7, 43):
            assert c["rated"][j][0] not in got[j] and c["rated"][j][0] not in res["cand"][j]


# ---- k = 1 and a users vector with repeats behind the seed prefix (both 16x16 launches)
@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
def test_seeded_k1(monkeypatch, form):
    ev._check(monkeypatch, "seeded planted k1", form, _planted_seeded(False), k=1, cuts=True)


@pytest.mark.parametrize("form", ["compacted, ordered", "no bitmap"])
def test_seeded_users_vector_with_repeats(monkeypatch, form):
    c = _planted_seeded(False)
    rng = np.random.default_rng(5)
    users = np.concatenate([rng.permutation(300), rng.integers(0, 300, 23), [7, 7, 7]]).astype(np.int32)
    ev._check(monkeypatch, "seeded planted users", form, c, users=users, cuts=True)


# ---- seed lists that end in masked entries.  The prefix stage ranks a masked item at -1e9 under its own id, so a seeded list is full
# whenever the prefix holds K' rows and the wave's flag is set; what a user with fewer than K' unmasked, unrated items in the prefix
# gets is a full list whose tail is masked and a threshold of -inf.  Here the bitmap leaves 40 rows of the prefix; users 3, 17, 40
# (wave 0), 130, 200 and 230 (wave 1) rate 15 of them and start with 25 real seeds and three masked ones, everybody else with 28 real
# ones.  Under the bitmap that is not compacted their masked rows are candidates too (at -1e9, ordered by id).  The plants (tile 1 of
# the main range) push the masked entries out.  Users 200 and 230 lie behind the crossing and must not certify.
SHORT = (3, 17, 40, 130, 200, 230)


def _short_seeds():
    def build():
        c = sc.sweep("a", n_users=300, n_items=N_ITEMS_S, plant_ids=_row(1, 1 + np.arange(sc.N_PLANTS)), ballast_ids=_row(4, np.arange(4)),
                     item_base=BASE)
        kept = 100 + 7 * np.arange(40)
        rated = [kept[:15] + BASE if j in SHORT else np.zeros(0, np.int64) for j in range(300)]
        return dict(c, bitmap_ids=np.setdiff1d(np.arange(P), kept) + BASE, rated=rated)
    return ev._case("short seeds", build)


@pytest.mark.parametrize("form", ["compacted, ordered", "bitmap, not compacted"])
def test_seed_lists_with_masked_tails(monkeypatch, form):
    c = _short_seeds()
    got, unc, res = ev._check(monkeypatch, "short seeds", form, c, cuts=True)
    assert 30 < unc < 270
    assert not np.isin(got[list(SHORT)], c["rated"][3]).any() and (res["cand"] >= 0).all()
    assert not res["cert"][[200, 230]].any() and res["cert"][[3, 17, 40, 130]].all()


# ---- live rows in total: lists that never fill (11, 27), fill exactly (28) and are full after the first insert (29) or a few (33).
# Of 6 400 items (no seeds: the fill counts from 0) and of 65 765 (seeds: the prefix holds a few of the live rows, the lists are full
# of masked entries and every live row of the main range enters through the full-list form).
@pytest.mark.parametrize("n_items", [6400, N_ITEMS_S])
@pytest.mark.parametrize("n_live", [11, 27, 28, 29, 33])
def test_live_rows_in_total(monkeypatch, n_live, n_items):
    c = ev._signed(n_live, n_items)
    for form in ("compacted, ordered", "compacted, id order"):
        got, unc, _ = ev._check(monkeypatch, "signed %d of %d" % (n_live, n_items), form, c)
        assert np.isin(got[:, :min(K, n_live)], np.setdiff1d(np.arange(n_items), c["bitmap_ids"])).all()
        assert n_live >= 28 or unc == 200                # (a list that is not full certifies nobody)
    if n_items == 6400:                                  # the same row count as the whole table: the not-compacted 16x16 launch
        ev._check(monkeypatch, "signed whole %d" % n_live, "no bitmap", dict(c, V=c["V"][:n_live], bitmap_ids=None))


# ---- partial and dead waves, padding columns: slices of one sweep of 600 users centred on the crossing, without seeds (5 003 items:
# every list starts empty) and behind the seed prefix (every live slot is full, a padding slot is empty and must not clear the flag
# nor take a candidate).  16 and 128 users: a block and a wave exactly.
def _waves(seeded, mask):
    def build():
        if not seeded:
            return sc.sweep("a", n_users=600, n_items=5003, mask=mask)
        rng = np.random.default_rng(66)
        plants = P + rng.choice(N_ITEMS_S - P, sc.N_PLANTS, replace=False)
        ballast = np.setdiff1d(P + rng.choice(N_ITEMS_S - P, 8, replace=False), plants)[:4]
        return sc.sweep("a", n_users=600, n_items=N_ITEMS_S, plant_ids=plants, ballast_ids=ballast, mask=mask, item_base=BASE)
    return ev._case("waves18 %s %s" % (seeded, mask), build)


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("n_users", [1, 15, 16, 17, 127, 128, 129, 513, 600])
def test_partial_and_dead_waves(monkeypatch, n_users, seeded):
    first = max(0, min(300 - n_users // 2, 600 - n_users))
    for form, mask in (("compacted, ordered", "N"), ("no bitmap", None)):
        base = _waves(seeded, mask)
        c = dict(base, U=base["U"][first:first + n_users])
        _, unc, _ = ev._check(monkeypatch, "waves18 %d %s %s" % (n_users, seeded, mask), form, c)
        assert n_users < 100 or 0 < unc < n_users         # (the crossing is inside the wider slices)
