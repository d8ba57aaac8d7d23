"""The hand-placed tile body of the screened route's fp16 pass (run with -m gpu on an MI355X).

Round 16 re-placed the common path of score_topk_dma_kernel's 16x16 body: body 0 is peeled out of the tile loop, a loop trip is
the odd body and the even one behind it, the ring slot comes from the tile counter, the fragment reads of a tile are issued in
another order with other counted waits, and a dead wave is told apart by its thresholds (+inf) and no longer by a test per tile.
None of that may change a bit of a result.  As in tests/test_screen_mfma16_gpu.py (whose helpers these follow) a mistake here
does not corrupt the call's output -- the exact rescoring and the certificate see to that -- it leaves users uncertified.  So
every case asserts three things: the screened call (CRH_SCORE_SCREEN=2) equals the exact route (CRH_SCORE_SCREEN=0) bit for bit
for every user, sampled users equal the C oracle, and the number of uncertified users is the constant the case states.  The
constants were taken from the library of the commit before the re-placement on these inputs: the approximate scores did not
change, so the counts cannot.  Every screened call runs twice, for equal bits.

Shapes.  Below 65 536 items the screen has no seeded prefix and one cut: the main range is the whole table, its tile count the
number of streamed rows / 32 rounded up (all rows, or the rows the bitmap leaves when the stream is compacted).  Each case builds
its item count from the tile count it wants and asserts that count and the cuts and the compaction that the library plans for
the shape, so it cannot silently test another count.  Seeded thresholds and more than one cut exist from 65 536 items on (prefix 8 192, cuts of 64
or 65 tiles): one case of 65 765 items covers both, the only one above 20 000 items."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

K = 20
FORMS = {                      # name: (bitmap, CRH_SCORE_SCREEN_COMPACT, CRH_SCORE_SCREEN_ORDER)
    "compacted, ordered": (True, 1, 1),
    "compacted, id order": (True, 1, 0),
    "bitmap, not compacted": (True, 0, 0),
    "no bitmap": (False, 1, 1),
}
# uncertified users per case where it is not 0 (from the parent commit's library on the same inputs: tables with fewer live rows
# than the screen's K' = 28 or little more, where the certificate has no margin to stand on)
UNCERTIFIED = {
    "tiles 0 last 32 c / compacted, ordered": 130, "tiles 0 last 32 c / compacted, id order": 130,
    "tiles 1 last 1 c / compacted, ordered": 130, "tiles 1 last 1 c / compacted, id order": 130,
    "tiles 1 last 1 / bitmap, not compacted": 130, "tiles 1 last 1 / no bitmap": 130,
    "tiles 1 last 31 c / compacted, ordered": 75, "tiles 1 last 31 c / compacted, id order": 75,
    "tiles 1 last 31 / bitmap, not compacted": 130,
    "tiles 1 last 32 c / compacted, ordered": 60, "tiles 1 last 32 c / compacted, id order": 60,
    "tiles 1 last 32 / bitmap, not compacted": 130,
    "tiles 2 last 1 c / compacted, ordered": 40, "tiles 2 last 1 c / compacted, id order": 40,
    "tiles 2 last 1 / bitmap, not compacted": 130,
}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _run(monkeypatch, mode, U, V, rated, bitmap_ids, item_base, compact, order):
    dev = _dev()
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    monkeypatch.setenv("CRH_SCORE_SCREEN_COMPACT", str(compact))
    monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", str(order))
    rp, rc = ops.rated_csr(rated, dev) if rated is not None else (None, None)
    bm = ops.make_bitmap(item_base + V.shape[0], bitmap_ids, dev) if bitmap_ids is not None else None
    route = ops.score_topk_route(U.shape[0], V.shape[0], V.shape[1], K, has_bitmap=bm is not None)
    plan = ops.score_topk_screen_plan(U.shape[0], V.shape[0], V.shape[1], K, has_bitmap=bm is not None) if route["screened"] else None
    s, i = ops.score_topk(torch.from_numpy(U).to(dev), None, torch.from_numpy(V).to(dev), K, rp, rc, bm, item_base=item_base)
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if route["screened"] else None
    return s.cpu().numpy(), i.cpu().numpy(), route, plan, unc


_exact_cache = {}


def _exact(monkeypatch, name, U, V, rated, bitmap_ids, item_base, n_sample):
    """The exact route's answer (cached under `name`: computed once, read-only), checked against the oracle on sampled users."""
    if name not in _exact_cache:
        s0, i0, r0, _, _ = _run(monkeypatch, 0, U, V, rated, bitmap_ids, item_base, 1, 1)
        assert not r0["screened"]
        pick = np.unique(np.concatenate([[0, U.shape[0] - 1], np.random.default_rng(0).integers(0, U.shape[0], n_sample)]))
        rowptr = col = None
        if rated is not None:
            rr = [rated[j] for j in pick]
            rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
            col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
        bm = orc.make_bitmap(item_base + V.shape[0], bitmap_ids) if bitmap_ids is not None else None
        ws, wi = orc.score_topk(U, pick.astype(np.int64), V, K, rowptr, col, bm, item_base=item_base)
        assert np.array_equal(i0[pick], wi)
        assert np.array_equal(s0[pick].view(np.uint32), ws.view(np.uint32))
        s0.setflags(write=False)
        i0.setflags(write=False)
        _exact_cache[name] = (s0, i0)
    return _exact_cache[name]


def _check(monkeypatch, name, form, U, V, cold=None, rated=None, item_base=0, n_sample=4, cuts=1):
    """One case in one stream form: screened == exact for every user, twice; the plan is the one the case was built for; the
    uncertified count is noted for _counts_as_stated.  Returns the screened ids."""
    has_bm, compact, order = FORMS[form]
    bitmap_ids = (cold if cold is not None else np.zeros(0, np.int64)) if has_bm else None
    key = "%s / %s" % (name, "bitmap" if has_bm else "none")
    s0, i0 = _exact(monkeypatch, key, U, V, rated, bitmap_ids, item_base, n_sample)
    got = None
    for rep in range(2):
        s2, i2, r2, plan, unc = _run(monkeypatch, 2, U, V, rated, bitmap_ids, item_base, compact, order)
        assert r2["screened"], r2
        assert plan["cuts"] == cuts and plan["compact"] == (has_bm and compact == 1), plan
        assert np.array_equal(i2, i0), np.argwhere((i2 != i0).any(1))[:5]
        assert np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
        print("UNC %s / %s: %d of %d users uncertified" % (name, form, unc, U.shape[0]))
        if got is not None:
            assert np.array_equal(got[0].view(np.uint32), s2.view(np.uint32)) and np.array_equal(got[1], i2) and got[2] == unc
        got = (s2, i2, unc)
    _seen["%s / %s" % (name, form)] = got[2]
    return got[1]


_seen = {}                     # uncertified counts of the cases a test has run, asserted by _counts_as_stated when it is through


def _counts_as_stated():
    got = dict(_seen)
    _seen.clear()
    assert got and got == {key: UNCERTIFIED.get(key, 0) for key in got}


def _tables(rng, n_users, n_items, scale=0.1):
    return ((rng.standard_normal((n_users, 128)) * scale).astype(np.float32),
            (rng.standard_normal((n_items, 128)) * scale).astype(np.float32))


def _stream(rng, n_rows):
    """A table that streams exactly n_rows rows in every form: (n_items, cold ids).  A quarter more rows are masked by the bitmap;
    the forms without compaction stream those too, which the callers account for."""
    n_items = n_rows + n_rows // 4 + 3
    cold = np.sort(rng.choice(n_items, n_items - n_rows, replace=False))
    return n_items, cold


# ---- tile counts of the main range: the peeled body (0 .. 3: odd and even trips behind it), the ring's wrap (4, 5), the id slots
# (8, 9), a block of tile bits (64, 65), lockstep windows (127 .. 129, 257); a full last tile and last tiles of 1 and of 31 rows.
# 130 users: a full wave, a wave of two columns, two dead waves.
_counts = {}


def _count_case(tiles, last, compacted):
    key = (tiles, last, compacted)
    if key not in _counts:
        rng = np.random.default_rng(1000 + 40 * tiles + last)
        n_rows = 32 * (tiles - 1) + last if tiles else 0
        if compacted:                  # the compacted stream holds the unmasked rows only
            n_items, cold = _stream(rng, n_rows) if tiles else (40, np.arange(40))
        else:                          # every row is streamed, masked or not
            n_items, cold = n_rows, np.sort(rng.choice(n_rows, n_rows // 5, replace=False))
        U, V = _tables(rng, 130, n_items)
        _counts[key] = dict(U=U, V=V, cold=cold, rated=[np.unique(rng.integers(0, n_items, int(rng.integers(0, 12)))) for _ in range(130)])
    return _counts[key]


@pytest.mark.parametrize("tiles,last", [(t, l) for t in [0, 1, 2, 3, 4, 5, 8, 9, 64, 65, 127, 128, 129, 257] for l in [32, 1, 31]
                                        if t or l == 32])          # (an empty range has no last tile: once)
def test_tile_counts(monkeypatch, tiles, last):
    for form, (has_bm, compact, _) in FORMS.items():
        compacted = has_bm and compact == 1
        if tiles == 0 and not compacted:
            continue                   # an empty main range exists only where the bitmap masks every row of a compacted stream
        c = _count_case(tiles, last, compacted)
        n_stream = c["V"].shape[0] - (len(c["cold"]) if compacted else 0)
        assert (n_stream + 31) // 32 == tiles and (tiles == 0 or n_stream - 32 * (tiles - 1) == last)
        _check(monkeypatch, "tiles %d last %d%s" % (tiles, last, " c" if compacted else ""), form, c["U"], c["V"], cold=c["cold"],
               rated=c["rated"] if has_bm else None)
    _counts_as_stated()


# ---- where the hits fall.  9 tiles and a last one of 31 rows (319 streamed rows), 150 users (all columns of a full wave and 22 of
# the next).  Every user scores row r at about (1 + f(r)) |w|^2: the table is a ramp along one direction w that all users share.
#   first     the 20 best rows are rows 0 .. 19 of the stream: the first tile fills the lists, no later tile holds a candidate
#   last      ... are the last 20 rows: the hits of the last tile run in the epilogue body
#   rising    scores rise along the stream: every tile of every wave holds candidates, every body takes the event branch
#   falling   scores fall along the stream: as `first`, with every later row just below the thresholds of the rows before it
def _ramp_case(kind, compacted):
    key = ("ramp", kind, compacted)
    if key not in _counts:
        rng = np.random.default_rng(2000 + len(kind))
        n_rows = 9 * 32 + 31
        n_items, cold = _stream(rng, n_rows) if compacted else (n_rows, np.sort(rng.choice(n_rows, n_rows // 5, replace=False)))
        w = (rng.standard_normal(128) * 0.1).astype(np.float32)
        U = (w[None, :] * (1 + rng.random((150, 1)) * 0.25)).astype(np.float32)
        live = np.setdiff1d(np.arange(n_items), cold) if compacted else np.arange(n_items)
        pos = np.zeros(n_items)                     # position along the stream, 0 .. 1 (masked rows of a compacted stream: 0)
        pos[live] = np.arange(len(live)) / len(live)
        f = {"first": np.where(pos * len(live) < 20, 1.0 - pos, 0.2 * pos), "last": np.where(pos * len(live) >= len(live) - 20, pos, 0.2 * pos),
             "rising": pos, "falling": 1.0 - pos}[kind]
        V = ((1 + f)[:, None] * w[None, :]).astype(np.float32)
        _counts[key] = dict(U=U, V=V, cold=cold)
    return _counts[key]


@pytest.mark.parametrize("kind", ["first", "last", "rising", "falling"])
def test_where_the_hits_fall(monkeypatch, kind):
    for form, (has_bm, compact, order) in FORMS.items():
        compacted = has_bm and compact == 1
        c = _ramp_case(kind, compacted)
        got = _check(monkeypatch, "hits %s%s" % (kind, " c" if compacted else ""), form, c["U"], c["V"], cold=c["cold"])
        best = np.argsort(-(c["V"] @ c["U"][0]), kind="stable")
        best = best[~np.isin(best, c["cold"])][:K] if has_bm else best[:K]
        assert set(got[0]) == set(best)
    _counts_as_stated()


# ---- dead and partial waves: 5 tiles and a last one of 31 rows; a dead wave walks, synchronises and fetches as ever and inserts nothing
@pytest.mark.parametrize("n_users", [1, 15, 16, 17, 127, 128, 129, 511, 512, 513])
def test_dead_and_partial_waves(monkeypatch, n_users):
    for form, (has_bm, compact, _) in FORMS.items():
        compacted = has_bm and compact == 1
        key = ("waves", compacted)
        if key not in _counts:
            rng = np.random.default_rng(3000 + compacted)
            n_rows = 5 * 32 + 31
            n_items, cold = _stream(rng, n_rows) if compacted else (n_rows, np.sort(rng.choice(n_rows, n_rows // 5, replace=False)))
            U, V = _tables(rng, 513, n_items)
            _counts[key] = dict(U=U, V=V, cold=cold, rated=[np.unique(rng.integers(0, n_items, int(rng.integers(0, 12)))) for _ in range(513)])
        c = _counts[key]
        _check(monkeypatch, "waves %d%s" % (n_users, " c" if compacted else ""), form, c["U"][:n_users], c["V"], cold=c["cold"],
               rated=c["rated"][:n_users] if has_bm else None)
    _counts_as_stated()


# ---- seeded thresholds and cuts at an off-grid shard base.  65 765 items: a prefix of 8 192 seeds the lists, the main range of
# 57 573 rows is 1 800 tiles in 28 cuts of 64 or 65 tiles (odd and even counts; compacted: fewer rows, the same 28 cuts by the
# plan).  "below": every row of the main range scores below the prefix's 28th best for every user, so no body takes the event
# branch and the lists leave as they were seeded; "above": the best 20 rows lie in the main range, spread over the cuts.
@pytest.mark.parametrize("kind", ["below", "above"])
@pytest.mark.parametrize("form", ["compacted, ordered", "bitmap, not compacted", "no bitmap"])
def test_cuts_and_seeded_thresholds(monkeypatch, kind, form):
    key = ("cuts", kind)
    if key not in _counts:
        rng = np.random.default_rng(4000)
        n_users, n_items, base = 40, 65536 + 7 * 32 + 5, 1_000_003
        U, V = _tables(rng, n_users, n_items)
        w = (rng.standard_normal(128) * 0.1).astype(np.float32)
        U = (U * np.float32(0.05) + w[None, :]).astype(np.float32)
        strong = rng.choice(8192, 64, replace=False) if kind == "below" else 8192 + rng.choice(n_items - 8192, 64, replace=False)
        V[strong] = ((2 + np.arange(64) / 64.0)[:, None] * w[None, :]).astype(np.float32)
        cold = base + np.setdiff1d(np.where(rng.random(n_items) < 0.2)[0], strong[32:])
        _counts[key] = dict(U=U, V=V, cold=cold, base=base, strong=strong)
    c = _counts[key]
    n_main = c["V"].shape[0] - 8192
    tiles = [(n_main + 31) // 32 * (s + 1) // 28 - (n_main + 31) // 32 * s // 28 for s in range(28)]
    assert set(tiles) == {64, 65} and sum(tiles) == 1800
    got = _check(monkeypatch, "cuts %s" % kind, form, c["U"], c["V"], cold=c["cold"], item_base=c["base"], cuts=28)
    assert np.isin(got - c["base"], c["strong"]).all()
    _counts_as_stated()
