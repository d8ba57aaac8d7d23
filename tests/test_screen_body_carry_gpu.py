"""The carried fetch state and the straightened trip of the screen pass's 16x16 tile body (run with -m gpu on an MI355X).

Round 22 changed how body16 of the COMPACTED score_topk_dma_kernel works out what it fetches: the global address of tile j + 3 and
of its ids is a scalar base carried from tile to tile plus a 32-bit lane offset, the id slot and the ring slot are carried LDS
offsets, the end-of-stream clamp is a scalar compare per tile, and the lane clamp of the last tile's ids is worked out two bodies
ahead; the tests of the two bounds of a trip moved into the bodies and the events out of the loop's common path.  In BOTH 16x16
kernels the maxima's dependent pair became one asm statement and the counted fragment waits name no register any more, so only
sched_barrier keeps a group's MFMAs behind its wait: that is all the uncompacted cases below cover (that kernel still recomputes
its fetch from the tile counter).  None of that may change a bit of a result.  As in tests/test_screen_body_gpu.py (whose helpers these follow) a mistake
does not corrupt the call's output -- the exact rescoring and the certificate see to that -- it leaves users uncertified.  So
every case asserts that the plan is the one it was built for, runs the screened call (CRH_SCORE_SCREEN=2) twice for equal bits,
compares it with the exact route (CRH_SCORE_SCREEN=0) bit for bit for every user, compares sampled users with the C oracle, and
asserts that the number of uncertified users is the constant recorded from the library of the commit before the change on the
same inputs (UNCERTIFIED below; 0 where a case is not listed).

Shapes (130 users unless stated: a full wave, a wave of two columns, two dead waves; d = 128, k = 20).
  * stream tile counts 1 .. 17 -- the ring's period 4, the id slots' period 8, both parities of the trip, and the look-ahead
    tiles 1 .. 3 beyond the stream's end, where the carried bases stop moving -- with a last tile of 1 row and of 32 rows, in the
    compacted and the uncompacted form (below 65 536 items: no prefix, one cut, the stream is the whole table);
  * a compacted stream of about 1 100 tiles with rated lists: the second and third block of rated-tile flags are fetched by the
    trip head's rare path;
  * 4 608 users over about 300 tiles: nine workgroups, so the lockstep window (128 tiles) is armed and crossed twice.  The plan
    does not report the window: the case relies on the route's rule (one cut, more than eight and at most 256 workgroups,
    CRH_SCORE_SYNC_WINDOW unset) and asserts only the cut;
  * 65 765 items: a prefix of 8 192 seeds the lists, 28 cuts of 64 or 65 tiles start at t0 > 0."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

K = 20
FORMS = {                      # name: (bitmap, CRH_SCORE_SCREEN_COMPACT, CRH_SCORE_SCREEN_ORDER)
    "compacted": (True, 1, 1),
    "uncompacted": (True, 0, 0),
}
# uncertified users per case where it is not 0 (from the parent commit's library on the same inputs: tables with fewer live rows
# than the screen's K' = 28 or little more, where the certificate has no margin to stand on)
UNCERTIFIED = {
    "tiles 1 last 1 compacted / compacted": 130, "tiles 1 last 1 uncompacted / uncompacted": 130,
    "tiles 1 last 32 compacted / compacted": 58, "tiles 1 last 32 uncompacted / uncompacted": 130,
    "tiles 2 last 1 compacted / compacted": 42, "tiles 2 last 1 uncompacted / uncompacted": 130,
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
    bm = ops.make_bitmap(item_base + V.shape[0], bitmap_ids, dev)
    route = ops.score_topk_route(U.shape[0], V.shape[0], V.shape[1], K, has_bitmap=True)
    plan = None
    if route["screened"]:
        plan = ops.score_topk_screen_plan(U.shape[0], V.shape[0], V.shape[1], K, has_bitmap=True)
        plan["rated_tiles"] = ops.score_topk_screen_rated_tiles(U.shape[0], V.shape[0], V.shape[1], K, has_bitmap=True, has_rated=rated is not None)
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
        bm = orc.make_bitmap(item_base + V.shape[0], bitmap_ids)
        ws, wi = orc.score_topk(U, pick.astype(np.int64), V, K, rowptr, col, bm, item_base=item_base)
        assert np.array_equal(i0[pick], wi)
        assert np.array_equal(s0[pick].view(np.uint32), ws.view(np.uint32))
        s0.setflags(write=False)
        i0.setflags(write=False)
        _exact_cache[name] = (s0, i0)
    return _exact_cache[name]


_seen = {}                     # uncertified counts of the cases a test has run, asserted by _counts_as_stated when it is through


def _check(monkeypatch, name, form, U, V, cold, rated=None, item_base=0, n_sample=4, cuts=1, rated_tiles=None):
    """One case in one stream form: the plan is the one the case was built for; screened == exact for every user, twice; the
    uncertified count is noted for _counts_as_stated.  Returns the screened ids."""
    _, compact, order = FORMS[form]
    s0, i0 = _exact(monkeypatch, name, U, V, rated, cold, item_base, n_sample)
    got = None
    for rep in range(2):
        s2, i2, r2, plan, unc = _run(monkeypatch, 2, U, V, rated, cold, item_base, compact, order)
        assert r2["screened"], r2
        assert plan["cuts"] == cuts and plan["compact"] == (compact == 1), plan
        if rated_tiles is not None:
            assert plan["rated_tiles"] == rated_tiles, plan
        assert np.array_equal(i2, i0), np.argwhere((i2 != i0).any(1))[:5]
        assert np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
        print("UNC %s / %s: %d of %d users uncertified" % (name, form, unc, U.shape[0]))
        if got is not None:
            assert np.array_equal(got[0].view(np.uint32), s2.view(np.uint32)) and np.array_equal(got[1], i2) and got[2] == unc
        got = (s2, i2, unc)
    _seen["%s / %s" % (name, form)] = got[2]
    return got[1]


def _counts_as_stated():
    got = dict(_seen)
    _seen.clear()
    assert got and got == {key: UNCERTIFIED.get(key, 0) for key in got}


def _tables(rng, n_users, n_items, scale=0.1):
    return ((rng.standard_normal((n_users, 128)) * scale).astype(np.float32),
            (rng.standard_normal((n_items, 128)) * scale).astype(np.float32))


def _stream(rng, n_rows, compacted):
    """A table that streams exactly n_rows rows: (n_items, cold ids).  Compacted: a quarter more rows are masked by the bitmap and
    left out of the stream; uncompacted: every row is streamed, a fifth of them masked."""
    if compacted:
        n_items = n_rows + n_rows // 4 + 3
        return n_items, np.sort(rng.choice(n_items, n_items - n_rows, replace=False))
    return n_rows, np.sort(rng.choice(n_rows, n_rows // 5, replace=False))


def _rated(rng, n_users, n_items, most=12):
    return [np.unique(rng.integers(0, n_items, int(rng.integers(0, most)))) for _ in range(n_users)]


# ---- tile counts of the stream
@pytest.mark.parametrize("last", [1, 32])
@pytest.mark.parametrize("tiles", [1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17])
def test_tile_counts(monkeypatch, tiles, last):
    for form, (_, compact, _) in FORMS.items():
        compacted = compact == 1
        rng = np.random.default_rng(2200 + 40 * tiles + last + (1000 if compacted else 0))
        n_rows = 32 * (tiles - 1) + last
        n_items, cold = _stream(rng, n_rows, compacted)
        U, V = _tables(rng, 130, n_items)
        n_stream = n_items - (len(cold) if compacted else 0)
        assert (n_stream + 31) // 32 == tiles and n_stream - 32 * (tiles - 1) == last
        _check(monkeypatch, "tiles %d last %d %s" % (tiles, last, form), form, U, V, cold, rated=_rated(rng, 130, n_items))
    _counts_as_stated()


# ---- the trip head's rare path fetching blocks of rated-tile flags: 1 100 tiles are three blocks of 512 tiles' flags; blocks 0 and
# 1 come with the prologue, block 2 is asked for 64 tiles into block 1.  Every user rated up to 40 items, so most tiles carry a flag.
def test_rated_tile_blocks(monkeypatch):
    rng = np.random.default_rng(2301)
    n_rows = 1100 * 32 - 9
    n_items, cold = _stream(rng, n_rows, True)
    assert n_items < 65536
    U, V = _tables(rng, 130, n_items)
    rated = _rated(rng, 130, n_items, most=40)
    got = _check(monkeypatch, "rated blocks", "compacted", U, V, cold, rated=rated, rated_tiles=True)
    for u in (0, 64, 129):
        assert not np.isin(got[u], rated[u]).any() and not np.isin(got[u], cold).any()
    _counts_as_stated()


# ---- nine workgroups: the lockstep window of 128 tiles is armed (more than eight workgroups, one cut) and crossed at tiles 128 and
# 256 of 300; wave 0 of every workgroup takes the trip head's rare path there
@pytest.mark.parametrize("form", list(FORMS))
def test_lockstep_window(monkeypatch, form):
    compacted = FORMS[form][1] == 1
    rng = np.random.default_rng(2302 + compacted)
    n_rows = 300 * 32 - 5
    n_items, cold = _stream(rng, n_rows, compacted)
    U, V = _tables(rng, 4608, n_items)
    _check(monkeypatch, "window %s" % form, form, U, V, cold, rated=_rated(rng, 4608, n_items, most=6), n_sample=6)
    _counts_as_stated()


# ---- 65 765 items at an off-grid shard base: a prefix of 8 192 seeds the lists, the main range of 57 573 rows is 1 800 tiles in 28
# cuts of 64 or 65 tiles (compacted: fewer rows, the same 28 cuts by the plan), each starting at its own t0 with its own clamp
@pytest.mark.parametrize("form", list(FORMS))
def test_cuts(monkeypatch, form):
    rng = np.random.default_rng(2304)
    n_users, n_items, base = 130, 65536 + 7 * 32 + 5, 1_000_003
    U, V = _tables(rng, n_users, n_items)
    w = (rng.standard_normal(128) * 0.1).astype(np.float32)
    U = (U * np.float32(0.05) + w[None, :]).astype(np.float32)
    strong = 8192 + rng.choice(n_items - 8192, 64, replace=False)
    V[strong] = ((2 + np.arange(64) / 64.0)[:, None] * w[None, :]).astype(np.float32)
    cold = base + np.setdiff1d(np.where(rng.random(n_items) < 0.2)[0], strong[32:])
    n_main = n_items - 8192
    tiles = [(n_main + 31) // 32 * (s + 1) // 28 - (n_main + 31) // 32 * s // 28 for s in range(28)]
    assert set(tiles) == {64, 65} and sum(tiles) == 1800
    got = _check(monkeypatch, "cuts", form, U, V, cold, item_base=base, cuts=28)
    assert np.isin(got - base, strong).all()
    _counts_as_stated()
