"""The 16x16x32 MFMA form of the screened route's fp16 pass (run with -m gpu on an MI355X).

The screen's kernel (score_topk_dma_kernel, fp16 d=128) holds its users in blocks of 16 columns and a tile's 32 rows as two
16-row halves of four 4-row groups.  A mistake in that layout does not corrupt the call's output -- the exact rescoring and the
certificate see to that -- it only leaves users uncertified, who then get the right answer slowly from the fallback.  So every
case asserts three things: the screened call (CRH_SCORE_SCREEN=2) equals the exact route (CRH_SCORE_SCREEN=0) bit for bit and
for every user, sampled users equal the C oracle, and the number of uncertified users is what the case states.  The helpers
follow tests/test_score_screen_gpu.py; the exact route's answer of a case is computed once and shared."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

K = 20
PAD = np.iinfo(np.int32).max


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _tables(rng, n_users, n_items, d=128, scale=0.1):
    return ((rng.standard_normal((n_users, d)) * scale).astype(np.float32),
            (rng.standard_normal((n_items, d)) * scale).astype(np.float32))


def _rated(rng, n_users, lo, hi, max_len=40):
    return [np.unique(rng.integers(lo, hi, int(rng.integers(0, max_len)))) for _ in range(n_users)]


def _run(monkeypatch, mode, U, V, k, rated=None, bitmap_ids=None, item_base=0, compact=1, order=1):
    dev = _dev()
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    monkeypatch.setenv("CRH_SCORE_SCREEN_COMPACT", str(compact))
    monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", str(order))
    rp, rc = ops.rated_csr(rated, dev) if rated is not None else (None, None)
    bm = ops.make_bitmap(item_base + V.shape[0], bitmap_ids, dev) if bitmap_ids is not None else None
    route = ops.score_topk_route(U.shape[0], V.shape[0], V.shape[1], k, has_bitmap=bm is not None)
    plan = ops.score_topk_screen_plan(U.shape[0], V.shape[0], V.shape[1], k, has_bitmap=bm is not None) if route["screened"] else None
    s, i = ops.score_topk(torch.from_numpy(U).to(dev), None, torch.from_numpy(V).to(dev), k, rp, rc, bm, item_base=item_base)
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if route["screened"] else None
    return s.cpu().numpy(), i.cpu().numpy(), route, plan, unc


_exact_cache = {}


def _exact(monkeypatch, name, U, V, k, rated, bitmap_ids, item_base, n_sample=12):
    """The exact route's answer of a case (cached under `name`), checked against the oracle on sampled users when first computed."""
    if name not in _exact_cache:
        s0, i0, r0, _, _ = _run(monkeypatch, 0, U, V, k, rated, bitmap_ids, item_base)
        assert not r0["screened"]
        pick = np.unique(np.random.default_rng(0).integers(0, U.shape[0], n_sample))
        rowptr = col = None
        if rated is not None:
            rr = [rated[j] for j in pick]
            rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
            col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
        bm = orc.make_bitmap(item_base + V.shape[0], bitmap_ids) if bitmap_ids is not None else None
        ws, wi = orc.score_topk(U, pick.astype(np.int64), V, k, rowptr, col, bm, item_base=item_base)
        assert np.array_equal(i0[pick], wi)
        assert np.array_equal(s0[pick].view(np.uint32), ws.view(np.uint32))
        s0.setflags(write=False)
        i0.setflags(write=False)
        _exact_cache[name] = (s0, i0)
    return _exact_cache[name]


def _check(monkeypatch, name, U, V, k=K, rated=None, bitmap_ids=None, item_base=0, compact=1, order=1, n_sample=12):
    """Screened == exact for every user (and the exact answer == oracle on sampled users); returns (uncertified, plan, ids)."""
    s0, i0 = _exact(monkeypatch, name, U, V, k, rated, bitmap_ids, item_base, n_sample)
    s2, i2, r2, plan, unc = _run(monkeypatch, 2, U, V, k, rated, bitmap_ids, item_base, compact, order)
    assert r2["screened"], r2
    assert plan["compact"] == (bitmap_ids is not None and compact == 1), plan
    assert np.array_equal(i2, i0), np.argwhere((i2 != i0).any(1))[:5]
    assert np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
    print("%s (compact %d, order %d): %d of %d users uncertified" % (name, compact, order, unc, U.shape[0]))
    return unc, plan, i2


# ---- case 1: ragged edges.  1 037 users (no multiple of 16 or 128: a last wave of 13 columns and dead waves behind it), 5 003 items
# (a last tile of 11 rows, no seeded prefix)
_ragged = {}


def _ragged_case():
    if not _ragged:
        rng = np.random.default_rng(111)
        U, V = _tables(rng, 1037, 5003)
        _ragged.update(U=U, V=V, rated=_rated(rng, 1037, 0, 5003), cold=np.where(rng.random(5003) < 0.2)[0])
    return _ragged


@pytest.mark.parametrize("way", ["no-masks", "bitmap+rated", "bitmap+rated, not compacted"])
def test_ragged_edges(monkeypatch, way):
    c = _ragged_case()
    if way == "no-masks":
        unc, _, _ = _check(monkeypatch, "ragged/none", c["U"], c["V"])
    else:
        unc, _, _ = _check(monkeypatch, "ragged/masks", c["U"], c["V"], rated=c["rated"], bitmap_ids=c["cold"],
                           compact=0 if "not" in way else 1)
    assert unc == 0          # gaussian tables: the K' = 28 margin certifies every user


# ---- case 2: planted winners.  Each of 150 users owns 20 items that hold 2 U[u] / |U[u]| (score 2 |U[u]| ~ 2.3 against a background of
# |score| < 0.3 and < 1 for another user's plants): its top 20 are exactly those.  The planted ids cover every row of a tile (both
# 16-row halves, all four 4-row groups), the whole first tile and the whole ragged last tile; the users are all columns of the
# first wave (0, 15, 16, 31, 127) and 128 .. 149 of the second.
# Under a mask a user keeps 18 of its plants, and its ranks 19 .. 28 go to the plants of the user closest to it.  Twenty IDENTICAL
# rows there are exact ties across ranks 20 and 28, which no certificate can pass (every user is uncertified, on the 32x32 form as
# well: 150 of 150 measured).  So the masked variants grade the plants: copy j holds (2 + j / 100) U[u] / |U[u]|, which puts
# ~0.01 * 0.5 between neighbouring ranks of a foreign group, 8 ranks = 0.04 between the 20th and the 28th score, against a bound
# B_u of about 1e-3 (|u| ~ 1.1, fp16 residual and 2^-12 of rows of norm 2).
_planted = {}


def _planted_case(graded=False):
    if graded not in _planted:
        rng = np.random.default_rng(222)
        n_users, n_items = 150, 5003
        U, V = _tables(rng, n_users, n_items)
        V *= np.float32(0.25)
        last0 = (n_items // 32) * 32
        pool = np.concatenate([np.arange(32), np.arange(last0, n_items),
                               rng.choice(np.arange(32, last0), n_users * K - 32 - (n_items - last0), replace=False)])
        ids = rng.permutation(pool).reshape(n_users, K)
        for u in range(n_users):
            V[ids[u]] = U[u] / np.linalg.norm(U[u]) * np.float32(2.0)
            if graded:
                V[ids[u]] *= (1 + np.arange(K, dtype=np.float32) / 200)[:, None]
        assert len(np.unique(ids)) == n_users * K
        assert set(ids.ravel() % 32) == set(range(32))                                   # every row of a tile: both halves, all g
        assert set(range(32)) <= set(ids.ravel()) and set(range(last0, n_items)) <= set(ids.ravel())   # first and last tile, whole
        _planted[graded] = dict(U=U, V=V, ids=ids)
    return _planted[graded]


def test_planted_winners_no_masks(monkeypatch):
    c = _planted_case()
    unc, _, got = _check(monkeypatch, "planted/none", c["U"], c["V"])
    assert np.array_equal(np.sort(got, axis=1), np.sort(c["ids"], axis=1))
    assert unc == 0


@pytest.mark.parametrize("compact,order", [(1, 1), (1, 0), (0, 0)])
def test_planted_winners_bitmap(monkeypatch, compact, order):
    """Two planted ids of every user are masked by the bitmap (with 20 % of the background): they drop out, the other 18 stay."""
    c = _planted_case(graded=True)
    ids = c["ids"]
    rng = np.random.default_rng(223)
    cold = np.union1d(np.setdiff1d(np.where(rng.random(c["V"].shape[0]) < 0.2)[0], ids.ravel()), ids[:, [3, 11]].ravel())
    if compact and not order:        # rows of the compacted stream in ascending id order: the plants still cover every row of a tile
        live = np.setdiff1d(np.arange(c["V"].shape[0]), cold)
        assert set(np.searchsorted(live, np.delete(ids, [3, 11], axis=1).ravel()) % 32) == set(range(32))
    unc, _, got = _check(monkeypatch, "planted/bitmap", c["U"], c["V"], bitmap_ids=cold, compact=compact, order=order)
    for u in range(ids.shape[0]):
        assert not np.isin(ids[u, [3, 11]], got[u]).any()
        assert np.isin(np.delete(ids[u], [3, 11]), got[u]).all()
    assert unc == 0


def test_planted_winners_rated(monkeypatch):
    """Two planted ids of every user are in that user's rated list (and ten random ones): they drop out for that user."""
    c = _planted_case(graded=True)
    ids = c["ids"]
    rng = np.random.default_rng(224)
    rated = [np.unique(np.concatenate([ids[u, [5, 17]], rng.integers(0, c["V"].shape[0], 10)])) for u in range(ids.shape[0])]
    unc, _, got = _check(monkeypatch, "planted/rated", c["U"], c["V"], rated=rated)
    for u in range(ids.shape[0]):
        kept = np.setdiff1d(ids[u], rated[u])
        assert 10 <= len(kept) <= 18
        assert not np.isin(ids[u, [5, 17]], got[u]).any() and np.isin(kept, got[u]).all()
    assert unc == 0


# ---- case 3: lists that do not fill.  48 items, every third masked, rated lists: thresholds stay -inf, masked rows are candidates
# of the non-compacted form (they enter at -1e9); 13 items: fewer than k
@pytest.mark.parametrize("n_items", [48, 13])
def test_lists_that_do_not_fill(monkeypatch, n_items):
    rng = np.random.default_rng(333)
    U, V = _tables(rng, 700, n_items)
    rated = _rated(rng, 700, 0, n_items)
    cold = np.arange(0, n_items, 3)
    unc = [_check(monkeypatch, "short/%d" % n_items, U, V, rated=rated, bitmap_ids=cold, compact=cp)[0] for cp in (1, 0)]
    s0, i0 = _exact_cache["short/%d" % n_items]
    assert (i0 == PAD).any() or (s0 == -1e9).any()      # the lists really did not fill
    assert unc[0] == unc[1]          # one approximate score in both forms: the same users are certified


# ---- case 4: cuts.  Few users: the screen cuts the item range (at tile bounds of an off-grid shard base) and merges the cuts' lists
@pytest.mark.parametrize("masks", [False, True])
def test_cuts_off_grid_base(monkeypatch, masks):
    rng = np.random.default_rng(444)
    n_users, n_items, base = 40, 300_000, 1_000_003
    U, V = _tables(rng, n_users, n_items)
    rated = _rated(rng, n_users, base - 50, base + n_items + 50) if masks else None
    cold = base + np.where(rng.random(n_items) < 0.2)[0] if masks else None
    assert ops.score_topk_screen_plan(n_users, n_items, 128, K, has_bitmap=masks)["cuts"] > 1
    unc, plan, _ = _check(monkeypatch, "cuts/%d" % masks, U, V, rated=rated, bitmap_ids=cold, item_base=base, n_sample=6)
    assert plan["cuts"] > 1
    assert unc == 0


# ---- case 5: k = 1 on case 1's tables
@pytest.mark.parametrize("masks", [False, True])
def test_k1(monkeypatch, masks):
    c = _ragged_case()
    unc, _, _ = _check(monkeypatch, "ragged-k1/%d" % masks, c["U"], c["V"], k=1, rated=c["rated"] if masks else None,
                       bitmap_ids=c["cold"] if masks else None)
    assert unc == 0


# ---- case 6: one approximate score everywhere -- the same users are certified whatever the screen's switches
def test_equal_counts_across_switches(monkeypatch):
    c = _ragged_case()
    unc = {(cp, od): _check(monkeypatch, "ragged/masks", c["U"], c["V"], rated=c["rated"], bitmap_ids=c["cold"], compact=cp, order=od)[0]
           for cp in (1, 0) for od in (1, 0)}
    assert len(set(unc.values())) == 1, unc
