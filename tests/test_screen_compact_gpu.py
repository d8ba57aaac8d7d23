"""The screened route's fp16 pass over the unmasked rows only (run with -m gpu on an MI355X).

Under a candidate bitmap stage 0 builds a live-row map of the shard's main range, packs only those rows, and the fp16 kernel walks
the compacted stream and takes a candidate's id from the map (CRH_SCORE_SCREEN_COMPACT=1, the default).  Every case runs
CRH_SCORE_SCREEN=2 with the compaction on and asserts (a) scores and ids equal the exact route's (CRH_SCORE_SCREEN=0) bit for bit
for every user, (b) they equal the C oracle on sampled users, (c) the uncertified-user count equals that of the same call with
CRH_SCORE_SCREEN_COMPACT=0: the candidate lists of every certifiable user are identical by construction."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

K = 20
KP = 28          # candidates per user of the screen
PREFIX = 8192    # seed prefix of shards of >= 65 536 items (ranked uncompacted)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _tables(rng, n_users, n_items, d=128, scale=0.1):
    return ((rng.standard_normal((n_users, d)) * scale).astype(np.float32),
            (rng.standard_normal((n_items, d)) * scale).astype(np.float32))


def _rated(rng, n_users, lo, hi, max_len=40):
    return [np.unique(rng.integers(lo, hi, int(rng.integers(0, max_len)))) for _ in range(n_users)]


def _bitmap(n_global, ids, dev):
    """As ops.make_bitmap, but an empty id list still gives a bitmap (nothing masked) and not None."""
    words = np.zeros((n_global + 31) // 32 + 1, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.int64)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).to(dev)


def _run(monkeypatch, mode, compact, U, users, V, k, rated, bitmap_ids, n_global, item_base):
    dev = _dev()
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    monkeypatch.setenv("CRH_SCORE_SCREEN_COMPACT", str(compact))
    rp, rc = ops.rated_csr(rated, dev) if rated is not None else (None, None)
    bm = _bitmap(n_global, bitmap_ids, dev) if bitmap_ids is not None else None
    tu = torch.from_numpy(users).to(dev) if users is not None else None
    n_users = U.shape[0] if users is None else len(users)
    route = ops.score_topk_route(n_users, V.shape[0], V.shape[1], k, has_bitmap=bm is not None)
    plan = ops.score_topk_screen_plan(n_users, V.shape[0], V.shape[1], k, has_bitmap=bm is not None)
    s, i = ops.score_topk(torch.from_numpy(U).to(dev), tu, torch.from_numpy(V).to(dev), k, rp, rc, bm, item_base=item_base)
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if route["screened"] else None
    return s.cpu().numpy(), i.cpu().numpy(), route, plan, unc


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _check(monkeypatch, U, V, k=K, users=None, rated=None, bitmap_ids=None, item_base=0, n_global=None, n_sample=12, seed=0,
           mode=2, min_cuts=1):
    """(a), (b), (c) of the module's docstring; returns the uncertified count and the exact route's answer."""
    n_global = item_base + V.shape[0] if n_global is None else n_global
    args = (U, users, V, k, rated, bitmap_ids, n_global, item_base)
    s0, i0, r0, _, _ = _run(monkeypatch, 0, 1, *args)
    assert not r0["screened"]
    s1, i1, r1, p1, unc1 = _run(monkeypatch, mode, 1, *args)
    assert r1["screened"], r1
    assert p1["compact"] == (bitmap_ids is not None), p1
    assert p1["cuts"] >= min_cuts, p1
    assert np.array_equal(i1, i0), np.argwhere((i1 != i0).any(1))[:5]
    assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32))
    rng = np.random.default_rng(seed)
    n = s0.shape[0]
    pick = np.unique(rng.integers(0, n, n_sample))
    urows = pick if users is None else users[pick]
    rowptr = col = None
    if rated is not None:
        rr = [rated[j] for j in pick]
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
        col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
    bm = orc.make_bitmap(n_global, bitmap_ids) if bitmap_ids is not None and len(bitmap_ids) else None
    ws, wi = orc.score_topk(U, urows.astype(np.int64), V, k, rowptr, col, bm, item_base=item_base)
    assert np.array_equal(i1[pick], wi)
    assert np.array_equal(s1[pick].view(np.uint32), ws.view(np.uint32))
    s2, i2, r2, p2, unc2 = _run(monkeypatch, mode, 0, *args)
    assert r2["screened"] and not p2["compact"]
    assert _same((s2, i2), (s0, i0))
    print("uncertified users: compacted %d, uncompacted %d of %d" % (unc1, unc2, n))
    assert unc1 == unc2
    return unc1, (s0, i0)


@pytest.mark.parametrize("share", [0.0, 0.2, 0.8])
def test_compact_prefix_and_masked_share(monkeypatch, share):
    rng = np.random.default_rng(21)
    n_users, n_items = 1000, 70_001
    U, V = _tables(rng, n_users, n_items)
    cold = np.where(rng.random(n_items) < share)[0]
    rated = _rated(rng, n_users, 0, n_items)           # uniform ids: every list of some length holds live and cold ones
    if share > 0:
        is_cold = np.zeros(n_items, bool)
        is_cold[cold] = True
        assert sum(1 for r in rated if len(r) and is_cold[r].any() and not is_cold[r].all()) > n_users // 2
    unc, _ = _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold)
    assert unc == 0          # gaussian tables: the K' = 28 margin certifies every user


def test_compact_off_grid_shard_base(monkeypatch):
    """A shard at a base that is no multiple of 32 under a GLOBAL bitmap whose bits outside the shard are clear (a map that
    counted them would shift every id), 300 users (no multiple of 128), rated ids on both sides of the shard."""
    rng = np.random.default_rng(22)
    n_items, base = 70_001, 1_000_003
    n_global = base + n_items + 5000
    U, V = _tables(rng, 300, n_items)
    assert (base + PREFIX) % 32 != 0 and (base + n_items) % 32 != 0
    cold = base + np.where(rng.random(n_items) < 0.2)[0]
    rated = _rated(rng, 300, base - 50, base + n_items + 50)
    unc, _ = _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold, item_base=base, n_global=n_global)
    assert unc == 0


def _structured_mask(rng, n_items, kind):
    """Masks over a 70 001-item shard; `kind` shapes the main range [PREFIX, n_items)."""
    cold = rng.random(n_items) < 0.2
    main = np.arange(PREFIX, n_items)
    if kind == "runs":                        # whole tiles of the uncompacted stream vanish, wherever they start
        for start in (PREFIX, PREFIX + 1000, 20_011, 40_000, n_items - 200):
            cold[start:start + int(rng.integers(64, 200))] = True
    elif kind in ("mult32", "mult32p1"):       # live rows of the main range: 32 m, 32 m + 1
        want = 0 if kind == "mult32" else 1
        live = main[~cold[main]]
        cold[live[:(len(live) - want) % 32]] = True
        assert (~cold[main]).sum() % 32 == want
    elif kind == "ends_masked":
        cold[[PREFIX, n_items - 1]] = True
    elif kind == "ends_live":
        cold[[PREFIX, n_items - 1]] = False
        cold[[PREFIX + 1, n_items - 2]] = True
    return np.where(cold)[0]


@pytest.mark.parametrize("kind", ["runs", "mult32", "mult32p1", "ends_masked", "ends_live"])
def test_compact_structured_masks(monkeypatch, kind):
    rng = np.random.default_rng(23)
    n_users, n_items = 300, 70_001
    U, V = _tables(rng, n_users, n_items)
    # the items at the ends of the main range score high for everybody: they are in the answer when live (and not rated)
    U[:, 0] = 1.0
    V[[PREFIX, n_items - 1]] = 0.0
    V[[PREFIX, n_items - 1], 0] = 5.0
    cold = _structured_mask(rng, n_items, kind)
    rated = _rated(rng, n_users, 0, n_items)
    _, (s0, i0) = _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold)
    if kind in ("ends_masked", "ends_live"):
        found = np.isin(i0, [PREFIX, n_items - 1]).any(1).mean()
        assert (found == 0.0) if kind == "ends_masked" else (found > 0.5)


@pytest.mark.parametrize("kind", ["few_main", "few_shard", "none_main"])
def test_compact_nearly_everything_masked(monkeypatch, kind):
    """The answers come from the seeds and the fallback: -1e9 entries and padding as the exact route writes them."""
    rng = np.random.default_rng(24)
    n_users, n_items = 300, 70_001
    U, V = _tables(rng, n_users, n_items)
    cold = np.zeros(n_items, bool)
    cold[PREFIX:] = True                                # the main range entirely masked
    cold[:PREFIX] = rng.random(PREFIX) < 0.2
    if kind == "few_main":
        cold[rng.choice(np.arange(PREFIX, n_items), KP - 5, replace=False)] = False
    elif kind == "few_shard":
        cold[:PREFIX] = True
        cold[rng.choice(PREFIX, 5, replace=False)] = False
        cold[rng.choice(np.arange(PREFIX, n_items), 7, replace=False)] = False
        assert (~cold).sum() < K
    rated = _rated(rng, n_users, 0, n_items)
    live = np.where(~cold)[0]
    for j in range(0, n_users, 3):                      # and rated lists that hit the few live items
        rated[j] = np.unique(np.concatenate([rated[j], rng.choice(live, 3)]))
    unc, (s0, i0) = _check(monkeypatch, U, V, rated=rated, bitmap_ids=np.where(cold)[0])
    if kind == "few_shard":
        assert unc == n_users
        assert (s0 == -1e9).any() or (i0 == np.iinfo(np.int32).max).any() or (s0 == -np.inf).any()


@pytest.mark.parametrize("n_items", [5000, 48])
def test_compact_no_prefix(monkeypatch, n_items):
    rng = np.random.default_rng(25)
    U, V = _tables(rng, 700, n_items)
    rated = _rated(rng, 700, 0, n_items)
    _check(monkeypatch, U, V, rated=rated, bitmap_ids=np.arange(0, n_items, 3))


def test_compact_cuts(monkeypatch):
    """Few users: the fp16 pass cuts the item range; the cuts' id bounds come from the map, and the cuts are merged."""
    rng = np.random.default_rng(26)
    n_users, n_items = 130, 300_000
    U, V = _tables(rng, n_users, n_items)
    rated = _rated(rng, n_users, 0, n_items)
    cold = np.where(rng.random(n_items) < 0.2)[0]
    assert ops.score_topk_screen_plan(n_users, n_items, 128, K)["cuts"] > 1
    unc, _ = _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold, min_cuts=2)
    assert unc == 0


def test_compact_k1_and_user_index(monkeypatch):
    rng = np.random.default_rng(27)
    n_rows, n_items = 2000, 70_001
    U, V = _tables(rng, n_rows, n_items)
    users = rng.integers(0, n_rows, 500).astype(np.int32)
    users[:4] = users[4]                                # repeated rows
    rated = _rated(rng, 500, 0, n_items)
    cold = np.where(rng.random(n_items) < 0.2)[0]
    _check(monkeypatch, U, V, k=1, users=users, rated=rated, bitmap_ids=cold)
    _check(monkeypatch, U, V, users=users, rated=rated, bitmap_ids=cold)


def test_compact_no_user_certified(monkeypatch):
    """CRH_SCORE_SCREEN=3: every user goes through the exact fallback."""
    rng = np.random.default_rng(28)
    n_users, n_items = 200, 70_001
    U, V = _tables(rng, n_users, n_items)
    rated = _rated(rng, n_users, 0, n_items)
    unc, _ = _check(monkeypatch, U, V, rated=rated, bitmap_ids=np.where(rng.random(n_items) < 0.2)[0], mode=3)
    assert unc == n_users


def test_compact_switch_without_bitmap(monkeypatch):
    """No candidate bitmap: the switch changes nothing."""
    rng = np.random.default_rng(29)
    U, V = _tables(rng, 500, 70_001)
    rated = _rated(rng, 500, 0, 70_001)
    unc, _ = _check(monkeypatch, U, V, rated=rated, bitmap_ids=None)
    assert unc == 0
