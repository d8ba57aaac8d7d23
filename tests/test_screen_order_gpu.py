"""The screened route's fp16 pass in descending item-norm order (run with -m gpu on an MI355X).

Under a candidate bitmap, when the fp16 pass is one cut, stage 0 sorts the live-row map of the main range stably by a 16-bit norm
key (CRH_SCORE_SCREEN_ORDER=1, the default) and the pass streams the rows in that order.  A streaming top-K' under the canonical
key does not depend on the order of arrival, so every case runs CRH_SCORE_SCREEN=2 (or 3) and asserts that scores and ids with the
order on equal (a) the exact route's (CRH_SCORE_SCREEN=0) and (b) those of CRH_SCORE_SCREEN_ORDER=0, bit for bit, and (c) that
crh_score_topk_uncertified gives the same count with the order on and off.  The map itself is checked through its test entry
point: a wrong order only costs speed, a map that is not a permutation loses an id that is rarely a winner.

Shapes.  The order applies to a pass of one cut.  A shard with a seed prefix (>= 65 536 items) is cut whenever its users do not
fill the chip's 256 workgroups of 512, so the 70 001-item cases (prefix, ragged last tile) run 130 700 users: 256 workgroups, the
last one with a full wave, a wave of 12 users and two empty ones.  The 5 000-item cases (no prefix) are one cut at any user
count and run 300 users (three waves, the last one partly empty).  300 users x 70 001 items is 30 cuts: see
test_order_not_with_cuts."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops

pytestmark = pytest.mark.gpu

K = 20
PREFIX = 8192        # seed prefix of shards of >= 65 536 items (ranked unordered and uncompacted)
SIZES = [70_001, 5_000]     # with a prefix and a ragged last tile / without a prefix
USERS = {70_001: 130_700, 5_000: 300}      # (see the module's docstring)


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _tables(rng, n_items, kind="gauss", n_users=None, d=128, scale=0.1):
    n_users = USERS[n_items] if n_users is None else n_users
    U = (rng.standard_normal((n_users, d), dtype=np.float32) * np.float32(scale))
    V = (rng.standard_normal((n_items, d), dtype=np.float32) * np.float32(scale))
    if kind == "one_norm":            # entries of one magnitude: every row's sum of squares is 2 exactly, in any order of summation
        V = (0.125 * rng.choice(np.float32([-1, 1]), (n_items, d))).astype(np.float32)
    elif kind == "lognormal":
        V = (V * np.exp(rng.normal(0.0, 0.3, (n_items, 1)))).astype(np.float32)
    elif kind == "zero_rows":
        V[rng.random(n_items) < 0.1] = 0.0
        V[-1] = 0.0
    return U, V


def _rated(rng, n_users, lo, hi, max_len=40, every=None, every_min=0):
    """Rated lists as CSR (int64 row offsets, ascending distinct int32 ids per user): 0 .. max_len - 1 uniform ids of [lo, hi)
    per user; `every`: ids of which each user also rates the first every_min .. len(every)."""
    lens = rng.integers(0, max_len, n_users)
    owner = np.repeat(np.arange(n_users, dtype=np.int64), lens)
    ids = rng.integers(lo, hi, owner.shape[0], dtype=np.int64)
    if every is not None:
        cnt = rng.integers(every_min, len(every) + 1, n_users)
        owner = np.concatenate([owner, np.repeat(np.arange(n_users, dtype=np.int64), cnt)])
        ids = np.concatenate([ids, np.asarray(every, np.int64)[np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)]])
    key = np.unique((owner << 32) | ids)
    rowptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=n_users), out=rowptr[1:])
    return rowptr, (key & 0xFFFFFFFF).astype(np.int32)


def _bitmap(n_global, ids, dev):
    words = np.zeros((n_global + 31) // 32 + 1, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.int64)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).to(dev)


def _run(monkeypatch, mode, order, U, V, k, rated, bitmap_ids, n_global, item_base):
    dev = _dev()
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", str(order))
    rp, rc = (torch.from_numpy(rated[0]).to(dev), torch.from_numpy(rated[1]).to(dev)) if rated is not None else (None, None)
    bm = _bitmap(n_global, bitmap_ids, dev)
    route = ops.score_topk_route(U.shape[0], V.shape[0], V.shape[1], k, has_bitmap=True)
    ordered = ops.score_topk_screen_ordered(U.shape[0], V.shape[0], V.shape[1], k, has_bitmap=True)
    s, i = ops.score_topk(torch.from_numpy(U).to(dev), None, torch.from_numpy(V).to(dev), k, rp, rc, bm, item_base=item_base)
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if route["screened"] else None
    return s.cpu().numpy(), i.cpu().numpy(), route, ordered, unc


def _check(monkeypatch, U, V, k=K, rated=None, bitmap_ids=(), item_base=0, n_global=None, mode=2, expect_ordered=True):
    """(a), (b), (c) of the module's docstring; returns the uncertified count."""
    n_global = item_base + V.shape[0] if n_global is None else n_global
    args = (U, V, k, rated, bitmap_ids, n_global, item_base)
    s0, i0, r0, _, _ = _run(monkeypatch, 0, 1, *args)
    assert not r0["screened"]
    s1, i1, r1, o1, unc1 = _run(monkeypatch, mode, 1, *args)
    assert r1["screened"], r1
    assert o1 == expect_ordered
    assert np.array_equal(i1, i0), np.argwhere((i1 != i0).any(1))[:5]
    assert np.array_equal(s1.view(np.uint32), s0.view(np.uint32))
    s2, i2, r2, o2, unc2 = _run(monkeypatch, mode, 0, *args)
    assert r2["screened"] and not o2
    assert np.array_equal(i1, i2), np.argwhere((i1 != i2).any(1))[:5]
    assert np.array_equal(s1.view(np.uint32), s2.view(np.uint32))
    print("uncertified users: order on %d, off %d of %d" % (unc1, unc2, U.shape[0]))
    assert unc1 == unc2
    return unc1


def _prefix(n_items):
    return PREFIX if n_items >= 8 * PREFIX else 0


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("share", [0.2, 0.8])
def test_order_masked_share(monkeypatch, n_items, share):
    rng = np.random.default_rng(41)
    U, V = _tables(rng, n_items)
    cold = np.where(rng.random(n_items) < share)[0]
    unc = _check(monkeypatch, U, V, rated=_rated(rng, U.shape[0], 0, n_items), bitmap_ids=cold)
    assert unc == 0          # gaussian tables: the K' = 28 margin certifies every user


@pytest.mark.parametrize("n_items", SIZES)
def test_order_off_grid_item_base(monkeypatch, n_items):
    rng = np.random.default_rng(42)
    base = 1_000_003
    n_global = base + n_items + 5000
    assert (base + _prefix(n_items)) % 32 != 0 and (base + n_items) % 32 != 0
    U, V = _tables(rng, n_items)
    cold = base + np.where(rng.random(n_items) < 0.2)[0]
    rated = _rated(rng, U.shape[0], base - 50, base + n_items + 50)
    _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold, item_base=base, n_global=n_global)


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("live", [0, 1])
def test_order_main_range_nearly_empty(monkeypatch, n_items, live):
    """No live row / a single live row in the main range (the prefix, where there is one, keeps its mask of 20 %)."""
    rng = np.random.default_rng(43)
    U, V = _tables(rng, n_items)
    P = _prefix(n_items)
    cold = rng.random(n_items) < 0.2
    cold[P:] = True
    if live:
        cold[P + (n_items - P) // 3] = False
    _check(monkeypatch, U, V, rated=_rated(rng, U.shape[0], 0, n_items), bitmap_ids=np.where(cold)[0])


@pytest.mark.parametrize("n_items", SIZES)
def test_order_rated_lists_hold_the_highest_norms(monkeypatch, n_items):
    """The rows streamed first are rated by every user: they enter no list, and the thresholds must not rise on them."""
    rng = np.random.default_rng(44)
    U, V = _tables(rng, n_items, "lognormal")
    cold = np.where(rng.random(n_items) < 0.2)[0]
    live = np.setdiff1d(np.arange(_prefix(n_items), n_items), cold)
    top = live[np.argsort(-(V[live].astype(np.float64) ** 2).sum(1))[:60]]
    rated = _rated(rng, U.shape[0], 0, n_items, every=top, every_min=30)
    _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold)


@pytest.mark.parametrize("n_items", SIZES)
def test_order_k1(monkeypatch, n_items):
    rng = np.random.default_rng(45)
    U, V = _tables(rng, n_items)
    _check(monkeypatch, U, V, k=1, rated=_rated(rng, U.shape[0], 0, n_items), bitmap_ids=np.where(rng.random(n_items) < 0.2)[0])


@pytest.mark.parametrize("n_items", SIZES)
@pytest.mark.parametrize("kind", ["one_norm", "lognormal", "zero_rows"])
def test_order_norm_shapes(monkeypatch, n_items, kind):
    """One key for every row (the ascending order), widely spread keys, rows of zeros (the key that sorts last)."""
    rng = np.random.default_rng(46)
    U, V = _tables(rng, n_items, kind)
    _check(monkeypatch, U, V, rated=_rated(rng, U.shape[0], 0, n_items), bitmap_ids=np.where(rng.random(n_items) < 0.2)[0])


@pytest.mark.parametrize("n_items", SIZES)
def test_order_nan_and_inf_rows(monkeypatch, n_items):
    """One NaN row and one inf row, both live: no user certifies and the fallback answers."""
    rng = np.random.default_rng(47)
    U, V = _tables(rng, n_items)
    cold = rng.random(n_items) < 0.2
    P = _prefix(n_items)
    a, b = P + (n_items - P) // 4, P + (n_items - P) // 2
    cold[[a, b]] = False
    V[a, 5] = np.nan
    V[b, 77] = np.inf
    unc = _check(monkeypatch, U, V, rated=_rated(rng, U.shape[0], 0, n_items), bitmap_ids=np.where(cold)[0])
    assert unc == U.shape[0]


@pytest.mark.parametrize("n_items", SIZES)
def test_order_no_user_certified(monkeypatch, n_items):
    """CRH_SCORE_SCREEN=3: every user goes through the exact fallback."""
    rng = np.random.default_rng(48)
    U, V = _tables(rng, n_items)
    unc = _check(monkeypatch, U, V, rated=_rated(rng, U.shape[0], 0, n_items), bitmap_ids=np.where(rng.random(n_items) < 0.2)[0],
                 mode=3)
    assert unc == U.shape[0]


def test_order_not_with_cuts(monkeypatch):
    """Few users over a long range: the fp16 pass cuts the item range, the cuts' bounds need the ascending map, and the call
    reports "not ordered" and answers as before (the shape of test_screen_compact_gpu.test_compact_cuts)."""
    rng = np.random.default_rng(26)
    n_users, n_items = 130, 300_000
    U, V = _tables(rng, n_items, n_users=n_users)
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    assert not ops.score_topk_screen_ordered(300, 70_001, 128, K)
    assert ops.score_topk_screen_plan(n_users, n_items, 128, K)["cuts"] > 1
    assert not ops.score_topk_screen_ordered(n_users, n_items, 128, K)
    cold = np.where(rng.random(n_items) < 0.2)[0]
    unc = _check(monkeypatch, U, V, rated=_rated(rng, n_users, 0, n_items), bitmap_ids=cold, expect_ordered=False)
    assert unc == 0


@pytest.mark.parametrize("n_items,prefix", [(70_001, PREFIX), (5_000, 0)])
@pytest.mark.parametrize("kind", ["gauss", "lognormal", "zero_rows", "one_norm", "nonfinite"])
@pytest.mark.parametrize("base", [0, 1_000_003])
def test_order_map(n_items, prefix, kind, base):
    """The map out of stage 0 alone: the first `count` entries are exactly the unmasked ids of the main range, each once; the keys
    along the map do not increase; ids ascend inside a key; two runs give the same map; the keys are those of the rows."""
    dev = _dev()
    rng = np.random.default_rng(49)
    _, V = _tables(rng, n_items, "gauss" if kind == "nonfinite" else kind, n_users=1)
    cold = rng.random(n_items) < 0.2
    if kind == "nonfinite":
        a, b = prefix + 100, n_items - 7
        cold[[a, b]] = False
        V[a, 3] = np.nan
        V[b, 100] = -np.inf
    n_global = base + n_items + 100
    bm = _bitmap(n_global, base + np.where(cold)[0], dev)
    tv = torch.from_numpy(V).to(dev)
    want = base + prefix + np.where(~cold[prefix:])[0]
    m_asc, k_asc = (t.cpu().numpy() for t in ops.score_topk_screen_map(bm, tv, base, prefix, ordered=False))
    assert np.array_equal(m_asc, want)
    m, keys = (t.cpu().numpy() for t in ops.score_topk_screen_map(bm, tv, base, prefix, ordered=True))
    assert len(m) == len(want) and np.array_equal(np.sort(m), want)
    assert (np.diff(keys) <= 0).all()
    same = np.diff(keys) == 0
    assert (np.diff(m)[same] > 0).all()
    m2, keys2 = (t.cpu().numpy() for t in ops.score_topk_screen_map(bm, tv, base, prefix, ordered=True))
    assert np.array_equal(m, m2) and np.array_equal(keys, keys2)
    # the keys are the rows' own: the same multiset as along the ascending map, and each the high half of an fp32 sum of
    # squares: its roundings (relative 2^-24 each, a few per addend of a sum of positive terms) stay far inside 2^-16, and that
    # moves a sum across one step of the key (2^-7) at the most
    assert np.array_equal(keys, k_asc[np.argsort(-k_asc, kind="stable")])
    ss = (V[m - base].astype(np.float64) ** 2).sum(1)
    finite = np.isfinite(ss)
    assert (keys[~finite] == 0x7F80).all()
    lo = ((ss[finite] * (1 - 2.0 ** -16)).astype(np.float32)).view(np.uint32) >> 16
    hi = ((ss[finite] * (1 + 2.0 ** -16)).astype(np.float32)).view(np.uint32) >> 16
    assert ((keys[finite] >= lo) & (keys[finite] <= hi)).all()
    if kind == "one_norm":
        assert np.array_equal(m, want)
