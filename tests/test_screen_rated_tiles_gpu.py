"""The rated-tile flags of the screened route's fp16 pass on the GPU (run with -m gpu on an MI355X).

Under a candidate bitmap the pass streams the live rows only, and a call with rated lists flags, per workgroup of 512 slots and
32-row tile of that stream, the waves (128 slots) that rated a row of the tile.  A candidate in a tile whose bit is clear is
unrated by construction and skips the membership filter and the list search.  The flags may move neither an output nor the number
of uncertified users.

A flag that is wrongly CLEAR lets a rated row into a list; stage 2 then refuses the user (a rated candidate certifies nobody) and
the exact fallback still returns the right rows -- so such a fault shows in `score_topk_uncertified`, which every case compares
between CRH_SCORE_SCREEN_RATED_TILES=1 and =0, and in the flags themselves, which are compared word for word with a numpy
restatement.  A flag that is wrongly SET costs time only; nothing but the word-for-word comparison sees it.

Tables are random (d = 128, k = 20, CRH_SCORE_SCREEN=2, a bitmap that leaves about 80 % of the rows).  The rated lists are built from the
exact scores: some of each user's three best rows go into its own list (they must vanish from the output), and the best row of
some users goes into the list of a user of ANOTHER wave of the same workgroup (it must stay)."""
import ctypes

import numpy as np
import pytest
import torch

from coldrec_amd import _lib, ops
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

K, D = 20, 128
OFF_GRID_BASE = 1_000_003


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# ---- the flags, restated
def flags_np(stream_ids, rated, n_users, n_main):
    """[workgroups][blocks * 64] uint32: tile t of the stream in word t >> 3, nibble 4 (t & 7), bit w for wave w of the workgroup.
    stream_ids: the ids of the live rows of the main range in stream order; an id that is not among them (prefix, cold, outside the
    shard) sets nothing."""
    row_of = {int(g): q for q, g in enumerate(stream_ids)}
    groups = ((n_users + 127) // 128 + 3) // 4
    blocks = ((n_main + 31) // 32 + 511) // 512
    out = np.zeros((groups, blocks * 64), np.uint32)
    for slot in range(n_users):
        wave = slot // 128
        for g in (rated[slot] if rated[slot] is not None else ()):
            q = row_of.get(int(g))
            if q is not None:
                t = q >> 5
                out[wave // 4, t >> 3] |= np.uint32(1 << (4 * (t & 7) + (wave & 3)))
    return out


# ---- cases: tables, bitmap, rated lists; built once, read-only
_cases = {}


def _tables(n_users, n_items, seed):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((n_users, D), dtype=np.float32)
    V = rng.standard_normal((n_items, D), dtype=np.float32)
    V *= np.exp(rng.normal(0.0, 0.2, (n_items, 1))).astype(np.float32)          # some spread of the norms: the ordered map is no identity
    cold = np.where(rng.random(n_items) < 0.2)[0]
    return rng, U, V, cold


def _planted_lists(rng, U, V, cold, item_base, n_extra):
    """Rated lists from the exact scores.  Slot j rates 1 .. 3 of its own three best live rows -- but a slot 128 q + 5 never its very
    best one: that row goes into the list of slot 128 ((q + 3) % 4) + 5 of the SAME workgroup, another wave, when that slot exists
    -- plus n_extra random ids.  Returns (lists of global ids, own: [n_users][3] local ids with -1 where not rated, kept: {slot:
    local id of a row somebody else rated})."""
    n_users, n_items = U.shape[0], V.shape[0]
    S = U @ V.T
    S[:, cold] = -np.inf
    top3 = np.argsort(-S, axis=1)[:, :3]
    own = np.full((n_users, 3), -1, np.int64)
    rated = []
    for j in range(n_users):
        m = 1 + j % 3
        mine = top3[j, 1:1 + m] if j % 128 == 5 else top3[j, :m]
        own[j, :len(mine)] = mine
        extra = set(int(x) for x in rng.integers(0, n_items, n_extra)) - {int(top3[j, 0])}
        rated.append(set(int(x) for x in mine) | extra)
    kept = {}
    for j in range(5, n_users, 128):
        wave = j // 128
        other = (wave // 4) * 512 + ((wave % 4 + 1) % 4) * 128 + 5
        if other < n_users:
            rated[j].add(int(top3[other, 0]))
            kept[other] = int(top3[other, 0])
    lists = [np.array(sorted(r), np.int64) + item_base for r in rated]
    return lists, own, kept


def case_prefix():
    """700 x 90 001, an 8 192-row prefix, an off-grid base: the main range in cuts, id order, four blocks of flags."""
    if "prefix" not in _cases:
        rng, U, V, cold = _tables(700, 90_001, 20)
        lists, own, kept = _planted_lists(rng, U, V, cold, OFF_GRID_BASE, 40)
        _cases["prefix"] = dict(U=U, V=V, cold=cold, rated=lists, own=own, kept=kept, item_base=OFF_GRID_BASE, prefix=8192)
    return _cases["prefix"]


def case_ordered():
    """600 x 4 000, no prefix, one cut, streamed by descending norm."""
    if "ordered" not in _cases:
        rng, U, V, cold = _tables(600, 4000, 21)
        lists, own, kept = _planted_lists(rng, U, V, cold, 0, 30)
        _cases["ordered"] = dict(U=U, V=V, cold=cold, rated=lists, own=own, kept=kept, item_base=0, prefix=0)
    return _cases["ordered"]


def _plans(n_users, n_items, has_rated=True):
    plan = ops.score_topk_screen_plan(n_users, n_items, D, K, has_bitmap=True)
    return (plan["cuts"], plan["compact"], ops.score_topk_screen_ordered(n_users, n_items, D, K, has_bitmap=True),
            ops.score_topk_screen_rated_tiles(n_users, n_items, D, K, has_bitmap=True, has_rated=has_rated))


def _run(monkeypatch, mode, switch, case, users=None, rated="case", ws_bytes=None):
    """One score_topk call: (scores, ids, uncertified or None).  ws_bytes: call the library with a workspace of that many bytes."""
    dev = _dev()
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    monkeypatch.setenv("CRH_SCORE_SCREEN_RATED_TILES", str(switch))
    base = case["item_base"]
    if "Ut" not in case:          # (device copies made once per case)
        case["Ut"], case["Vt"] = torch.from_numpy(case["U"]).to(dev), torch.from_numpy(case["V"]).to(dev)
        case["bm"] = ops.make_bitmap(base + case["Vt"].shape[0], case["cold"] + base, dev)
    Ut, Vt, bm = case["Ut"], case["Vt"], case["bm"]
    lists = case["rated"] if isinstance(rated, str) else rated
    if lists is not None and users is not None:
        lists = [lists[u] for u in users]
    rp, rc = ops.rated_csr(lists, dev) if lists is not None else (None, None)
    ut = None if users is None else torch.from_numpy(np.asarray(users, np.int32)).to(dev)
    n_users = Ut.shape[0] if users is None else len(users)
    if ws_bytes is None:
        s, i = ops.score_topk(Ut, ut, Vt, K, rp, rc, bm, item_base=base)
    else:
        s = torch.empty((n_users, K), dtype=torch.float32, device=dev)
        i = torch.empty((n_users, K), dtype=torch.int32, device=dev)
        ws = ops._workspace(ws_bytes, dev)
        code = _lib.lib().crh_score_topk_f32_ex(_lib.ptr(Ut), _lib.ptr(ut), n_users, _lib.ptr(Vt), Vt.shape[0], D, _lib.ptr(rp), _lib.ptr(rc),
                                                _lib.ptr(bm), K, base, _lib.ptr(s), _lib.ptr(i), _lib.ptr(ws), ws_bytes,
                                                _lib.current_stream(), 0, None, None)
        _lib.check(code, "crh_score_topk_f32_ex")
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if mode else None
    return s.cpu().numpy(), i.cpu().numpy(), unc


def _same(a, b):
    return np.array_equal(a[1], b[1]) and np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _oracle_rows(case, got, users=None, lists="case", n_sample=6):
    """Sampled slots of `got` against the C oracle."""
    n = got[1].shape[0]
    pick = np.unique(np.concatenate([np.random.default_rng(0).integers(0, n, n_sample), [0, n - 1]]))
    rows = pick if users is None else np.asarray(users)[pick]
    lists = case["rated"] if isinstance(lists, str) else lists
    rowptr = col = None
    if lists is not None:
        rr = [lists[r] for r in rows]
        rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
        col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
    bm = orc.make_bitmap(case["item_base"] + case["V"].shape[0], case["cold"] + case["item_base"])
    ws, wi = orc.score_topk(case["U"], rows.astype(np.int64), case["V"], K, rowptr, col, bm, item_base=case["item_base"])
    assert np.array_equal(got[1][pick], wi)
    assert np.array_equal(got[0][pick].view(np.uint32), ws.view(np.uint32))


def _three_way(monkeypatch, case, users=None, rated="case", ws_bytes=None):
    """exact route == screened with the flags == screened without them (bytes and uncertified count); returns the outputs."""
    exact = _run(monkeypatch, 0, 1, case, users, rated)
    on = _run(monkeypatch, 2, 1, case, users, rated, ws_bytes)
    off = _run(monkeypatch, 2, 0, case, users, rated, ws_bytes)
    print("uncertified: flags on %d, off %d" % (on[2], off[2]))
    assert _same(on, exact), np.argwhere((on[1] != exact[1]).any(1))[:5]
    assert _same(off, exact)
    assert on[2] == off[2], (on[2], off[2])
    return exact


# ---- the flags against the restatement
def _stream_ids(case, ordered):
    dev = _dev()
    base, V = case["item_base"], case["V"]
    bm = ops.make_bitmap(base + V.shape[0], case["cold"] + base, dev)
    ids, _ = ops.score_topk_screen_map(bm, torch.from_numpy(V).to(dev), item_base=base, prefix=case["prefix"], ordered=ordered)
    return bm, ids.cpu().numpy()


def _flag_lists(case, ids, n_users):
    """Rated lists that hit the corners: the first and the last row of a 512-tile block, the last (partial) tile, the prefix, cold
    rows, ids outside the shard on both sides, one id twice in a list and in two lists of one wave."""
    base, n_items = case["item_base"], case["V"].shape[0]
    rated = [None] * n_users
    n_live = len(ids)
    edge = 512 * 32 if n_live > 512 * 32 else 0
    rated[3] = [ids[edge]]                                        # first row of a block (slot 3: wave 0)
    rated[130] = [ids[edge - 1 if edge else n_live // 2]]         # last row of the block before (wave 1)
    rated[n_users - 1] = [ids[n_live - 1], ids[n_live - 1]]       # the last, partial tile; twice in one list (the last wave)
    rated[131] = [ids[n_live - 1]]                                # ... and once more from another wave
    rated[7] = [base + 5] if case["prefix"] else [ids[0]]         # a row of the prefix: not in the stream
    rated[260] = [int(case["cold"][len(case["cold"]) // 2]) + base, int(case["cold"][-1]) + base]      # cold rows (wave 2)
    rated[8] = [base - 1] if base else [ids[1]]                   # below the shard
    rated[9] = [base + n_items, base + n_items + 700]             # above it
    rated[400] = [ids[33], ids[64], ids[n_live // 3]]             # wave 3
    rated[401] = [ids[33]]                                        # the same bit again
    return [None if r is None else np.asarray(r, np.int64) for r in rated]


@pytest.mark.parametrize("name", ["prefix", "ordered"])
def test_flags_equal_restatement(name):
    case = case_prefix() if name == "prefix" else case_ordered()
    n_users, n_items, ordered = case["U"].shape[0], case["V"].shape[0], name == "ordered"
    cuts, compact, ord_plan, rt = _plans(n_users, n_items)
    assert compact and rt and ord_plan == ordered and (cuts == 1) == ordered, (cuts, compact, ord_plan, rt)
    bm, ids = _stream_ids(case, ordered)
    n_main = n_items - case["prefix"]
    assert len(ids) % 32 != 0 and (name != "prefix" or len(ids) > 3 * 512 * 32)       # a partial last tile; four blocks
    for lists in (_flag_lists(case, ids, n_users), case["rated"]):
        rp, rc = ops.rated_csr(lists, _dev())
        got = ops.score_topk_screen_flags(bm, torch.from_numpy(case["V"]).to(_dev()), rp, rc, item_base=case["item_base"],
                                          prefix=case["prefix"], ordered=ordered).cpu().numpy().view(np.uint32)
        want = flags_np(ids, lists, n_users, n_main)
        assert got.shape == want.shape, (got.shape, want.shape)
        assert np.array_equal(got, want), np.argwhere(got != want)[:8]
        assert want.any()


# ---- ranking
@pytest.mark.parametrize("name", ["prefix", "ordered"])
def test_ranking(monkeypatch, name):
    case = case_prefix() if name == "prefix" else case_ordered()
    n_users, n_items, ordered = case["U"].shape[0], case["V"].shape[0], name == "ordered"
    cuts, compact, ord_plan, rt = _plans(n_users, n_items)
    assert compact and rt and ord_plan == ordered and (cuts == 1) == ordered, (cuts, compact, ord_plan, rt)
    exact = _three_way(monkeypatch, case)
    _oracle_rows(case, exact)
    ids = exact[1].astype(np.int64) - case["item_base"]
    for j in range(n_users):                          # a user's own rated rows vanish ...
        mine = case["own"][j][case["own"][j] >= 0]
        assert len(mine) >= 1 and not np.isin(mine, ids[j]).any(), j
    assert len(case["kept"]) >= 3
    for j, row in case["kept"].items():               # ... a row that another wave of the workgroup rated stays
        assert row in ids[j], (j, row)


def test_one_long_cut(monkeypatch):
    """600 x 2.6 M: every cut spans three or more 512-tile blocks of flags and starts off a block boundary, so both buffers are
    refilled while the cut streams.  Tables are drawn on the device; the lists hold each user's three best rows and 40 random ids."""
    dev = _dev()
    n_users, n_items, base = 600, 2_600_017, 0
    cuts, compact, ordered, rt = _plans(n_users, n_items)
    assert compact and rt and not ordered and cuts > 1, (cuts, compact, ordered, rt)
    g = torch.Generator(device=dev)
    g.manual_seed(22)
    U = torch.randn((n_users, D), generator=g, device=dev)
    V = torch.randn((n_items, D), generator=g, device=dev)
    cold = torch.nonzero(torch.rand(n_items, generator=g, device=dev) < 0.2).flatten().cpu().numpy()
    case = dict(Ut=U, Vt=V, cold=cold, item_base=base, rated=None, prefix=8192)
    case["bm"] = ops.make_bitmap(n_items, cold, dev)
    # the cuts' tile ranges [NT c / S, NT (c + 1) / S) over the live rows of the main range: most touch three blocks of 512 tiles (the
    # prologue brings two, the third is fetched while the cut streams, into the buffer of the first) and start off a block boundary
    NT = ((n_items - 8192) - int((cold >= 8192).sum()) + 31) // 32
    t0 = NT * np.arange(cuts + 1) // cuts
    spans = (t0[1:] - 1) // 512 - t0[:-1] // 512 + 1
    print("cuts %d, tiles %d; blocks touched per cut: %s" % (cuts, NT, np.bincount(spans)))
    assert (spans >= 3).sum() > cuts // 2 and ((t0[:-1] % 512 != 0) & (spans >= 3)).sum() > cuts // 2
    first = _run(monkeypatch, 0, 1, case, rated=None)
    rng = np.random.default_rng(23)
    lists = [np.unique(np.concatenate([first[1][j, :3].astype(np.int64), rng.integers(0, n_items, 40)])) for j in range(n_users)]
    exact = _three_way(monkeypatch, case, rated=lists)
    for j in range(n_users):
        assert not np.isin(first[1][j, :3], exact[1][j]).any(), j


# ---- callers off the grid
def test_users_vector_with_repeats(monkeypatch):
    case = case_ordered()
    users = np.concatenate([np.arange(0, 600, 7), [5, 5, 5, 133, 133], np.arange(599, 300, -11)])
    plans = _plans(len(users), 4000)
    print("plan (cuts, compact, ordered, rated tiles):", plans)
    assert plans[1] and plans[3], plans
    exact = _three_way(monkeypatch, case, users=users)
    _oracle_rows(case, exact, users=users)


@pytest.mark.parametrize("n_users", [130, 515])
def test_dead_waves(monkeypatch, n_users):
    """130 slots: two live waves and two dead ones in the only workgroup; 515: a second workgroup with one live wave of three slots."""
    case = case_ordered()
    users = np.arange(n_users)
    plans = _plans(n_users, 4000)
    print("plan (cuts, compact, ordered, rated tiles):", plans)
    assert plans[1] and plans[3], plans
    exact = _three_way(monkeypatch, case, users=users)
    _oracle_rows(case, exact, users=users)


def test_no_rated_lists(monkeypatch):
    case = case_ordered()
    assert _plans(600, 4000, has_rated=False)[1:] == (True, True, False)
    exact = _three_way(monkeypatch, case, rated=None)
    _oracle_rows(case, exact, lists=None)


def test_workspace_without_room_for_the_flags(monkeypatch):
    """The largest workspace that does not hold the flags: the call keeps its route, compaction and order, and its results."""
    case = case_ordered()
    L = _lib.lib()
    full = int(L.crh_score_topk_workspace_bytes(600, 4000, D, K))
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    monkeypatch.setenv("CRH_SCORE_SCREEN_RATED_TILES", "1")
    assert L.crh_score_topk_screen_rated_tiles(600, 4000, full, 1, 1) == 1
    assert L.crh_score_topk_screen_ordered(600, 4000, full, 1) == 1
    lo, hi = 0, full                                      # the smallest workspace of the ordered plan ...
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if L.crh_score_topk_screen_ordered(600, 4000, mid, 1) else (mid, hi)
    lo = hi                                               # ... which does not hold the flags; above it the plan no longer changes
    assert L.crh_score_topk_screen_rated_tiles(600, 4000, lo, 1, 1) == 0
    hi = full
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if L.crh_score_topk_screen_rated_tiles(600, 4000, mid, 1, 1) else (mid, hi)
    cuts, compact = ctypes.c_int32(0), ctypes.c_int32(0)
    _lib.check(L.crh_score_topk_screen_plan(600, 4000, lo, 1, ctypes.byref(cuts), ctypes.byref(compact)), "crh_score_topk_screen_plan")
    assert L.crh_score_topk_screened(4, 600, 4000, D, K, lo, 1, 0) == 1 and compact.value == 1 and cuts.value == 1
    assert L.crh_score_topk_screen_ordered(600, 4000, lo, 1) == 1 and L.crh_score_topk_screen_rated_tiles(600, 4000, lo, 1, 1) == 0
    small = _three_way(monkeypatch, case, ws_bytes=lo)
    assert _same(small, _run(monkeypatch, 2, 1, case))    # ... and equal the call with the full workspace
