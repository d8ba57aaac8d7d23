"""The screened route of fp32 d=128 ranking (run with -m gpu on an MI355X).

An fp16 screen keeps 28 candidates per user, the candidates are rescored with the canonical fmaf chain, and a per-user error
bound certifies that nothing else can enter the top-k; the other users take an exact fallback.  Every case asserts that the
screened call returns exactly what the exact route returns (CRH_SCORE_SCREEN=0), bit for bit and for every user, and matches the
C oracle on sampled users.  CRH_SCORE_SCREEN=2 screens these small shapes; 3 certifies nobody, so every user goes through the
fallback."""
import numpy as np
import pytest
import torch

from coldrec_amd import ops
from oracle import oracle_np as orc

pytestmark = pytest.mark.gpu

K = 20


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _rated(rng, n_users, lo, hi, max_len=40):
    return [np.unique(rng.integers(lo, hi, int(rng.integers(0, max_len)))) for _ in range(n_users)]


def _run(monkeypatch, mode, U, users, V, k, rated, bitmap_ids, n_global, item_base):
    dev = _dev()
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    rp, rc = ops.rated_csr(rated, dev) if rated is not None else (None, None)
    bm = ops.make_bitmap(n_global, bitmap_ids, dev) if bitmap_ids is not None else None
    tu = torch.from_numpy(users).to(dev) if users is not None else None
    n_users = U.shape[0] if users is None else len(users)
    route = ops.score_topk_route(n_users, V.shape[0], V.shape[1], k, has_bitmap=bm is not None)
    s, i = ops.score_topk(torch.from_numpy(U).to(dev), tu, torch.from_numpy(V).to(dev), k, rp, rc, bm, item_base=item_base)
    torch.cuda.synchronize()
    unc = ops.score_topk_uncertified() if route["screened"] else None
    return s.cpu().numpy(), i.cpu().numpy(), route, unc


def _check(monkeypatch, U, V, k=K, users=None, rated=None, bitmap_ids=None, item_base=0, n_sample=24, seed=0, oracle=True):
    """Screened (mode 2) == exact (mode 0) for every user, == oracle on sampled users; returns the uncertified count."""
    n_global = item_base + V.shape[0]
    s0, i0, r0, _ = _run(monkeypatch, 0, U, users, V, k, rated, bitmap_ids, n_global, item_base)
    assert not r0["screened"]
    s2, i2, r2, unc = _run(monkeypatch, 2, U, users, V, k, rated, bitmap_ids, n_global, item_base)
    assert r2["screened"], r2
    assert np.array_equal(i2, i0), np.argwhere((i2 != i0).any(1))[:5]
    assert np.array_equal(s2.view(np.uint32), s0.view(np.uint32))
    s3, i3, r3, unc3 = _run(monkeypatch, 3, U, users, V, k, rated, bitmap_ids, n_global, item_base)
    assert r3["screened"] and unc3 == s0.shape[0]
    assert np.array_equal(i3, i0) and np.array_equal(s3.view(np.uint32), s0.view(np.uint32))
    if oracle:
        rng = np.random.default_rng(seed)
        n = s0.shape[0]
        pick = np.unique(rng.integers(0, n, n_sample))
        urows = pick if users is None else users[pick]
        rr = [rated[j] for j in pick] if rated is not None else None
        rowptr = col = None
        if rr is not None:
            rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rr])]).astype(np.int64)
            col = np.concatenate(rr + [np.zeros(0, np.int64)]).astype(np.int64)
        bm = orc.make_bitmap(n_global, bitmap_ids) if bitmap_ids is not None else None
        ws, wi = orc.score_topk(U, urows.astype(np.int64), V, k, rowptr, col, bm, item_base=item_base)
        assert np.array_equal(i0[pick], wi)
        assert np.array_equal(s0[pick].view(np.uint32), ws.view(np.uint32))
    return unc


def _tables(rng, n_users, n_items, d=128, scale=0.1):
    return ((rng.standard_normal((n_users, d)) * scale).astype(np.float32),
            (rng.standard_normal((n_items, d)) * scale).astype(np.float32))


@pytest.mark.parametrize("masks", [False, True])
def test_screen_equals_exact(monkeypatch, masks):
    rng = np.random.default_rng(1)
    U, V = _tables(rng, 3000, 100_000)
    rated = _rated(rng, 3000, 0, 100_000) if masks else None
    cold = np.where(rng.random(100_000) < 0.2)[0] if masks else None
    unc = _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold)
    assert unc == 0          # gaussian tables: the K' = 28 margin certifies every user


def test_screen_duplicates_across_boundary(monkeypatch):
    """Rows repeated across ranks k .. K' (and beyond): exact ties the certificate must refuse and the fallback must order."""
    rng = np.random.default_rng(2)
    U, V = _tables(rng, 1500, 70_000)
    for j in range(0, 60):                      # user j's direction, 15..40 copies: ties straddle 20 and 28
        row = U[j] / np.linalg.norm(U[j]) * 2.0
        ids = rng.choice(70_000, 15 + (j % 26), replace=False)
        V[ids] = row
    _check(monkeypatch, U, V, bitmap_ids=np.where(rng.random(70_000) < 0.1)[0])


def test_screen_few_unmasked_items(monkeypatch):
    """Catalogues where most users have fewer than K' (or k) unmasked items: -1e9 entries and padding."""
    rng = np.random.default_rng(3)
    n_items = 48
    U, V = _tables(rng, 700, n_items)
    rated = _rated(rng, 700, 0, n_items, max_len=40)
    cold = np.arange(0, n_items, 3)
    _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold)
    _check(monkeypatch, U, V[:13], rated=[r[r < 13] for r in rated])      # fewer items than k: padded lists


def test_screen_off_grid_base_cuts_and_users(monkeypatch):
    """An item shard at an off-grid base, few users (the screen cuts the item range and merges), users through `users`."""
    rng = np.random.default_rng(4)
    n_rows, n_items, base = 4000, 90_001, 1_000_003
    U, V = _tables(rng, n_rows, n_items)
    users = rng.integers(0, n_rows, 333).astype(np.int32)
    users[:5] = users[5]                         # repeated rows
    rated = _rated(rng, 333, base - 50, base + n_items + 50)
    cold = base + np.where(rng.random(n_items) < 0.2)[0]
    unc = _check(monkeypatch, U, V, users=users, rated=rated, bitmap_ids=cold, item_base=base)
    assert unc == 0


@pytest.mark.parametrize("scale", [1e-19, 1e17])
def test_screen_scale_extremes(monkeypatch, scale):
    """Whole tables near the ends of the fp32 range (the power-of-two scales) and rows of tiny magnitude inside a table (fp16
    subnormals, flushed into the residual)."""
    rng = np.random.default_rng(5)
    U, V = _tables(rng, 1200, 70_000)
    V[rng.random(70_000) < 0.3] *= np.float32(1e-6)
    U[:100] *= np.float32(1e-7)
    _check(monkeypatch, (U * np.float32(scale)).astype(np.float32), (V / np.float32(scale ** 0.5)).astype(np.float32))


def test_screen_non_finite_rows_fall_back(monkeypatch):
    rng = np.random.default_rng(6)
    U, V = _tables(rng, 800, 70_000)
    V[40_123] = np.nan
    V[50_000, 7] = np.inf
    rated = _rated(rng, 800, 0, 70_000)
    unc = _check(monkeypatch, U, V, rated=rated, oracle=False)
    assert unc == 800                            # R is not finite: no user can be certified


def test_screen_coarse_grid_many_fail(monkeypatch):
    """0/1 tables on four columns: every score is 0..4, the top 28 of a user are exact ties, so (almost) no user can be
    certified and the fallback ranks them."""
    rng = np.random.default_rng(7)
    U = np.zeros((900, 128), np.float32)
    V = np.zeros((70_000, 128), np.float32)
    U[:, :4] = rng.integers(0, 2, (900, 4))
    V[:, :4] = rng.integers(0, 2, (70_000, 4))
    unc = _check(monkeypatch, U, V, bitmap_ids=np.where(rng.random(70_000) < 0.2)[0])
    assert unc > 800


def test_screen_headline(monkeypatch):
    """131 072 users x 10 M items under the default dispatcher: screened, identical to the exact route for every user."""
    dev = _dev()
    n_users, n_items, d = 131072, 10_000_000, 128
    g = torch.Generator(device=dev).manual_seed(11)
    lim = (6.0 / (n_users + d)) ** 0.5
    U = (torch.rand((n_users, d), device=dev, generator=g) * 2 - 1) * lim
    lim = (6.0 / (n_items + d)) ** 0.5
    V = (torch.rand((n_items, d), device=dev, generator=g) * 2 - 1) * lim
    lens = torch.randint(0, 40, (n_users,), device=dev, generator=g)
    owner = torch.repeat_interleave(torch.arange(n_users, device=dev), lens)
    key = torch.unique(owner * n_items + torch.randint(0, n_items, owner.shape, device=dev, generator=g))
    rowptr = torch.zeros(n_users + 1, dtype=torch.int64, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(key // n_items, minlength=n_users), 0)
    col = (key % n_items).to(torch.int32)
    cold = torch.nonzero(torch.rand(n_items, device=dev, generator=g) < 0.2).flatten().cpu().numpy()
    bm = ops.make_bitmap(n_items, cold, dev)
    out = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("CRH_SCORE_SCREEN", mode)
        r = ops.score_topk_route(n_users, n_items, d, 20)
        assert r["screened"] == (mode == "1") and r["route"] == "fused-dma" and r["dma_form"] == "barrier"
        s, i = ops.score_topk(U, None, V, 20, rowptr, col, bm)
        torch.cuda.synchronize()
        if mode == "1":
            unc = ops.score_topk_uncertified()
            print("headline uncertified users:", unc)
        out[mode] = (s.cpu().numpy(), i.cpu().numpy())
    assert np.array_equal(out["1"][1], out["0"][1])
    assert np.array_equal(out["1"][0].view(np.uint32), out["0"][0].view(np.uint32))
    assert unc <= n_users // 1000
