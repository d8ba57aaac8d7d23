"""The premises of tests/test_screen_certificate_gpu.py, checked with the host model alone (no GPU).

The GPU module compares the library's uncertified count with oracle/screen_model.py on the inputs of tests/screen_cases.py.
That comparison pins the bound B_u only if the inputs are what they claim to be, so this module asserts, per sweep: both
score functions are exact on them (fp64 == float32 evaluation), the model's crossing lies in the middle half of the sweep,
deleting any term of B_u with a non-zero share moves the model's count by at least 5 users, and the guard band (users with
|e_k - (A_last + B_u)| < 1e-4 B_u, left out of the asserted count) holds at most 2 % of the sweep.  Per refusal case: the
victim is outside the approximate top 28 and inside the exact top k, the true error is at least half of B_u, the sound
predicate refuses, and the predicate without its dominant term certifies a list that is not the oracle's.

Model figures (400 users x 5 003 items, k = 20; uncertified users of the sound predicate, then with the term deleted):
    sweep   shares of B_u at the middle user (R, resid, g_d, g')     sound   -R    -resid   -g_d   -g'
    a       0      0      3.0 %   97.0 %                             192     192   192      126    0
    b       45.1 % 0      1.7 %   53.2 %                             197     0     197      161    0
    c       0      28.0 % 2.2 %   69.9 %                             198     198   0        172    0
    d       0      99.2 % 0.024 % 0.78 %                            198     198   0        190    0
"""
import numpy as np
import pytest

from oracle import oracle_np as orc
from oracle import screen_model as sm
from tests import screen_cases as sc

K = sc.K
GUARD = 1.0e-4
_cache = {}


def _sweep(kind):
    if kind not in _cache:
        case = sc.sweep(kind)
        _cache[kind] = (case, sc.model(case))
    return _cache[kind]


def _refusal(side):
    if side not in _cache:
        case = sc.refusal_item_side() if side == "item" else sc.refusal_user_side()
        _cache[side] = (case, sc.model(case))
    return _cache[side]


def _uncertified(res):
    return int((~res["cert"]).sum())


@pytest.mark.parametrize("kind", "abcd")
def test_sweep_scores_are_exact(kind):
    """fp64 and float32 evaluation agree: the approximate score over every item (products of the fp16 copies, summed in
    float32 in two different orders) and the fmaf chain over every item (C oracle against the fp64 dot product)."""
    case, _ = _sweep(kind)
    U, V = case["U"], case["V"]
    st = sm.stage0(U, V, np.arange(U.shape[0]), np.ones(V.shape[0], bool))
    sm.assert_products_exact(st["uh"], st["vh"])
    pick = np.array([0, 1, 199, 200, 398, 399])
    su, sv = 2.0 ** st["e_users"], 2.0 ** st["e_items"]
    uh32, vh32 = (st["uh"][pick] * su).astype(np.float32), (st["vh"] * sv).astype(np.float32)
    assert np.array_equal(uh32.astype(np.float64), st["uh"][pick] * su) and np.array_equal(vh32.astype(np.float64), st["vh"] * sv)
    want = (st["uh"][pick] * su) @ (st["vh"] * sv).T
    prod = uh32[:, None, :] * vh32[None, :, :]                            # float32 products (exact), two summation orders
    fwd = np.zeros(prod.shape[:2], np.float32)
    bwd = np.zeros(prod.shape[:2], np.float32)
    for c in range(128):
        fwd += prod[:, :, c]
        bwd += prod[:, :, 127 - c]
    assert np.array_equal(fwd.astype(np.float64), want) and np.array_equal(bwd.astype(np.float64), want)
    assert np.array_equal(prod.sum(2, dtype=np.float32).astype(np.float64), want)      # (pairwise)
    chain = orc.scores_dense(U, pick.astype(np.int64), V)
    assert np.array_equal(chain.astype(np.float64), U[pick].astype(np.float64) @ V.astype(np.float64).T)
    if kind == "a":                          # a == s wherever both rows are fp16-representable: here everywhere
        assert np.array_equal(want / (su * sv), chain.astype(np.float64))


@pytest.mark.parametrize("kind", "abcd")
def test_sweep_crossing_and_term_shares(kind):
    case, res = _sweep(kind)
    n = case["U"].shape[0]
    fails = ~res["cert"]
    sweep_users = n - 1 if kind == "d" else n                # (sweep d: the last user is the scale setter)
    assert res["cert"][sweep_users:].all()
    count = _uncertified(res)
    assert fails[n - count - (n - sweep_users):sweep_users].all() and not fails[:sweep_users - count].any()   # one crossing
    assert n // 4 <= sweep_users - count < 3 * n // 4, count
    gap = res["e_k"] - res["a_last"]
    assert np.array_equal(gap[:sweep_users], np.full(sweep_users, case["g"]))        # e_k - A_last is g for every user
    assert (np.diff(res["B"][:sweep_users]) > 0).all()
    mid = n // 2
    shares = res["terms"][mid] / res["B"][mid]
    print("sweep %s: g = %.6e, %d of %d uncertified, shares %s" % (kind, case["g"], count, n, np.round(shares, 5)))
    moved = {}
    for t, term in enumerate(sm.TERMS):
        moved[term] = _uncertified(sc.model(case, drop_term=term))
        if shares[t] > 0.0:
            assert abs(moved[term] - count) >= 5, (term, moved[term], count)
        else:
            assert moved[term] == count
    print("  with a term deleted: %s" % moved)
    want = {"a": (0, 0, 0.030, 0.970), "b": (0.45, 0, 0.017, 0.53), "c": (0, 0.28, 0.022, 0.70), "d": (0, 0.992, 2.44e-4, 0.0078)}[kind]
    assert np.allclose(shares, want, rtol=0.05), shares
    if kind == "d":                          # |u^| differs from |u| by more than the sweep's resolution
        step = np.diff(res["B"][:sweep_users]).max() / res["B"][mid]
        assert (res["un"][mid] - res["uhn"][mid]) / res["un"][mid] > 10 * step


@pytest.mark.parametrize("rated", [False, True])
@pytest.mark.parametrize("kind", "abcd")
def test_sweep_guard_band(kind, rated):
    res = sc.model(sc.sweep(kind, rated=True)) if rated else _sweep(kind)[1]
    _, inside = sm.guarded_count(res, GUARD)
    assert inside <= 0.02 * len(res["cert"]), inside


@pytest.mark.parametrize("kind,mask", [(kd, m) for kd in "abcd" for m in "RN"])
def test_masked_sweeps_follow_the_unmasked_rows(kind, mask):
    """What the masked GPU cases rest on: with the masked row counted in, the model's count is another one by >= 5 users, and the
    guard band of the masked sweep holds at most 2 %."""
    case = sc.sweep(kind, mask=mask)
    res = sc.model(case)
    n = case["U"].shape[0]
    count = _uncertified(res)
    assert n // 4 <= n - count < 3 * n // 4, count
    assert sm.guarded_count(res, GUARD)[1] <= 0.02 * n
    blind = dict(case, bitmap_ids=np.setdiff1d(case["bitmap_ids"], [case["ballast"]["r1" if mask == "R" else "n1"]]))
    other = _uncertified(sc.model(blind))
    print("sweep %s, %s row masked: %d uncertified; %d if the maxima covered the masked row" % (kind, mask, count, other))
    assert abs(other - count) >= 5


@pytest.mark.parametrize("side", ["item", "user"])
def test_refusal_case(side):
    case, res = _refusal(side)
    U, V, u, victim = case["U"], case["V"], case["victim_user"], case["victim"]
    ws, wi = orc.score_topk(U, None, V, K)
    assert victim not in res["cand"][u] and victim in wi[u]
    assert wi[u, 0] == victim                                            # the true best item
    st = sm.stage0(U, V, np.arange(U.shape[0]), np.ones(V.shape[0], bool))
    approx = float(st["uh"][u] @ st["vh"][victim])
    err = float(ws[u, 0]) - approx
    ratio = err / res["B"][u]
    print("%s-side refusal: true error %.4f = %.3f of B_u = %.4f; gap %.4f" % (side, err, ratio, res["B"][u], res["e_k"][u] - res["a_last"][u]))
    assert 0.5 <= ratio <= 1.0
    assert not res["cert"][u] and res["cert"][np.arange(U.shape[0]) != u].all()
    shares = res["terms"][u] / res["B"][u]
    assert sm.TERMS[int(np.argmax(shares))] == case["dominant"]
    bad = sc.model(case, drop_term=case["dominant"])
    assert bad["cert"][u]
    assert not np.array_equal(bad["top"][u], wi[u]) and victim not in bad["top"][u]
    # the other users' certified lists are the oracle's
    for j in range(1, U.shape[0]):
        assert np.array_equal(res["top"][j], wi[j])


def test_certified_lists_are_the_oracle_s():
    """The model's own soundness on a sweep: every certified user's k best candidates are the oracle's top k."""
    case, res = _sweep("b")
    _, wi = orc.score_topk(case["U"], None, case["V"], K)
    ok = res["cert"]
    assert ok.any() and np.array_equal(res["top"][ok], wi[ok])
