"""The margin rule of the screened route's fp16 pass, on a numpy model of one user's streaming list (no GPU).

The pass keeps K' = 28 candidates per user.  Without the rule a row is a candidate when its approximate score is above the list's
tail; with it, once the tail is an item, the threshold is max(tail, L[k-1] - M) with M > 2 B_u.  The model below is the kernel's
bookkeeping for one user -- the strict hit test against the threshold in the register, "cannot enter" under the key (score
descending, id ascending), a rated row entering at -1e9, the threshold recomputed by every insert -- and the certificate of stage 2
over the list it leaves.  For every drawn case it asserts what DESIGN proves:

* with T the list without the rule, A its tail, N the list with it and a_k the final k-th approximate score (equal in both):
  N = T whenever A >= a_k - 2 B; otherwise both calls certify;
* certified-ness is equal in every case, the exact top k of a certified call is the true one, and the clause stage 2 gained,
  e_k > (a_k - M) + B, holds whenever the old predicate does;
* every threshold the rule ever supplied lies strictly below a_k - 2 B;
* fl(a_k - M) < a_k - 2 B in exact arithmetic for |a_k| <= 2^12 B over magnitudes 2^-40 .. 2^40 (the float subtraction is safe).
"""
from fractions import Fraction

import numpy as np
import pytest

from oracle import screen_model as sm

KP = sm.KP
MASKED = np.float32(sm.MASKED)
NEG_INF = np.float32(-np.inf)
F32_MIN_NORMAL = np.float32(2.0 ** -126)


def margin_of(B):
    """M of screen_margin_kernel for a largest bound B (scale 1): 2 (1 + 2^-10) B rounded up to a float, never below 2^-126."""
    if not np.isfinite(B):
        return np.float32(np.inf)
    return np.maximum(sm.up_float(np.array([2.0 * (1.0 + 2.0 ** -10) * float(B)]))[0], F32_MIN_NORMAL).astype(np.float32)


def better(s1, i1, s2, i2):
    return s1 > s2 or (s1 == s2 and i1 < i2)


def tau_of(L, k, M, used):
    """The threshold of a list (dma_new_tau / the kernel's prologue).  ``used`` collects the values the rule supplied."""
    if len(L) < KP:
        return NEG_INF
    tail = L[KP - 1][0]
    t = tail if tail >= MASKED else NEG_INF
    if tail > MASKED and M is not None:
        m = np.float32(L[k - 1][0] - M)                  # the kernel's float subtraction
        if m > t:
            used.append(m)
            t = m
    return t


def stream(arrivals, k, M, seeds=()):
    """One user's list after ``arrivals`` = [(approximate score, id, rated)] in stream order.  M None: no rule."""
    L = sorted(seeds, key=lambda e: (-e[0], e[1]))[:KP]
    used = []
    tau = tau_of(L, k, M, used)
    for s, gi, rated in arrivals:
        if not s > tau:                                  # the hit test of the tile: strict
            continue
        if len(L) == KP and not better(max(s, MASKED), gi, *L[KP - 1]):
            continue                                     # cannot enter a full list
        e = (MASKED if rated else s, gi)
        p = sum(1 for x in L if better(x[0], x[1], e[0], e[1]))
        if p < KP:
            L.insert(p, e)
            del L[KP:]
            if len(L) == KP:
                tau = tau_of(L, k, M, used)
    return L, used


def certificate(L, exact, k, B, M):
    """(certified, the k best of the list by (exact descending, id ascending), the new clause) as stage 2 decides them."""
    if len(L) < KP or any(s <= MASKED for s, _ in L):
        return False, None, None
    order = sorted(L, key=lambda e: (-exact[e[1]], e[1]))
    e_k = exact[order[k - 1][1]]
    cert = e_k > float(L[KP - 1][0]) + B
    clause = True if M is None or not np.isfinite(M) else e_k > (float(L[k - 1][0]) - float(M)) + B
    return bool(cert), [gi for _, gi in order[:k]], bool(clause)


def check_case(arr, exact, k, B, seeds=(), cuts=1):
    """Runs one drawn case with and without the rule (``cuts`` item-range cuts of the stream, merged) and asserts the claims."""
    M = margin_of(B)
    assert float(M) > 2.0 * B

    def run(m):
        if cuts == 1:
            return stream(arr, k, m, seeds)
        out, used = list(seeds), []
        bounds = np.linspace(0, len(arr), cuts + 1).astype(int)
        for c in range(cuts):                            # every cut starts from the seeds and stores its own range's entries
            Lc, uc = stream(arr[bounds[c]:bounds[c + 1]], k, m, seeds)
            own = {gi for _, gi, _ in arr[bounds[c]:bounds[c + 1]]}
            out += [e for e in Lc if e[1] in own]
            used += uc
        return sorted(out, key=lambda e: (-e[0], e[1]))[:KP], used

    T, _ = run(None)
    N, used = run(M)
    off, _ = run(np.float32(np.inf))
    assert off == T                                      # M = +inf is the kernel without the rule
    full_T = len(T) == KP and T[KP - 1][0] > MASKED
    assert (len(N) == KP and N[KP - 1][0] > MASKED) == full_T
    cT, topT, _ = certificate(T, exact, k, B, None)
    cN, topN, clause = certificate(N, exact, k, B, M)
    assert cN == cT
    if not full_T:
        assert N == T and not used                       # a list whose tail never becomes an item is untouched
        return cN, N == T
    a_k, A = float(T[k - 1][0]), float(T[KP - 1][0])
    assert N[:k] == T[:k]                                # the k best always pass
    assert all(float(t) < a_k - 2.0 * B for t in used), (used, a_k, B)
    assert float(N[KP - 1][0]) <= A
    if A >= a_k - 2.0 * B:
        assert N == T
    else:
        assert cT and cN
    if cN:
        assert clause
        live = [gi for s, gi, rated in list(arr) + [(s, gi, False) for s, gi in seeds if s > MASKED] if not rated]
        truth = sorted(set(live), key=lambda gi: (-exact[gi], gi))[:k]
        assert topN == truth and topT == truth
    return cN, N == T


def draw(rng, n, kind, B, gap):
    """Approximate scores (float32) of n rows and exact scores within +-B of them.  ``gap``: how far below the 20 best the
    bulk of the rows starts, in units of B -- it decides on which side of a_k - 2 B the tail falls."""
    if kind == "random":
        a = rng.standard_normal(n)
    elif kind == "ties":
        a = rng.integers(-6, 7, n) / 4.0
    else:                                                # a head, then a bulk that starts `gap` bounds below it
        a = np.concatenate([1.0 + rng.random(24) * 0.01, 1.0 - gap * B - rng.random(n - 24) * 8.0 * B])
    a = a.astype(np.float32)
    exact = a.astype(np.float64) + rng.uniform(-B, B, n)
    return a, exact


ORDERS = ("random", "ascending", "descending", "best last", "zigzag")


def arrival_order(rng, a, order):
    n = len(a)
    idx = np.argsort(a, kind="stable")
    if order == "random":
        return rng.permutation(n)
    if order == "ascending":                             # every row enters: the adversary of a streaming top-K'
        return idx
    if order == "descending":
        return idx[::-1]
    if order == "best last":
        return np.concatenate([rng.permutation(idx[:-40]), idx[-40:]])
    return np.stack([idx[:n // 2], idx[::-1][:n // 2]], 1).ravel()


@pytest.mark.parametrize("k", [1, 20])
@pytest.mark.parametrize("kind", ["random", "ties", "gapped"])
def test_rule_leaves_results_and_counts(k, kind):
    rng = np.random.default_rng(1900 + k + len(kind))
    seen = {"equal": 0, "thinned": 0, "cert": 0, "uncert": 0}
    for trial in range(60):
        n = int(rng.integers(60, 400))
        # bounds from "certifies easily" to "never certifies"; gaps on both sides of 2 B and close to it
        B = float(rng.choice([1e-4, 1e-3, 3e-3, 2e-2, 0.2]))
        gap = float(rng.choice([0.5, 1.9, 2.0, 2.1, 3.0, 6.0]))
        a, exact = draw(rng, n, kind, B, gap)
        order = arrival_order(rng, a, ORDERS[trial % len(ORDERS)])
        rated = rng.random(n) < 0.05
        ids = rng.permutation(10 * n)[:n]                # ids unrelated to the arrival order
        ex = {int(ids[j]): float(exact[j]) for j in range(n)}
        arr = [(a[j], int(ids[j]), bool(rated[j])) for j in order]
        seeds = ()
        if trial % 3 == 1:                               # a full seed list (some of its rows rated: they sit at -1e9)
            arr, head = arr[KP:], arr[:KP]
            seeds = tuple((MASKED if r else s, gi) for s, gi, r in head)
            if trial % 2:                                # all its entries items
                seeds = tuple((s, gi) for s, gi, r in head)
                arr = [(s, gi, False) if gi in {g for _, g, _ in head} else (s, gi, r) for s, gi, r in arr]
            for s, gi, r in head:
                if r and trial % 2 == 0:
                    ex.pop(gi)                           # (a rated row is nobody's answer)
        cert, same = check_case(arr, ex, k, B, seeds, cuts=2 if trial % 4 == 3 else 1)
        seen["cert" if cert else "uncert"] += 1
        seen["equal" if same else "thinned"] += 1
    # the gapped draws reach both sides of every claim (k = 1: the best of a head of 24 always certifies)
    assert min(seen.values()) > 0 or kind != "gapped" or k == 1, seen


def test_short_and_masked_lists():
    rng = np.random.default_rng(7)
    B = 1e-3
    for n_live in (11, 27, 28, 29):                      # fewer than K' live rows: the list never fills, the rule never engages
        a, exact = draw(rng, n_live, "random", B, 0)
        ex = {j: float(exact[j]) for j in range(n_live)}
        cert, same = check_case([(a[j], j, False) for j in rng.permutation(n_live)], ex, 20, B)
        assert same or n_live == 29
        assert n_live >= 28 or not cert
    # seeds that end in masked entries: thresholds stay -inf / -1e9 until items push them out; then the rule engages
    a, exact = draw(rng, 200, "gapped", B, 6.0)
    ex = {j + 100: float(exact[j]) for j in range(200)}
    seeds = tuple((np.float32(0.5 - j / 64.0), j) for j in range(20)) + tuple((MASKED, 20 + j) for j in range(8))
    ex.update({j: 0.5 - j / 64.0 for j in range(20)})
    check_case([(a[j], j + 100, False) for j in range(200)], ex, 20, B, seeds)
    check_case([(a[j], j + 100, False) for j in range(200)], ex, 1, B, seeds, cuts=2)


def test_nonfinite_bound_switches_the_rule_off():
    assert margin_of(np.inf) == np.inf and margin_of(np.nan) == np.inf
    used = []
    L = [(np.float32(1.0 - j / 64.0), j) for j in range(KP)]
    assert tau_of(L, 20, np.float32(np.inf), used) == L[KP - 1][0] and not used


def test_float_subtraction_is_safe():
    """fl(a_k - M) < a_k - 2 B exactly, for every |a_k| <= 2^12 B (B_u holds 2^-12 |u^| N^ >= 2^-12 |a|), magnitudes 2^-40 .. 2^40."""
    rng = np.random.default_rng(11)
    for e in list(range(-40, 41, 4)) + [-39, 39]:
        for _ in range(200):
            B = float(2.0 ** e * rng.uniform(1.0, 2.0))
            ratio = float(rng.choice([0.0, 1e-3, 1.0, 37.0, 1000.0, 4095.0, 4096.0]))
            a_k = np.float32(ratio * B * rng.choice([-1.0, 1.0]))
            if abs(float(a_k)) > 4096.0 * B:             # (the rounding of a_k itself)
                a_k = np.float32(np.nextafter(a_k, np.float32(0)))
            M = margin_of(B)
            t = np.float32(a_k - M)
            assert Fraction(float(M)) > 2 * Fraction(B)
            assert Fraction(float(t)) < Fraction(float(a_k)) - 2 * Fraction(B), (e, a_k, M, B)
    # an underflowing bound: M is the smallest normal float, never 0
    assert margin_of(1e-60) == F32_MIN_NORMAL and np.float32(np.float32(0) - margin_of(1e-60)) < 0
