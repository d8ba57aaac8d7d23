"""SCREEN MODEL -- TEST INFRASTRUCTURE ONLY (numpy / fp64 restatement of stages 0 and 2 of the screened ranking).

Written from DESIGN.md 4.1.5 and the header comment of ``coldrec_amd/csrc/score_screen.hip``; nothing under
``coldrec_amd/`` may import it.  It answers one question per user of a screened ``score_topk`` call: does the
certificate ``e_k > A_last + B_u`` hold, with

    B_u = |u| R + |u - u^| N^ + g_d |u| N + g' |u^| N^          (terms 1 .. 4 below)

so that the count of users it refuses can be compared with ``ops.score_topk_uncertified()``.

The model does not imitate the fp16 MFMA pass.  It takes the approximate score to be the exact value of u^.v^ and
*asserts* that its inputs make every fp32 accumulation order return just that (``assert_products_exact``): then the
approximate score does not depend on the MFMA shape, the tile order, the cuts or the seeded prefix, and the only thing
left between the model and the kernel is the fp64 evaluation of one formula (operation order and contraction: a few
2^-53; the tests keep a guard band of 1e-4 B_u).  The exact score is the C oracle's fmaf chain.

The scale.  One power-of-two scale per table, exponent 15 - (frexp exponent of the largest finite |x|).  The user
table's maximum is taken over the selected rows; the item table's over every row of the shard, masked or not, as
DESIGN.md 4.1.5 and ``screen_maxabs_kernel`` have it (the scale only has to be a power of two for the bound to hold).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

from oracle import oracle_np as orc

KP = 28                                   # K': candidates per user
D = 128
GAMMA_D = D * 2.0 ** -24 / (1.0 - D * 2.0 ** -24)
GAMMA_P = 2.0 ** -12
TERMS = ("R", "resid", "gamma_d", "gamma_p")      # |u| R, |u - u^| N^, g_d |u| N, g' |u^| N^
MASKED = -1.0e9


def scale_exp(x: np.ndarray) -> int:
    """Exponent e of a table's scale 2^e: (largest finite |x|) * 2^e < 2^15; 0 for a table without a positive finite entry."""
    ax = np.abs(np.asarray(x, np.float32))
    ax = ax[np.isfinite(ax)]
    m = float(ax.max()) if ax.size else 0.0
    if not m > 0.0:
        return 0
    return 15 - int(np.frexp(np.float32(m))[1])


def f16_copy(x: np.ndarray, e: int) -> np.ndarray:
    """The fp16 copy of x * 2^e (round to nearest even, |.| < 2^-14 flushed to zero), scaled back; float64, exact."""
    with np.errstate(over="ignore", invalid="ignore"):
        y = np.ldexp(np.asarray(x, np.float32), e).astype(np.float32)
        h = y.astype(np.float16)
    h[np.abs(h.astype(np.float32)) < np.float32(2.0 ** -14)] = np.float16(0.0)
    return np.ldexp(h.astype(np.float64), -e)


def up_float(x: np.ndarray) -> np.ndarray:
    """float32 >= x for x >= 0 (elementwise); +inf for NaN or beyond the float range."""
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        f = x.astype(np.float32)
        low = f.astype(np.float64) < x
        f = np.where(low, np.nextafter(f, np.float32(np.inf)), f).astype(np.float32)
    f[~(x <= 3.0e38)] = np.float32(np.inf)
    return f


def up_norm(s: np.ndarray) -> np.ndarray:
    with np.errstate(invalid="ignore"):
        return up_float(np.sqrt(np.asarray(s, np.float64)) * (1.0 + 2.0 ** -30))


def row_norms(x: np.ndarray, xh: np.ndarray):
    """Per row (|x|, |x^|, |x - x^|): fp64 sums, sqrt * (1 + 2^-30), rounded up to float32; a non-finite row gives +inf."""
    x64 = np.asarray(x, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sxx = (x64 * x64).sum(1)
        shh = (xh * xh).sum(1)
        sdd = ((x64 - xh) ** 2).sum(1)
    bad = np.isnan(sxx) | np.isnan(sdd)
    out = [up_norm(sxx), up_norm(shh), up_norm(sdd)]
    for o in out:
        o[bad] = np.float32(np.inf)
    return out


def _quantum(x: np.ndarray) -> np.ndarray:
    """The largest power of two that divides each finite non-zero float64 of x (inf for zeros)."""
    m, ex = np.frexp(x)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)
    low = mi & -mi
    q = np.ldexp(low.astype(np.float64), ex - 53)
    return np.where(x == 0.0, np.inf, q)


def assert_products_exact(uh: np.ndarray, vh: np.ndarray) -> None:
    """Every sum of the products u^[j, c] * v^[i, c] over c, in any order and with any partial sums, is exact in fp32:
    all of user j's products are multiples of a power of two q_j and the sum of their magnitudes stays below 2^24 q_j
    (sufficient, evaluated per user against the per-column extremes of the item table)."""
    vq = _quantum(vh).min(0)                              # per column: what divides every entry (inf: the column is zero)
    vmax = np.abs(vh).max(0)
    uq = _quantum(uh)
    live = (uh != 0.0) & np.isfinite(vq)[None, :]
    with np.errstate(invalid="ignore"):
        q = np.where(live, uq * np.where(np.isfinite(vq), vq, 1.0)[None, :], np.inf).min(1)
    total = (np.abs(uh) * vmax[None, :]).sum(1)
    ok = ~np.isfinite(q) | (total < q * 2.0 ** 24)
    assert ok.all(), "approximate scores are not exact in fp32 for users %s" % np.where(~ok)[0][:8]


def bound(un, uhn, udn, R, N, Nh, drop_term: Optional[str] = None):
    """(B_u, its four terms) in fp64 from the float32 norms, as screen_certify_kernel evaluates it."""
    un, uhn, udn = (np.asarray(a, np.float64) for a in (un, uhn, udn))
    R, N, Nh = float(R), float(N), float(Nh)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.stack([un * R, udn * Nh, GAMMA_D * un * N, GAMMA_P * uhn * Nh], 1)
        if drop_term is not None:
            t[:, TERMS.index(drop_term)] = 0.0
        B = (t[:, 0] + t[:, 1] + t[:, 2] + t[:, 3] + 2.0 ** -126) * (1.0 + 2.0 ** -20)
    return B, t


def stage0(U, V, sel, live, drop_term: Optional[str] = None) -> dict:
    """Stage 0 of a call over the user rows ``sel`` and an item shard whose unmasked rows are ``live`` (bool per row):
    scales, fp16 copies (masked rows zero), norms, the item maxima R, N, N^ over the unmasked rows, and B_u."""
    Us = U[sel]
    e_i, e_u = scale_exp(V), scale_exp(Us)
    vh = f16_copy(V, e_i)
    vh[~live] = 0.0                                        # (masked rows are zeros in the stream or absent from it)
    uh = f16_copy(Us, e_u)
    vn, vhn, vdn = row_norms(V[live], vh[live])
    R = float(vdn.max()) if vdn.size else 0.0
    N = float(vn.max()) if vn.size else 0.0
    Nh = float(vhn.max()) if vhn.size else 0.0
    un, uhn, udn = row_norms(Us, uh)
    B, terms = bound(un, uhn, udn, R, N, Nh, drop_term)
    return dict(uh=uh, vh=vh, B=B, terms=terms, R=R, N=N, Nh=Nh, e_items=e_i, e_users=e_u, un=un, uhn=uhn, udn=udn)


def certify(U, V, k: int, users=None, bitmap_ids=None, rated: Optional[Sequence] = None, item_base: int = 0,
            drop_term: Optional[str] = None, check_exact: bool = True) -> dict:
    """The certificate of every user of the call ``score_topk(U, users, V, k, rated, bitmap, item_base)``.

    ``bitmap_ids`` / ``rated[j]``: global item ids (as the library takes them).  ``drop_term`` (one of TERMS) evaluates
    the predicate with that term of B_u deleted -- the CPU test's way to show what a wrong bound would do.
    Returns arrays over the users: ``cert`` (bool), ``B``, ``terms`` (n, 4), ``e_k``, ``a_last``, ``margin`` =
    e_k - (A_last + B_u), ``cand`` (n, 28 global ids, approximate order; -1 where the list is short), ``top``
    (n, k: the k best candidates by (exact desc, id asc)), and the scalars ``R``, ``N``, ``Nh``, ``e_items``, ``e_users``."""
    U = np.ascontiguousarray(U, np.float32)
    V = np.ascontiguousarray(V, np.float32)
    assert U.shape[1] == D and V.shape[1] == D
    sel = np.arange(U.shape[0]) if users is None else np.asarray(users, np.int64)
    Us = U[sel]
    n, n_items = Us.shape[0], V.shape[0]
    live = np.ones(n_items, bool)
    if bitmap_ids is not None and len(bitmap_ids):
        loc = np.asarray(bitmap_ids, np.int64) - item_base
        live[loc[(loc >= 0) & (loc < n_items)]] = False

    # ---- stage 0: scales, fp16 copies, norms, item maxima over the unmasked rows
    st0 = stage0(U, V, sel, live, drop_term)
    uh, vh, B, terms = st0["uh"], st0["vh"], st0["B"], st0["terms"]
    if check_exact:
        assert_products_exact(uh, vh[live])

    # ---- stage 1 (its result, not its code): top K' by (approximate desc, id asc) over the unmasked, unrated items
    cand = np.full((n, KP), -1, np.int64)
    a_cand = np.full((n, KP), -np.inf)
    vht = np.ascontiguousarray(vh.T)
    for j0 in range(0, n, 64):
        A = uh[j0:j0 + 64] @ vht
        A[:, ~live] = -np.inf
        for j in range(j0, min(j0 + 64, n)):
            a = A[j - j0]
            if rated is not None and rated[j] is not None and len(rated[j]):
                loc = np.asarray(rated[j], np.int64) - item_base
                a[loc[(loc >= 0) & (loc < n_items)]] = -np.inf
            if n_items > KP:
                thr = np.partition(a, n_items - KP)[n_items - KP]
                pool = np.where(a >= thr)[0]
            else:
                pool = np.arange(n_items)
            pool = pool[a[pool] > -np.inf]
            order = pool[np.argsort(-a[pool], kind="stable")][:KP]        # pool ascending: ties keep id order
            cand[j, :len(order)] = order
            a_cand[j, :len(order)] = a[order]

    # ---- stage 2: exact chain over the candidates, the predicate
    full = (cand >= 0).all(1)
    union = np.unique(cand[cand >= 0])
    S = orc.scores_dense(U, sel, V[union]).astype(np.float64) if union.size else np.zeros((n, 0))
    pos = np.searchsorted(union, np.where(cand >= 0, cand, union[0] if union.size else 0))
    e = np.where(cand >= 0, np.take_along_axis(S, pos, 1), -np.inf)
    cert = np.zeros(n, bool)
    e_k = np.full(n, np.nan)
    margin = np.full(n, np.nan)
    top = np.full((n, k), -1, np.int64)
    for j in range(n):
        if not full[j]:
            continue
        order = np.lexsort((cand[j], -e[j]))
        top[j] = cand[j, order[:k]] + item_base
        e_k[j] = e[j, order[k - 1]]
        if not (np.isfinite(e[j]).all() and np.isfinite(a_cand[j]).all()):
            continue
        thr = a_cand[j, KP - 1] + B[j]
        thr += abs(thr) * 2.0 ** -50
        margin[j] = e_k[j] - (a_cand[j, KP - 1] + B[j])
        cert[j] = bool(e_k[j] > thr and e_k[j] > MASKED)
    return dict(cert=cert, B=B, terms=terms, e_k=e_k, a_last=a_cand[:, KP - 1], margin=margin,
                cand=np.where(cand >= 0, cand + item_base, -1), a_cand=a_cand, e_cand=e, top=top,
                **{q: st0[q] for q in ("R", "N", "Nh", "e_items", "e_users", "un", "uhn", "udn")})


def guarded_count(res: dict, guard: float = 1.0e-4):
    """(uncertified users outside the guard band, users inside it): a user is inside when |margin| < guard * B_u."""
    with np.errstate(invalid="ignore"):
        inside = np.abs(res["margin"]) < guard * res["B"]
    return int((~res["cert"] & ~inside).sum()), int(inside.sum())
