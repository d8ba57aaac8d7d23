"""Inputs on which the screened ranking's certificate is decided by the size of its bound (tests/test_screen_certificate*.py).

Every table entry sits on a grid chosen so that (oracle/screen_model.py asserts the first, the CPU test the second)
* every sum of fp16 x fp16 products is exact in fp32 in any order: the approximate score is the exact value of u^.v^
  whatever the MFMA shape, the tile order, the cuts or the seeded prefix;
* the fmaf chain of the sweeps is exact as well.

A sweep.  Every user is u = (1, 2^-8, knobs ..., 0 ...): the same two scoring components, plus "knob" components in
dimensions where every item is zero -- they change |u|, |u^| and |u - u^|, hence B_u, and no score.  So all users rank the
items alike: 20 planted items score 1 + (19 - r) 2^-6 (r = 0 .. 19), eight score 1 - g + (27 - r) 2^-18 (r = 20 .. 27; g a
multiple of 2^-18), the background at most 0.51.  e_k - A_last is g for every user (k = 20), B_u grows with the user's
index and crosses g once: the call's uncertified count is the position of the crossing, which pins B_u although the
library reports only a count.  "Ballast" rows orthogonal to every user set the item maxima: n1, n2 (representable, norms
3 and 2.5: N and N^), r1, r2 (off the fp16 grid: R).  Dimensions: 0, 1 scores; 2 .. 7 knobs; 8 .. 15 ballast;
16 .. 127 background only.

    a  everything representable: B_u = (g_d N + g' N^) |u|, knob (512 + j) 2^-10
    b  a with the rows r1, r2: the |u| R term is about 45 % of B_u
    c  a fixed knob 0.75 plus a float32 residual below half an fp16 ulp that grows with j: |u - u^| N^ is 13 .. 40 %
    d  a user of 2^24 sets the user scale, so every component below 2^-4 is flushed: u = (1, 2^-8, f_j) has u^ = (1, 0, 0),
       |u^| = 1 < |u| by 4.5e-4 |u| (15 steps of the sweep) and |u - u^| N^ is 99 % of B_u.  Here the approximate score is
       v^_0 alone and the eight lower plants tie at 1 - G (G = 3/32): f_j is centred so that B_u crosses G.
"""
import numpy as np

from oracle import screen_model as sm

K = 20
N_PLANTS = 29                 # 28 and one more that enters a list when a rated list removes one of them
DELTA = 2.0 ** -18
D_GAP = 3.0 / 32.0            # sweep d: e_k - A_last
D_STEP = 3.0e-5               # sweep d: relative step of f_j (and so of B_u) per user
OFF = np.float32(1.0 + 0.45 * 2.0 ** -10)       # rounds to 1.0 in fp16: residual 0.45 * 2^-10 per component


def _users(kind, n_users, f_mid=None):
    U = np.zeros((n_users, 128), np.float32)
    U[:, 0] = 1.0
    U[:, 1] = 2.0 ** -8
    j = np.arange(n_users, dtype=np.float64) * (400.0 / n_users)        # position on the 400-user sweep
    if kind in "ab":
        U[:, 2] = (512.0 + np.floor(j)) * 2.0 ** -10
    elif kind == "c":
        U[:, 2] = (0.75 + (0.1 + 0.3 * j / 400.0) * 2.0 ** -11).astype(np.float32)
    else:
        U[:, 2] = (f_mid * (1.0 + (j - 200.0) * D_STEP)).astype(np.float32)
        U[-1] = 0.0
        U[-1, 0] = 2.0 ** 24                                           # sets the scale; ranks like everybody, certified
    return U


def _items(kind, n_items, g, plant_ids, ballast_ids, seed):
    rng = np.random.default_rng(seed)
    V = np.zeros((n_items, 128), np.float32)
    V[:, 0] = rng.integers(-32, 33, n_items) * 2.0 ** -6               # background: score <= 0.5 + 2^-9
    V[:, 1] = rng.integers(-32, 33, n_items) * 2.0 ** -6
    V[:, 16:] = rng.integers(-4, 5, (n_items, 112)) * 2.0 ** -6
    V[plant_ids] = 0.0
    r = np.arange(K)
    V[plant_ids[:K], 0] = 1.0 + (K - 1 - r) * 2.0 ** -6
    lo = np.arange(K, N_PLANTS)
    if kind == "d":
        V[plant_ids[K:], 0] = 1.0 - D_GAP
        v1 = 1.0 + (N_PLANTS - lo) * 2.0 ** -10                         # (flushed on the user side: only the exact order sees it)
    else:
        V[plant_ids[K:], 0] = 1.0 - 2.0 ** -7
        steps = np.where(lo < 28, 27 - lo, -6)                          # the 29th: 1 - g - 6 * 2^-18
        v1 = 2.0 ** 8 * (2.0 ** -7 - g + steps * DELTA)
        assert ((v1 >= 1.0) & (v1 < 2.0)).all() and (v1 * 1024 == np.round(v1 * 1024)).all(), (g, v1)
    V[plant_ids[K:], 1] = v1
    for name, row in ballast_ids.items():
        V[row] = 0.0
        if name == "n1":
            V[row, 8] = 3.0
        elif name == "n2":
            V[row, 9] = 2.5
        elif name == "r1":
            V[row, 10:12] = OFF
        elif name == "r2":
            V[row, 12] = OFF
    return V


def sweep(kind, n_users=400, n_items=5003, mask=None, rated=False, plant_ids=None, ballast_ids=None, item_base=0, seed=7):
    """One sweep as a dict: U, V, bitmap_ids, rated (global ids), plant_ids (local, rank order), item_base, g, kind.
    ``mask``: None, or "R" / "N": a bitmap masks r1 / n1 (and a fifth of the background), so that R comes from r2 (sweep
    b; 0 in the others, which then hold a masked r1) or N and N^ from n2.  ``rated``: user j rates the plant of rank
    21 + j % 8, so the 29th plant ends every list.  The gap g is the smallest multiple of 2^-18 that is no less than the
    middle user's B_u under the masks of the case (sweep d: f_j is centred instead)."""
    rng = np.random.default_rng(seed + 1)
    names = ["n1", "n2"] + (["r1", "r2"] if kind == "b" else ["r1"] if mask == "R" else [])
    if plant_ids is None or ballast_ids is None:
        pool = rng.permutation(n_items)
        plant_ids = pool[:N_PLANTS] if plant_ids is None else np.asarray(plant_ids)
        if ballast_ids is None:
            ballast_ids = np.setdiff1d(pool[N_PLANTS:N_PLANTS + 64], plant_ids)[:4]
    plant_ids = np.asarray(plant_ids, np.int64)
    ballast = dict(zip(names, [int(q) for q in ballast_ids]))
    special = np.concatenate([plant_ids, np.fromiter(ballast.values(), np.int64)])
    assert len(np.unique(special)) == len(special)
    bitmap_ids = None
    if mask is not None:
        cold = np.setdiff1d(np.where(rng.random(n_items) < 0.2)[0], special)
        bitmap_ids = np.union1d(cold, [ballast["r1" if mask == "R" else "n1"]]) + item_base
    live = np.ones(n_items, bool)
    if bitmap_ids is not None:
        live[bitmap_ids - item_base] = False
    sel = np.arange(n_users)
    V = _items(kind, n_items, 2.0 ** -9, plant_ids, ballast, seed)
    if kind == "d":
        lo, hi = 0.01, 0.06                                # B_u of the middle user is monotone in f: centre it on the gap
        for _ in range(60):
            f_mid = 0.5 * (lo + hi)
            B = sm.stage0(_users(kind, n_users, f_mid), V, sel, live)["B"][n_users // 2]
            lo, hi = (f_mid, hi) if B < D_GAP else (lo, f_mid)
        U, g = _users(kind, n_users, f_mid), D_GAP
    else:
        U = _users(kind, n_users)
        B = sm.stage0(U, V, sel, live)["B"][n_users // 2]
        g = float(np.ceil(B / DELTA) * DELTA)
        V = _items(kind, n_items, g, plant_ids, ballast, seed)
    rl = [np.array([plant_ids[K + j % 8] + item_base]) for j in range(n_users)] if rated else None
    return dict(kind=kind, U=U, V=V, bitmap_ids=bitmap_ids, rated=rl, plant_ids=plant_ids, ballast=ballast,
                item_base=item_base, g=g)


def model(case, k=K, users=None, drop_term=None):
    return sm.certify(case["U"], case["V"], k, users=users, bitmap_ids=case["bitmap_ids"], rated=case["rated"],
                      item_base=case["item_base"], drop_term=drop_term)


# ---- the two refusal cases: inputs on which only a sound bound gives the right answer
def _refusal_background(rng, n_items):
    V = np.zeros((n_items, 128), np.float32)
    V[:, :64] = rng.integers(0, 9, (n_items, 64)) * 2.0 ** -4          # entries 0 .. 0.5 on dims 0 .. 63
    return V


def refusal_item_side(n_items=3001, seed=11):
    """User 0 is 1 in all 128 dimensions.  The victim row is 1 + 0.49 * 2^-10 everywhere: it rounds to 1.0, its residual is
    parallel to u (Cauchy-Schwarz is tight), its exact score 128 + 62.7 ulps (ulp = 2^-10) is the best and its approximate score
    128 is the 29th: 28 representable decoys lie between, twenty at +62 .. +52.5 ulps (j components raised by an ulp, every
    other one with a component at 1 - 2^-11) and eight at +9 .. +2.  Users 1 .. 4 are unit vectors of dimension 0, which rank 20
    rows of v_0 = 3 - t / 64 first: they certify."""
    rng = np.random.default_rng(seed)
    V = _refusal_background(rng, n_items)
    V[:, 64:] = V[:, :64]                                               # background scores <= 64 against the user of ones
    ids = rng.permutation(n_items)[:49]
    victim, decoys, pads = int(ids[0]), ids[1:29], ids[29:49]
    V[victim] = np.float32(1.0 + 0.49 * 2.0 ** -10)
    half_ulps = np.concatenate([124 - np.arange(20), 2 * (9 - np.arange(8))])      # 62 .. 52.5 and 9 .. 2 ulps
    for row, h in zip(decoys, half_ulps):
        V[row] = 1.0
        V[row, 1:1 + (h + 1) // 2] = 1.0 + 2.0 ** -10
        if h % 2:
            V[row, 127] = 1.0 - 2.0 ** -11
    V[pads] = 0.0
    V[pads, 0] = 3.0 - np.arange(20) / 64.0
    U = np.zeros((5, 128), np.float32)
    U[0] = 1.0
    U[1:, 0] = 1.0
    return dict(kind="item-side", U=U, V=V, bitmap_ids=None, rated=None, item_base=0, victim=victim, victim_user=0,
                dominant="R")


def refusal_user_side(n_items=3001, seed=12):
    """The mirror image.  User 1 (2^24 in dimension 0) sets the user scale, so components below 2^-4 are flushed.  User 0 is 1 on
    dimensions 0 .. 63 and 0.05 on 64 .. 127: u^ keeps the first half only, and the residual is parallel to the victim row, 1 on
    dimensions 64 .. 127 and 0 elsewhere (representable, norm 8 = N^): approximate score 0, exact score 3.2, the best.  The
    decoys hold one component x on dimension 0: twenty at 3 .. 2.7, eight at 0.5 .. 0.39; the background scores at most 1/16.  Users 1 .. 4 (the scale setter and unit vectors of dimension 0) rank the decoys alike and certify."""
    rng = np.random.default_rng(seed)
    V = np.zeros((n_items, 128), np.float32)
    V[:, 0] = rng.integers(-16, 5, n_items) * 2.0 ** -6                 # <= 1/16
    V[:, 1:32] = rng.integers(-8, 9, (n_items, 31)) * 2.0 ** -6
    V[:, 32:63] = -V[:, 1:32]                                           # dims 1 .. 63 sum to zero: user 0 scores v_0 as well
    ids = rng.permutation(n_items)[:29]
    victim, decoys = int(ids[0]), ids[1:29]
    V[victim] = 0.0
    V[victim, 64:] = 1.0
    V[decoys] = 0.0
    V[decoys, 0] = np.concatenate([3.0 - np.arange(20) / 64.0, 0.5 - np.arange(8) / 64.0])
    U = np.zeros((5, 128), np.float32)
    U[0, :64] = 1.0
    U[0, 64:] = np.float32(0.05)
    U[1, 0] = 2.0 ** 24
    U[2:, 0] = 1.0
    return dict(kind="user-side", U=U, V=V, bitmap_ids=None, rated=None, item_base=0, victim=victim, victim_user=0,
                dominant="resid")
