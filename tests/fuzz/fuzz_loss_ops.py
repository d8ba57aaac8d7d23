#!/usr/bin/env python3
"""Randomised parity fuzzing of seven fused loss kernels (csrc/clcrec.hip, csrc/ccfcrec.hip, csrc/aldi.hip,
csrc/infonce.hip, csrc/gar.hip, csrc/mtpr.hip, csrc/vbpr.hip) against their float64 restatements
(tests/clcrec_restate.py, tests/ccfcrec_restate.py, tests/aldi_restate.py, tests/infonce_restate.py, and the three named
below).

CLCRec, CCFCRec, ALDI, per case: a width from every multiple of 4 in [4, 256], small B, G, P, N and S (now and then a batch long enough for an
owner to split into chunks), an id pattern per id tensor from {uniform, a few hot ids, one owner}, a scale per table from
{0.05, 0.3, 1.5} and temperatures / coefficients the trainers accept.  Then
  * the kernel against the float64 restatement.  The bar of a case is 8x the distance of the float32 restatement from the
    float64 one at that same case, computed here on the CPU, and no lower than the fixed bar of the kernel's test file
    (tests/test_clcrec_gpu.py 1e-5 / 1e-4, tests/test_ccfcrec_gpu.py LOSS_BAR / GRAD_BAR, tests/test_aldi_gpu.py the same).
    Loss terms: relative error, a term's magnitude floored at 1e-6 of the total (a term that far below the total is
    rounding noise in any float32 evaluation; ALDI's, as in its file, over the total); gradients: error over the table's
    maximum; a gradient the restatement leaves all zero must be all zero;
  * a second, identical call: every output bit-equal.
InfoNCE (kind ``infonce``), per case: a width from every multiple of 4 in [4, 256]; N mostly in [1, 700] with extra weight
on 32 k - 1, 32 k, 32 k + 1 and 128 k +- 1, one case in ten in [1000, 2100]; tau from {0.05, 0.2, 1.0}; b_cos on or off
(rows of length ~scale then, at most sqrt(10 tau)); a scale from the same three; a share of near-duplicate rows
v2 = v1 + 2 % noise from {0, 1/4, all}, the other rows augmented (v1 + 70 % noise) or independent; now and then a zero
row; a mode from {the whole view, row ids, row ids with a device count n_dev < n_max, row ids with scale + accumulate
on pre-filled tables}.  Row ids are permutations (the op wants them unique).  Then
  * the kernel against the float64 restatement: the loss's relative error within max(8x the float32 restatement's, 1e-5),
    no absolute floor; each gradient row by row, rho = max over rows of max|row error| / max|reference row|, within
    max(8x the float32 restatement's rho, 1e-4); a row the restatement leaves all zero must be all zero;
  * a second, identical call bit-equal; every table row outside the batch untouched; scale (a power of two) + accumulate
    equal to pre + scale * g bit for bit.
GAR, MTPR, VBPR (kinds ``gar``, ``mtpr``, ``vbpr``: csrc/gar.hip, csrc/mtpr.hip, csrc/vbpr.hip, which end in loss_common.h's
owner pass; tests/gar_restate.py, tests/mtpr_restate.py, tests/vbpr_restate.py), per case: a width from every multiple of
4 in [4, 256] (MTPR: [4, 128], its kernel's range; its tables are d and 2 d wide); B in [1, 100] and, in about one case in
seven, B in [300, 700] with a ``hot`` or ``one`` pattern on every id tensor, so that owners split into chunks of 256; an id
pattern per id tensor and a scale per table from the same sets (GAR: raw, G = tanh of a table; MTPR: its restatement's
sizes times the scale; VBPR: rows sized so that a dot product is of order 4 x the two scales at every width); a mode
(cold user or cold item; VBPR in item mode with or without h_adv); alpha, beta from {0, .., 1}, wd1 from {0, 0.01, 0.05},
lmd from {0, 0.7, 1}; for GAR reg from {0, 1e-4, 1e-2, 1, B}.  Judged as the others, over the total as ALDI: against the
float64 restatement with the case's bar 8x the float32 restatement's distance and no lower than the kernel file's fixed
bars (LOSS_BAR / GRAD_BAR of tests/test_gar_gpu.py, tests/test_mtpr_gpu.py, tests/test_vbpr_gpu.py), every gradient the call
returns (VBPR's grad_hsum among them; none where there is no h_adv); a second, identical call bit-equal.
On a mismatch the seed and the drawn parameters are printed and the exit status is 1.  Without --only every case draws its
kind from all seven; with it, from the kinds named, in the order named.

    python tests/fuzz/fuzz_loss_ops.py --cases 200 [--seed 0] [--only clcrec,ccfcrec,aldi,infonce,gar,mtpr,vbpr]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from coldrec_amd import ops  # noqa: E402
from tests import aldi_restate, ccfcrec_restate, clcrec_restate, gar_restate, infonce_restate  # noqa: E402
from tests import mtpr_restate, vbpr_restate  # noqa: E402
from tests import test_aldi_gpu as ald  # noqa: E402
from tests import test_ccfcrec_gpu as ccf  # noqa: E402
from tests import test_gar_gpu as gar  # noqa: E402
from tests import test_mtpr_gpu as mtpr  # noqa: E402
from tests import test_vbpr_gpu as vbpr  # noqa: E402

DEV = torch.device("cuda:0")
SCALES = [0.05, 0.3, 1.5]
PATTERNS = ["uniform", "hot", "one"]
SEED = None


def fail(what, **kw):
    print("MISMATCH", what, "seed", SEED, kw, flush=True)
    sys.exit(1)


def draw_ids(rng, n, shape, pattern):
    """int64 ids in [0, n): uniform, four in five on three hot ids, or one id everywhere."""
    size = int(np.prod(shape))
    ids = rng.integers(0, n, size)
    if pattern == "hot":
        hot = rng.integers(0, n, 3)
        ids = np.where(rng.random(size) < 0.8, hot[rng.integers(0, 3, size)], ids)
    elif pattern == "one":
        ids = np.full(size, int(rng.integers(0, n)))
    return torch.from_numpy(ids.astype(np.int64).reshape(shape))


def table(rng, rows, d, scale):
    return torch.from_numpy((rng.standard_normal((rows, d)) * scale).astype(np.float32))


def distances(got, want, over_total=False):
    """(worst loss-term error, worst gradient error / maximum) of (terms, g1, g2, ...) numpy tuples; the last term is the
    total.  A gradient whose reference is all zero counts with its own largest entry; one that is None on both sides is
    skipped."""
    terms, ref = np.asarray(got[0], np.float64), np.asarray(want[0], np.float64)
    total = abs(ref[-1])
    den = total if over_total else np.maximum(np.abs(ref), 1e-6 * total)
    rel = float((np.abs(terms - ref) / den).max())
    errs = []
    for g, w in zip(got[1:], want[1:]):
        if w is None:
            assert g is None
            continue
        g = np.asarray(g, np.float64)
        top = np.abs(w).max()
        errs.append(float(np.abs(g - w).max() / top) if top > 0 else float(np.abs(g).max()))
    return rel, max(errs)


def judge(kind, params, fused, want, f32, fixed, over_total=False):
    """``fused()`` -> (loss, g1, g2, ...) device tensors, any number of gradients, a None where the call has none (the
    restatement must have None there too); called twice."""
    a, b = fused(), fused()
    torch.cuda.synchronize()
    if not all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b)):
        fail(kind + ": two identical calls differ in their bits", **params)
    got = tuple(None if t is None else t.cpu().numpy() for t in a)
    if len(got) != len(want) or any((g is None) != (w is None) for g, w in zip(got, want)):
        fail(kind + ": the call and the restatement return different gradients", **params)
    if not all(np.isfinite(t).all() for t in got if t is not None):
        fail(kind + ": output not finite", **params)
    ref_rel, ref_err = distances(f32, want, over_total)
    bars = (max(8 * ref_rel, fixed[0]), max(8 * ref_err, fixed[1]))
    rel, err = distances(got, want, over_total)
    for g, w in zip(got[1:], want[1:]):
        if w is None:
            continue
        zero = (w == 0).all(1)
        if g[zero].any():
            fail(kind + ": gradient not zero where the restatement's row is", **params)
    if not (rel <= bars[0] and err <= bars[1]):
        fail(kind + " against the float64 restatement", loss=rel, grad=err, bars=bars, float32=(ref_rel, ref_err), **params)


def case_clcrec(rng):
    d = 4 * int(rng.integers(1, 65))
    B, G = int(rng.integers(1, 41)), int(rng.integers(1, 41))
    if rng.random() < 0.15:
        B, G = int(rng.integers(60, 140)), int(rng.integers(1, 4))               # a user with more than 64 records
    nu, ni = int(rng.integers(1, 30)), int(rng.integers(1, 60))
    su, sv, sf = (float(rng.choice(SCALES)) for _ in range(3))
    pu, pi = str(rng.choice(PATTERNS)), str(rng.choice(PATTERNS))
    T, lam = float(rng.choice([0.1, 0.5, 2.0])), float(rng.choice([0.0, 0.1, 0.5, 1.0]))
    reg, ns = float(rng.choice([0.0, 1e-4, 1e-2])), float(rng.choice([0.0, 0.5, 1.0]))
    params = dict(d=d, B=B, G=G, nu=nu, ni=ni, scales=(su, sv, sf), ids=(pu, pi), T=T, lam=lam, reg=reg, num_sample=ns)
    U, V = table(rng, nu, d, su), table(rng, ni, d, sv)
    users, items = draw_ids(rng, nu, (B,), pu), draw_ids(rng, ni, (B, 1 + G), pi)
    M = B * (1 + G)
    rand_index = torch.from_numpy(rng.integers(0, M, int(M * ns)).astype(np.int64))
    E = table(rng, int(torch.unique(items).numel()), d, sf)
    inp = (U, V, E, users, items, rand_index)
    want = clcrec_restate.step(*inp, T, lam, reg)
    f32 = clcrec_restate.step(*inp, T, lam, reg, dtype=torch.float32)
    plan = ops.clcrec_plan(users.to(DEV), items.to(DEV), nu, ni)
    counts = torch.bincount(rand_index, minlength=M).to(torch.int32).to(DEV)
    dev = [t.to(DEV) for t in (U, V, E)]
    judge("clcrec", params, lambda: ops.clcrec(*dev, plan, counts, T, lam, reg), want, f32, (1e-5, 1e-4))


def case_ccfcrec(rng):
    d = 4 * int(rng.integers(1, 65))
    B, P, N, S = int(rng.integers(1, 33)), int(rng.integers(1, 5)), int(rng.integers(1, 13)), int(rng.integers(1, 13))
    if rng.random() < 0.15:
        B, P, N, S = int(rng.integers(120, 160)), 1, int(rng.integers(1, 3)), int(rng.integers(1, 3))  # a user in chunks
    nu, ni = int(rng.integers(2, 30)), int(rng.integers(1, 60))
    su, sv, sq = (float(rng.choice(SCALES)) for _ in range(3))
    pu, pi = str(rng.choice(PATTERNS)), str(rng.choice(PATTERNS))
    tau, lam = float(rng.choice([0.05, 0.1, 0.5])), float(rng.choice([0.1, 0.6, 1.0]))
    params = dict(d=d, B=B, P=P, N=N, S=S, nu=nu, ni=ni, scales=(su, sv, sq), ids=(pu, pi), tau=tau, lambda1=lam)
    U, V, Q = table(rng, nu, d, su), table(rng, ni, d, sv), table(rng, B, d, sq)
    users, neg_users = draw_ids(rng, nu, (B,), pu), draw_ids(rng, nu, (B,), pu)
    # k_b != u_b, as a sampled negative user is: a user met only in records with k_b = u_b has the gradient +g - g, which
    # autograd forms as s + (-s) = 0 exactly and no other summation order does
    neg_users = torch.where(neg_users == users, (users + 1) % nu, neg_users)
    ids = (users, draw_ids(rng, ni, (B,), pi), neg_users, draw_ids(rng, ni, (B, P), pi), draw_ids(rng, ni, (B, P, N), pi),
           draw_ids(rng, ni, (B, S), pi))
    want = ccfcrec_restate.step(U, V, Q, *ids, tau, lam)
    f32 = ccfcrec_restate.step(U, V, Q, *ids, tau, lam, dtype=torch.float32)
    plan = ops.ccfcrec_plan(*(t.to(DEV) for t in ids), nu, ni)
    dev = [t.to(DEV) for t in (U, V, Q)]
    judge("ccfcrec", params, lambda: ops.ccfcrec(*dev, plan, tau, lam), want, f32, (ccf.LOSS_BAR, ccf.GRAD_BAR))


def case_aldi(rng):
    d = 4 * int(rng.integers(1, 65))
    B = int(rng.integers(1, 101))
    nu, ni = int(rng.integers(1, 30)), int(rng.integers(1, 60))
    st, sg = float(rng.choice(SCALES)), float(rng.choice(SCALES))
    pats = tuple(str(rng.choice(PATTERNS)) for _ in range(3))
    coef = [ald.COEF, ald.IDEN_ONLY, (0.5, 0.5, 0.5), (0.0, 0.0, 1.0)][int(rng.integers(0, 4))]
    params = dict(d=d, B=B, nu=nu, ni=ni, scales=(st, sg), ids=pats, coef=coef)
    U, V = table(rng, nu, d, st), table(rng, ni, d, st)
    users, pos, neg = draw_ids(rng, nu, (B,), pats[0]), draw_ids(rng, ni, (B,), pats[1]), draw_ids(rng, ni, (B,), pats[2])
    w = torch.from_numpy((0.2 + 0.8 * rng.random(ni)).astype(np.float32))
    for _ in range(50):        # L_rate's signs must be the same in every precision (tests/test_aldi.py demands the same)
        gu, gp, gn = (table(rng, B, d, sg) for _ in range(3))
        if aldi_restate.min_rate_gap(U, V, users, pos, neg, gu, gp, gn) >= 1e-5:
            break
    else:
        fail("aldi: no student outputs with min(|tp - sp|, |tn - sn|) >= 1e-5 in 50 draws", **params)
    inp = (U, V, users, pos, neg, gu, gp, gn, w)
    want = aldi_restate.step(*inp, *coef)
    f32 = aldi_restate.step(*inp, *coef, dtype=torch.float32)
    dev = [t.to(DEV) for t in inp]
    judge("aldi", params, lambda: ops.aldi(*dev, *coef), want, f32, (ald.LOSS_BAR, ald.GRAD_BAR), over_total=True)


def draw_nce_rows(rng):
    """The batch size: mostly 1 .. 700 with extra weight beside the wave (32 k) and workgroup (128 k) edges; one case in
    ten 1000 .. 2100, where the column splits hold more than one tile and some hold none."""
    u = rng.random()
    if u < 0.10:
        return int(rng.integers(1000, 2101))
    if u < 0.40:
        return 32 * int(rng.integers(1, 22)) + int(rng.integers(-1, 2))
    if u < 0.55:
        return 128 * int(rng.integers(1, 6)) + int(rng.choice([-1, 1]))
    return int(rng.integers(1, 701))


def case_infonce(rng):
    d = 4 * int(rng.integers(1, 65))
    n = draw_nce_rows(rng)
    tau, b_cos = float(rng.choice([0.05, 0.2, 1.0])), bool(rng.random() < 0.7)
    scale = float(rng.choice(SCALES))
    # raw dot products: rows of length ~scale, and no longer than sqrt(10 tau), so that |v|^2 / tau stays within the ~87
    # nats of fp32's exp at the narrow widths too (beyond it every float32 evaluation flushes the off-diagonal terms)
    row_scale = scale if b_cos else min(scale, float(np.sqrt(10.0 * tau))) / np.sqrt(d)
    mode = str(rng.choice(["whole", "rows", "n_dev", "accumulate"]))
    near = float(rng.choice([0.0, 0.25, 1.0]))
    rest = str(rng.choice(["augmented", "independent"]))
    zero_row = bool(rng.random() < 0.15)
    extra = 0 if mode == "whole" else int(rng.integers(1, 41))
    r1n, r2n = n + extra + (0 if mode == "whole" else int(rng.integers(0, 30))), n + extra + (0 if mode == "whole" else 5)
    params = dict(d=d, n=n, tau=tau, b_cos=b_cos, scale=scale, mode=mode, near=near, rest=rest, zero_row=zero_row,
                  tables=(r1n, r2n))
    # the batch, then its rows scattered into the tables
    v1 = table(rng, n, d, row_scale)
    k = int(round(n * near))
    v2 = v1 + table(rng, n, d, row_scale) * 0.7 if rest == "augmented" else table(rng, n, d, row_scale)
    v2[:k] = v1[:k] + table(rng, k, d, row_scale) * 0.02
    if zero_row:
        which, at = int(rng.integers(0, 3)), int(rng.integers(0, n))
        if which != 1:
            v1[at] = 0.0
        if which != 0:
            v2[at] = 0.0
    want = [t.numpy() for t in infonce_restate.infonce(v1, v2, tau, b_cos)[1:]]
    f32 = [t.numpy() for t in infonce_restate.infonce(v1, v2, tau, b_cos, dtype=torch.float32)[1:]]
    if mode == "whole":
        T1, T2, rows1, rows2 = v1.to(DEV), v2.to(DEV), None, None
    else:
        T1, T2 = table(rng, r1n, d, row_scale), table(rng, r2n, d, row_scale)
        p1, p2 = rng.permutation(r1n), rng.permutation(r2n)
        T1[torch.from_numpy(p1[:n])], T2[torch.from_numpy(p2[:n])] = v1, v2
        T1, T2 = T1.to(DEV), T2.to(DEV)
        m = n + extra if mode == "n_dev" else n          # n_dev < n_max: the row ids go on past the batch
        rows1, rows2 = (torch.from_numpy(p[:m].astype(np.int32)).to(DEV) for p in (p1, p2))
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV) if mode == "n_dev" else None

    def fused():
        if mode == "whole":
            return ops.infonce(T1, T2, tau, b_cos)
        G1, G2 = torch.full_like(T1, 3.0), torch.full_like(T2, 3.0)
        loss, _, _ = ops.infonce(T1, T2, tau, b_cos, rows1=rows1, rows2=rows2, n_dev=n_dev, grad1=G1, grad2=G2)
        return loss, G1, G2

    a, b = fused(), fused()
    torch.cuda.synchronize()
    if not all(torch.equal(x, y) for x, y in zip(a, b)):
        fail("infonce: two identical calls differ in their bits", **params)
    loss, g1, g2 = a
    if mode != "whole":
        for G, r in ((g1, rows1), (g2, rows2)):
            untouched = torch.ones(G.shape[0], dtype=torch.bool, device=DEV)
            untouched[r[:n].long()] = False
            if not (G[untouched] == 3.0).all():
                fail("infonce: a row outside the batch was written", **params)
        if mode == "accumulate":                         # a power of two: pre + scale * g holds bit for bit
            s = float(rng.choice([0.25, 0.5, 2.0]))
            P1, P2 = torch.from_numpy(rng.standard_normal((r1n, d)).astype(np.float32)).to(DEV), \
                torch.from_numpy(rng.standard_normal((r2n, d)).astype(np.float32)).to(DEV)
            A1, A2 = P1.clone(), P2.clone()
            la, _, _ = ops.infonce(T1, T2, tau, b_cos, rows1=rows1, rows2=rows2, scale=s, accumulate=True, grad1=A1, grad2=A2)
            for A, P, G, r in ((A1, P1, g1, rows1), (A2, P2, g2, rows2)):
                E = P.clone()
                E[r.long()] += s * G[r.long()]
                if not torch.equal(A, E):
                    fail("infonce: scale + accumulate is not pre + scale * g bit for bit", accumulate_scale=s, **params)
            if not torch.equal(la, loss):
                fail("infonce: scale + accumulate changed the loss", accumulate_scale=s, **params)
        g1, g2 = g1[rows1[:n].long()], g2[rows2[:n].long()]
    got = [t.cpu().numpy() for t in (loss[0], g1, g2)]
    if not all(np.isfinite(t).all() for t in got):
        fail("infonce: output not finite", **params)
    # loss: relative, no absolute floor (a batch of one has the loss 0: then exactly); gradients: row by row
    top = abs(float(want[0]))
    rel, rel32 = (abs(float(x[0]) - float(want[0])) / top if top > 0 else abs(float(x[0])) for x in (got, f32))
    rho = [infonce_restate.row_rho(g, w) for g, w in zip(got[1:], want[1:])]
    rho32 = [infonce_restate.row_rho(g, w) for g, w in zip(f32[1:], want[1:])]
    for g, w in zip(got[1:], want[1:]):
        if g[(w == 0).all(1)].any():
            fail("infonce: gradient not zero where the restatement's row is", **params)
    bars = (max(8 * rel32, 1e-5), max(8 * rho32[0], 1e-4), max(8 * rho32[1], 1e-4))
    if not (rel <= bars[0] and rho[0] <= bars[1] and rho[1] <= bars[2]):
        fail("infonce against the float64 restatement", loss=rel, rho=rho, bars=bars, float32=(rel32, rho32), **params)


def draw_triples(rng, d_max=256):
    """What a case of the three (user, positive, negative) kernels starts from: (d, B, nu, ni, patterns, users, pos, neg).
    B in [1, 100]; about one case in seven B in [300, 700] with hot or single ids, so that owners split into chunks.
    neg != pos in every record, as a sampled negative is: an item met only in records with pos = neg has the gradient
    +g - g, which autograd forms as s + (-s) = 0 exactly and no other summation order does."""
    d = 4 * int(rng.integers(1, d_max // 4 + 1))
    B, pool = int(rng.integers(1, 101)), PATTERNS
    if rng.random() < 1 / 7:
        B, pool = int(rng.integers(300, 701)), ["hot", "one"]
    pats = tuple(str(rng.choice(pool)) for _ in range(3))
    nu, ni = int(rng.integers(1, 30)), int(rng.integers(2, 60))
    users, pos, neg = draw_ids(rng, nu, (B,), pats[0]), draw_ids(rng, ni, (B,), pats[1]), draw_ids(rng, ni, (B,), pats[2])
    neg = torch.where(neg == pos, (pos + 1) % ni, neg)
    return d, B, nu, ni, pats, users, pos, neg


def case_gar(rng):
    d, B, nu, ni, pats, users, pos, neg = draw_triples(rng)
    su, sv, sg = (float(rng.choice(SCALES)) for _ in range(3))
    cold_user = bool(rng.random() < 0.5)
    alpha, beta = float(rng.choice([0.0, 0.05, 0.5, 1.0])), float(rng.choice([0.0, 0.1, 0.5, 1.0]))
    reg = float(rng.choice([0.0, 1e-4, 1e-2, 1.0, float(B)]))
    params = dict(d=d, B=B, nu=nu, ni=ni, scales=(su, sv, sg), ids=pats, cold_user=cold_user, coef=(alpha, beta, reg))
    U, V = table(rng, nu, d, su), table(rng, ni, d, sv)
    G = torch.tanh(table(rng, B, d, sg))                           # the generator ends in a tanh
    inp = (U, V, users, pos, neg, G)
    want = gar_restate.step(*inp, alpha, beta, reg, cold_user)
    f32 = gar_restate.step(*inp, alpha, beta, reg, cold_user, dtype=torch.float32)
    plan = ops.gar_plan(users.to(DEV), pos.to(DEV), neg.to(DEV), nu, ni)
    dev = [t.to(DEV) for t in (U, V, G)]
    judge("gar", params, lambda: ops.gar(*dev, plan, alpha, beta, reg, cold_user=cold_user), want, f32,
          (gar.LOSS_BAR, gar.GRAD_BAR), over_total=True)


def case_mtpr(rng):
    d, B, nu, ni, pats, users, pos, neg = draw_triples(rng, d_max=128)     # MTPR's d <= 128: its tables are d and 2 d wide
    st, sh, sw = (float(rng.choice(SCALES)) for _ in range(3))
    cold_user = bool(rng.random() < 0.5)
    wd1 = float(rng.choice([0.0, 0.01, 0.05]))
    params = dict(d=d, B=B, nu=nu, ni=ni, scales=(st, sh, sw), ids=pats, cold_user=cold_user, wd1=wd1)
    wp, wq, hr = (d, 2 * d, B) if cold_user else (2 * d, d, 2 * B)
    # tests/mtpr_restate.py's sizes times the scale: rows of 0.5, projections xavier-sized
    P, Q, h = table(rng, nu, wp, 0.5 * st), table(rng, ni, wq, 0.5 * st), table(rng, hr, d, 0.5 * sh)
    weu, wei = table(rng, 2 * d, d, sw / d ** 0.5), table(rng, 2 * d, d, sw / d ** 0.5)
    inp = (P, Q, h, weu, wei, users, pos, neg)
    want = mtpr_restate.step(*inp, wd1, cold_user)
    f32 = mtpr_restate.step(*inp, wd1, cold_user, dtype=torch.float32)
    plan = ops.mtpr_plan(users.to(DEV), pos.to(DEV), neg.to(DEV), nu, ni)
    dev = [t.to(DEV) for t in (P, Q, h, weu, wei)]
    judge("mtpr", params, lambda: ops.mtpr(*dev, plan, wd1, cold_user=cold_user), want, f32, (mtpr.LOSS_BAR, mtpr.GRAD_BAR),
          over_total=True)


def case_vbpr(rng):
    d, B, nu, ni, pats, users, pos, neg = draw_triples(rng)
    st, sa, sh = (float(rng.choice(SCALES)) for _ in range(3))
    cold_user = bool(rng.random() < 0.5)
    adv = bool(not cold_user and rng.random() < 0.5)
    wd1, lmd = float(rng.choice([0.0, 0.01, 0.05])), float(rng.choice([0.0, 0.7, 1.0]))
    params = dict(d=d, B=B, nu=nu, ni=ni, scales=(st, sa, sh), ids=pats, cold_user=cold_user, h_adv=adv, wd1=wd1, lmd=lmd)
    w = 2.0 * d ** -0.25                     # a dot product of two rows: of order 4 x the two scales at every width
    P, Q = table(rng, nu, d, w * st), table(rng, ni, d, w * st)
    A = table(rng, ni if cold_user else nu, d, w * sa)
    h = table(rng, B if cold_user else 2 * B, d, w * sh)
    h_adv = h + table(rng, h.shape[0], d, 0.1 * w * sh) if adv else None
    inp = (P, Q, A, h, h_adv, users, pos, neg)
    want = vbpr_restate.step(*inp, wd1, cold_user, lmd)
    f32 = vbpr_restate.step(*inp, wd1, cold_user, lmd, dtype=torch.float32)
    plan = ops.vbpr_plan(users.to(DEV), pos.to(DEV), neg.to(DEV), nu, ni)
    dev = [None if t is None else t.to(DEV) for t in (P, Q, A, h, h_adv)]
    judge("vbpr", params, lambda: ops.vbpr(*dev[:4], plan, wd1, h_adv=dev[4], lmd=lmd, cold_user=cold_user, want_hsum=True),
          want, f32, (vbpr.LOSS_BAR, vbpr.GRAD_BAR), over_total=True)


KINDS = {"clcrec": case_clcrec, "ccfcrec": case_ccfcrec, "aldi": case_aldi, "infonce": case_infonce, "gar": case_gar,
         "mtpr": case_mtpr, "vbpr": case_vbpr}


def main():
    global SEED
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--only", default="", help="run only these kinds of case, comma-separated (%s)" % " / ".join(KINDS))
    args = ap.parse_args()
    SEED = args.seed
    only = [k for k in args.only.split(",") if k]
    for k in only:
        if k not in KINDS:
            ap.error("--only: unknown kind %r (kinds: %s)" % (k, ", ".join(KINDS)))
    kinds = only or list(KINDS)
    rng = np.random.default_rng(args.seed)
    counts = {k: 0 for k in KINDS}
    for _ in range(args.cases):
        which = kinds[0] if len(kinds) == 1 else str(rng.choice(kinds))
        KINDS[which](rng)
        counts[which] += 1
    print(f"fuzz ok: {counts} random cases within parity, seed {args.seed}")


if __name__ == "__main__":
    main()
