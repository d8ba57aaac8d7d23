#!/usr/bin/env python3
"""Randomised parity fuzzing of the three fused loss kernels (csrc/clcrec.hip, csrc/ccfcrec.hip, csrc/aldi.hip) against
their float64 restatements (tests/clcrec_restate.py, tests/ccfcrec_restate.py, tests/aldi_restate.py).

Per case: a width from every multiple of 4 in [4, 256], small B, G, P, N and S (now and then a batch long enough for an
owner to split into chunks), an id pattern per id tensor from {uniform, a few hot ids, one owner}, a scale per table from
{0.05, 0.3, 1.5} and temperatures / coefficients the trainers accept.  Then
  * the kernel against the float64 restatement.  The bar of a case is 8x the distance of the float32 restatement from the
    float64 one at that same case, computed here on the CPU, and no lower than the fixed bar of the kernel's test file
    (tests/test_clcrec_gpu.py 1e-5 / 1e-4, tests/test_ccfcrec_gpu.py LOSS_BAR / GRAD_BAR, tests/test_aldi_gpu.py the same).
    Loss terms: relative error, a term's magnitude floored at 1e-6 of the total (a term that far below the total is
    rounding noise in any float32 evaluation; ALDI's, as in its file, over the total); gradients: error over the table's
    maximum; a gradient the restatement leaves all zero must be all zero;
  * a second, identical call: every output bit-equal.
On a mismatch the seed and the drawn parameters are printed and the exit status is 1.

    python tests/fuzz/fuzz_loss_ops.py --cases 200 [--seed 0] [--only clcrec,ccfcrec,aldi]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from coldrec_amd import ops  # noqa: E402
from tests import aldi_restate, ccfcrec_restate, clcrec_restate  # noqa: E402
from tests import test_aldi_gpu as ald  # noqa: E402
from tests import test_ccfcrec_gpu as ccf  # noqa: E402

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
    """(worst loss-term error, worst gradient error / maximum) of (terms, g1, g2, g3) numpy tuples; the last term is the
    total.  A gradient whose reference is all zero counts with its own largest entry."""
    terms, ref = np.asarray(got[0], np.float64), np.asarray(want[0], np.float64)
    total = abs(ref[-1])
    den = total if over_total else np.maximum(np.abs(ref), 1e-6 * total)
    rel = float((np.abs(terms - ref) / den).max())
    errs = []
    for g, w in zip(got[1:], want[1:]):
        g = np.asarray(g, np.float64)
        top = np.abs(w).max()
        errs.append(float(np.abs(g - w).max() / top) if top > 0 else float(np.abs(g).max()))
    return rel, max(errs)


def judge(kind, params, fused, want, f32, fixed, over_total=False):
    """``fused()`` -> (loss, g1, g2, g3) device tensors; called twice."""
    a, b = fused(), fused()
    torch.cuda.synchronize()
    if not all(torch.equal(x, y) for x, y in zip(a, b)):
        fail(kind + ": two identical calls differ in their bits", **params)
    got = tuple(t.cpu().numpy() for t in a)
    if not all(np.isfinite(t).all() for t in got):
        fail(kind + ": output not finite", **params)
    ref_rel, ref_err = distances(f32, want, over_total)
    bars = (max(8 * ref_rel, fixed[0]), max(8 * ref_err, fixed[1]))
    rel, err = distances(got, want, over_total)
    for g, w in zip(got[1:], want[1:]):
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


KINDS = {"clcrec": case_clcrec, "ccfcrec": case_ccfcrec, "aldi": case_aldi}


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
