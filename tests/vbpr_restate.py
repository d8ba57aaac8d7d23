"""Restatement of the two-tower BPR loss of VBPR / AMR and of whole VBPR and AMR runs in plain torch (any dtype, runs
anywhere), written from the formulas.  d = the width; P (nu, d), Q (ni, d); content rows C, H = C[ids] @ W:

    base = <P[u], Q[i] - Q[j]>
    item mode  A (nu, d):  x = base + <A[u], H_i - H_j>,  x_adv = base + <A[u], Hadv_i - Hadv_j>
    user mode  A (ni, d):  x = base + <H_b, A[i] - A[j]>
    sp(t) = softplus(-t);  L_bpr = sum sp(x),  L_adv = lmd sum sp(x_adv)  (0 without H_adv)
    R_emb = wd1 sum_b (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2 + |A[u]|^2)   (user mode: |A[i]|^2 + |A[j]|^2 for |A[u]|^2)
    R_w = wd2 |W|^2

The kernel's ``h`` argument is H with one row per occurrence: (2 B, d) = positives then negatives in item mode, (B, d)
in user mode.  Gradients come from autograd: dense for the three tables (index_put accumulates duplicate ids).

AMR's run is written in the running-sum form: a noise buffer (ni, content_dim) of zeros that is never cleared; per step
noise += d L_bpr / d C, then the step's loss with C[ids] + eps normalize(noise[ids]) in the adversarial term (the noise a
constant), then noise += d (L_bpr + L_adv) / d C -- what the reference's never-cleared ``item_content.grad`` holds.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gar_restate import toy_data        # noqa: F401  (G26 uses G24's splits: make_dataset("toy", cold, seed=1))
from tests.mtpr_restate import adagrad        # noqa: F401  (Adagrad's default step over rows)

P_EMB, P_CTX = (0.05, 0.01), (0.05, 0.01)      # G26's (lr, wd) pairs: the default wd1 = 0 would leave R_emb untested
EPS, LMD = 0.1, 1.0


def loss_terms(P, Q, A, h, users, pos, neg, wd1, cold_user, h_adv=None, lmd=1.0):
    """(L_bpr, L_adv, R_emb, their sum)."""
    B = users.shape[0]
    base = (P[users] * (Q[pos] - Q[neg])).sum(1)
    if cold_user:
        assert h_adv is None
        x = base + (h * (A[pos] - A[neg])).sum(1)
        ra = (A[pos] ** 2).sum() + (A[neg] ** 2).sum()
    else:
        x = base + (A[users] * (h[:B] - h[B:])).sum(1)
        ra = (A[users] ** 2).sum()
    L = F.softplus(-x).sum()
    La = torch.zeros((), dtype=L.dtype)
    if h_adv is not None:
        La = lmd * F.softplus(-(base + (A[users] * (h_adv[:B] - h_adv[B:])).sum(1))).sum()
    R = wd1 * ((P[users] ** 2).sum() + (Q[pos] ** 2).sum() + (Q[neg] ** 2).sum() + ra)
    return L, La, R, L + La + R


def step(P, Q, A, h, h_adv, users, pos, neg, wd1, cold_user, lmd=1.0, dtype=torch.float64):
    """One step on leaf copies of the fp32 inputs in ``dtype``.  Returns (loss4, d P, d Q, d A, d h, d h_adv, hsum) as
    numpy float64; without h_adv its gradient is None; hsum = d h (+ d h_adv) summed per distinct cold object, ascending."""
    leaves = [None if t is None else t.detach().cpu().to(dtype).requires_grad_() for t in (P, Q, A, h, h_adv)]
    ids = [t.cpu().long() for t in (users, pos, neg)]
    terms = loss_terms(*leaves[:4], *ids, wd1, cold_user, leaves[4], lmd)
    live = [t for t in leaves if t is not None]
    grads = list(torch.autograd.grad(terms[3], live, allow_unused=True))
    grads = [torch.zeros_like(t) if g is None else g for g, t in zip(grads, live)]
    if h_adv is None:
        grads.append(None)
    own = ids[0] if cold_user else torch.cat(ids[1:])
    hs = owner_sums(grads[3] if grads[4] is None else grads[3] + grads[4], own)
    out = [None if g is None else g.double().numpy() for g in grads]
    return (np.array([float(t.detach()) for t in terms]),) + tuple(out) + (hs.double().numpy(),)


def owner_sums(rows, ids):
    """rows (M, d) summed per distinct id, the ids ascending."""
    uniq, inv = torch.unique(ids, return_inverse=True)
    return torch.zeros(uniq.shape[0], rows.shape[1], dtype=rows.dtype).index_add_(0, inv, rows)


def init(nu, ni, content_dim, d, cold_user):
    """(PQ2, W) in the reference's draw order on the global CPU stream: the Embeddings P, Q, PQ2 (their normal_ draws; P's
    and Q's are overwritten by the loaded tables), xavier_uniform_ on PQ2, then randn + xavier_uniform_ for W."""
    nn.Embedding(nu, d)
    nn.Embedding(ni, d)
    A = nn.Embedding(ni if cold_user else nu, d)
    nn.init.xavier_uniform_(A.weight)
    W = nn.init.xavier_uniform_(torch.randn(content_dim, d, dtype=torch.float32))
    return A.weight.detach().clone(), W


def published(P, Q, A, W, content, cold_user):
    """(user_emb, item_emb) = [main | aux], whose product is the reference's score1 + score2."""
    cw = content @ W
    return (torch.cat([P, cw], 1), torch.cat([Q, A], 1)) if cold_user else (torch.cat([P, A], 1), torch.cat([Q, cw], 1))


def run(data, dtype, cold_user, start, amr=False, width=64, epochs=2, bs=512, seed=2024, p_emb=P_EMB, p_ctx=P_CTX, eps=EPS,
        lmd=LMD):
    """The whole training run (no evaluation) on the global random streams.  ``start``: VBPR (P, Q) = the backbone's
    tables, PQ2 and W are drawn by ``init``; AMR (P, Q, PQ2, W).  torch.optim.Adagrad over P, Q, PQ2, Adam over W.
    Returns dict(init = the initial (P, Q, PQ2, W) (float32), terms (steps, 3) = [bpr, regs, batch_loss] or (steps, 4) =
    [bpr, adv, regs, batch_loss] with regs = R_emb + R_w, trained = the four tensors at the end, snaps = per epoch the
    four tensors, touched = (user mask, item mask), noise_norms = the noise's Frobenius norm after each addition)."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    set_seed(seed, False)
    content = np.asarray(data.mapped_user_content if cold_user else data.mapped_item_content)
    first = tuple(torch.as_tensor(np.asarray(t), dtype=torch.float32) for t in start)
    if not amr:
        first = first + init(data.user_num, data.item_num, content.shape[1], width, cold_user)
    content = torch.as_tensor(content, dtype=torch.float32).to(dtype)
    P, Q, A, W = (nn.Parameter(t.to(dtype).clone()) for t in first)
    (lr1, wd1), (lr2, wd2) = p_emb, p_ctx
    opts = [torch.optim.Adagrad([P, A, Q], lr=lr1), torch.optim.Adam([W], lr=lr2)]
    touched = (np.zeros(P.shape[0], bool), np.zeros(Q.shape[0], bool))
    noise = torch.zeros_like(content)
    terms, snaps, norms = [], [], []
    for _ in range(epochs):
        eu, ei, ej = (torch.from_numpy(x).long() for x in epoch_triples(data, bs))
        touched[0][eu.numpy()] = True
        touched[1][ei.numpy()] = True
        touched[1][ej.numpy()] = True
        for lo in range(0, eu.shape[0], bs):
            u, p, n = eu[lo:lo + bs], ei[lo:lo + bs], ej[lo:lo + bs]
            ids = u if cold_user else torch.cat([p, n])
            h = content[ids] @ W
            h_adv = None
            if amr:
                plain = loss_terms(P, Q, A, h, u, p, n, wd1, cold_user)[0]
                dh, = torch.autograd.grad(plain, h, retain_graph=True)
                noise.index_add_(0, ids, dh @ W.detach().T)
                norms.append(float(torch.linalg.norm(noise)))
                h_adv = (content[ids] + eps * F.normalize(noise[ids])) @ W
                h.retain_grad()
                h_adv.retain_grad()
            t = loss_terms(P, Q, A, h, u, p, n, wd1, cold_user, h_adv, lmd)
            rw = wd2 * (W ** 2).sum()
            total = t[3] + rw
            for o in opts:
                o.zero_grad()
            total.backward()
            if amr:
                noise.index_add_(0, ids, (h.grad + h_adv.grad) @ W.detach().T)
                norms.append(float(torch.linalg.norm(noise)))
            for o in opts:
                o.step()
            row = [float(t[0].detach())] + ([float(t[1].detach())] if amr else [])
            terms.append(row + [float((t[2] + rw).detach()), float(total.detach())])
        snaps.append(tuple(x.detach().double().numpy().copy() for x in (P, Q, A, W)))
    return dict(init=tuple(t.numpy().copy() for t in first), terms=np.array(terms, np.float64), trained=snaps[-1], snaps=snaps,
                touched=touched, noise_norms=np.array(norms, np.float64))


# ---- the G26 fixtures ---------------------------------------------------------------------------------------------------

NAMES = ("P", "Q", "PQ2", "W")
FILES = ("user_emb_main_P", "item_emb_main_Q", "user_emb_aux", "item_emb_aux", "W")      # the reference's --save_emb names


def start_of(fx, amr):
    """What a run of the fixture starts from: VBPR the backbone's (user, item) tables, AMR VBPR's saved (P, Q, PQ2, W)."""
    if amr:
        return tuple(fx["loaded_" + k] for k in ("user_emb_main", "item_emb_main", "user_emb_aux", "w_value"))
    return fx["loaded_U"], fx["loaded_V"]


def best_of(fx):
    """The best epoch's (P, Q, PQ2, W) of the fixture: stored apart only where the best epoch is not the last."""
    return tuple(fx[("trained_" if bool(fx["best_is_last"]) else "best_") + k] for k in NAMES)


def ranked_of(fx, content, cold_user):
    """dict(user_emb, item_emb) = the fixture's best-epoch [main | aux] pair in float64, beside the fixture's lists: what
    tests.test_gar_gpu.lists_vs_reference takes."""
    four = [torch.from_numpy(np.asarray(t, np.float64)) for t in best_of(fx)]
    user, item = published(*four, torch.from_numpy(np.asarray(content, np.float64)), cold_user)
    out = {k: fx[k] for k in fx.files}
    out.update(user_emb=user.numpy(), item_emb=item.numpy())
    return out


def run_distances(fx, terms, best, trained, noise_norms=None):
    """Against G26: (worst |term - G26's| / G26's batch_loss over the steps, [|best tensor - G26's| / its scale for P, Q,
    PQ2, W], [the same for the trained four], worst relative difference of the noise norms or None)."""
    want = fx["terms"]
    assert terms.shape == want.shape
    rel = float((np.abs(terms - want) / np.abs(want[:, -1:])).max())
    dist = lambda t, w: float(np.abs(np.asarray(t, np.float64) - w).max() / np.abs(w).max())
    e_noise = None
    if noise_norms is not None:
        w = fx["noise_norms"]
        assert noise_norms.shape == w.shape
        e_noise = float((np.abs(noise_norms - w) / w).max())
    return (rel, [dist(t, w) for t, w in zip(best, best_of(fx))],
            [dist(t, fx["trained_" + k]) for t, k in zip(trained, NAMES)], e_noise)


# ---- the cases of the kernel tests (tests/test_vbpr.py measures the float32 formula at them, tests/test_vbpr_gpu.py the
# kernel) --------------------------------------------------------------------------------------------------------------

# B, d, nu, ni; "chunks": 3 users with 2 chunk + 1 records each, four of 5 items with 2 chunk + 1 of the 2B occurrences and
# the fifth with 4 chunk + 2
CASES = [(1, 4, 11, 11), (2, 4, 11, 13), (33, 20, 11, 30), (32, 32, 40, 40), (63, 64, 50, 400), (65, 124, 300, 500),
         (300, 128, 11, 500), (7, 256, 11, 13), ("chunks", 64, 3, 5), (2048, 64, 300, 500), (16417, 4, 300, 500)]
CASE_IDS = lambda c: "B%s-d%d" % c[:2]
VARIANTS = [(False, False), (False, True), (True, False)]          # (cold_user, with h_adv)
VARIANT_IDS = lambda v: ("user" if v[0] else "item") + ("-adv" if v[1] else "")
WD1, CASE_LMD = 0.01, 0.7


def inputs(case, cold_user, adv=False, chunk=256, seed=0, scale=1.0):
    """(P, Q, A, h, h_adv or None, users, pos, neg) on the CPU; ids drawn with repeats; h_adv = h + a shift of a tenth
    of its size."""
    B, d, nu, ni = case
    g = torch.Generator().manual_seed(2600 + seed + d + 7 * (B if B != "chunks" else 513) + int(cold_user))
    if B == "chunks":
        B = 3 * (2 * chunk + 1)
        users = torch.arange(3).repeat_interleave(2 * chunk + 1)[torch.randperm(B, generator=g)]
        occ = torch.cat([torch.arange(4).repeat_interleave(2 * chunk + 1), torch.full((4 * chunk + 2,), 4)])
        occ = occ[torch.randperm(2 * B, generator=g)]
        pos, neg = occ[:B].clone(), occ[B:].clone()
    else:
        users = torch.randint(nu, (B,), generator=g)
        pos, neg = torch.randint(ni, (B,), generator=g), torch.randint(ni, (B,), generator=g)
    size = scale * (8.0 / d) ** 0.5 * 0.5                       # scores of order one at every width
    P, Q = torch.randn(nu, d, generator=g) * size, torch.randn(ni, d, generator=g) * size
    A = torch.randn(ni if cold_user else nu, d, generator=g) * size
    h = torch.randn(B if cold_user else 2 * B, d, generator=g) * size
    h_adv = h + torch.randn(h.shape, generator=g) * (0.1 * size) if adv else None
    return P, Q, A, h, h_adv, users, pos, neg


def edge_cases(cold_user, adv):
    """(tag, inputs, wd1, lmd) of the edges."""
    out = []
    base = (33, 20, 11, 30)
    inp = list(inputs(base, cold_user, adv, seed=1))
    inp[7] = inp[7].clone()
    inp[7][5] = inp[6][5]                                             # a record with pos == neg: x = 0
    out.append(("pos-is-neg", inp, WD1, CASE_LMD))
    inp = list(inputs(base, cold_user, adv, seed=2))
    inp[6], inp[7] = inp[6].clone(), inp[7].clone()
    inp[6][0], inp[7][0], inp[6][1], inp[7][1] = 7, 8, 9, 7           # item 7: a positive in record 0, a negative in 1
    out.append(("pos-and-neg", inp, WD1, CASE_LMD))
    inp = list(inputs(base, cold_user, adv, seed=3))
    inp[5] = torch.full_like(inp[5], 4)                               # one user owns every record
    out.append(("one-user", inp, WD1, CASE_LMD))
    out.append(("wd0", list(inputs(base, cold_user, adv, seed=4)), 0.0, CASE_LMD))
    inp = list(inputs((65, 64, 50, 400), cold_user, adv, seed=5))
    inp[3] = torch.zeros_like(inp[3])                                 # H = 0
    out.append(("h-zero", inp, WD1, CASE_LMD))
    out.append(("scores-beyond-30", list(inputs((65, 64, 50, 400), cold_user, adv, seed=7, scale=9.0)), WD1, CASE_LMD))
    out.append(("one-record", list(inputs((1, 20, 11, 30), cold_user, adv, seed=8)), WD1, CASE_LMD))
    if adv:
        inp = list(inputs((65, 64, 50, 400), cold_user, adv, seed=9))
        inp[4] = inp[3].clone()                                       # H_adv == H: L_adv = lmd L_bpr
        out.append(("adv-is-plain", inp, WD1, CASE_LMD))
        out.append(("lmd-zero", list(inputs((65, 64, 50, 400), cold_user, adv, seed=10)), WD1, 0.0))
    return out


EDGE_TAGS = [(v, k, e[0]) for v in VARIANTS for k, e in enumerate(edge_cases(*v))]


def distances(got, want):
    """(worst error of the four loss terms over the total, [error / maximum of each gradient; None where there is none])."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]).max() / abs(want[0][3])
    errs = []
    for g, w in zip(got[1:], want[1:]):
        if w is None:
            assert g is None
            continue
        top = np.abs(w).max()
        errs.append(float(np.abs(np.asarray(g, np.float64) - w).max() / top) if top > 0 else float(np.abs(g).max()))
    return float(rel), errs
