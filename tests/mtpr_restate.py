"""Restatement of MTPR's loss, of Adagrad's default step and of a whole MTPR run in plain torch (any dtype, runs
anywhere), written from the formulas.  d = the width; weu, wei (2 d, d); content rows C, H = C[ids] @ W:

    item mode  P (nu, 2 d), Q (ni, d):   e = P[u] weu;  f_x = [Q[x] | H_x] wei;  h_x = H_x wei[d:]
               s_x = <e, f_x>,  z_x = <e, h_x>                                  (x = i the positive, j the negative)
    user mode  P (nu, d), Q (ni, 2 d):   e_f = [P[u] | H_b] weu;  e_z = H_b weu[d:];  q_x = Q[x] wei
               s_x = <e_f, q_x>,  z_x = <e_z, q_x>
    sp(t) = softplus(-t);  L_i = sum sp(s_i - s_j), L_f = sum sp(z_i - z_j), L_if = sum sp(s_i - z_j), L_fi = sum sp(z_i - s_j)
    R_emb = wd1 sum_b (|P[u]|^2 + |Q[i]|^2 + |Q[j]|^2);   R_w = wd2 (|W|^2 + |weu|^2) + wd3 |wei|^2

The kernel's ``h`` argument is H with one row per occurrence: (2 B, d) = positives then negatives in item mode, (B, d)
in user mode.  Gradients come from autograd: dense for the two tables (index_put accumulates duplicate ids).
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gar_restate import toy_data        # noqa: F401  (G25 uses G24's splits: make_dataset("toy", cold, seed=1))

P_EMB, P_CTX, P_PROJ = (0.05, 0.0), (0.05, 0.01), (0.05, 0.01)      # the reference's default (lr, wd) pairs


def init(nu, ni, content_dim, d, cold_user):
    """The five tensors in the reference's draw order on the global CPU stream: Embedding P (its normal_ draw, then
    xavier_uniform_), Embedding Q likewise, then randn + xavier_uniform_ for W, weu, wei."""
    P = nn.Embedding(nu, d if cold_user else 2 * d)
    nn.init.xavier_uniform_(P.weight)
    Q = nn.Embedding(ni, 2 * d if cold_user else d)
    nn.init.xavier_uniform_(Q.weight)
    W = nn.init.xavier_uniform_(torch.randn(content_dim, d, dtype=torch.float32))
    weu = nn.init.xavier_uniform_(torch.randn(2 * d, d, dtype=torch.float32))
    wei = nn.init.xavier_uniform_(torch.randn(2 * d, d, dtype=torch.float32))
    return P.weight.detach().clone(), Q.weight.detach().clone(), W, weu, wei


def scores(P, Q, h, weu, wei, users, pos, neg, cold_user):
    """(s_i, s_j, z_i, z_j), each (B,)."""
    B, d = users.shape[0], weu.shape[1]
    if cold_user:
        ef = torch.cat([P[users], h], 1) @ weu
        ez = h @ weu[d:]
        qi, qj = Q[pos] @ wei, Q[neg] @ wei
        return (ef * qi).sum(1), (ef * qj).sum(1), (ez * qi).sum(1), (ez * qj).sum(1)
    e = P[users] @ weu
    hi, hj = h[:B] @ wei[d:], h[B:] @ wei[d:]
    fi, fj = Q[pos] @ wei[:d] + hi, Q[neg] @ wei[:d] + hj
    return (e * fi).sum(1), (e * fj).sum(1), (e * hi).sum(1), (e * hj).sum(1)


def loss_terms(P, Q, h, weu, wei, users, pos, neg, wd1, cold_user):
    """(L_i, L_f, L_if, L_fi, R_emb, their sum)."""
    si, sj, zi, zj = scores(P, Q, h, weu, wei, users, pos, neg, cold_user)
    sp = lambda t: F.softplus(-t).sum()
    Li, Lf, Lif, Lfi = sp(si - sj), sp(zi - zj), sp(si - zj), sp(zi - sj)
    R = wd1 * ((P[users] ** 2).sum() + (Q[pos] ** 2).sum() + (Q[neg] ** 2).sum())
    return Li, Lf, Lif, Lfi, R, Li + Lf + Lif + Lfi + R


def step(P, Q, h, weu, wei, users, pos, neg, wd1, cold_user, dtype=torch.float64):
    """One step on leaf copies of the fp32 inputs in ``dtype``.  Returns (loss6, d P, d Q, d h, d weu, d wei) as numpy
    float64."""
    leaves = [t.detach().cpu().to(dtype).requires_grad_() for t in (P, Q, h, weu, wei)]
    ids = [t.cpu().long() for t in (users, pos, neg)]
    terms = loss_terms(*leaves, *ids, wd1, cold_user)
    grads = torch.autograd.grad(terms[5], leaves, allow_unused=True)
    z = lambda g, t: (torch.zeros_like(t) if g is None else g).double().numpy()
    return (np.array([float(t.detach()) for t in terms]),) + tuple(z(g, t) for g, t in zip(grads, leaves))


def adagrad(p, g, s, ids, lr, eps=1e-10):
    """Adagrad's default step over the rows ``ids`` in the tensors' own dtype: returns new (p, s)."""
    p, s = p.clone(), s.clone()
    ids = ids.long()
    s[ids] = s[ids] + g[ids] * g[ids]
    p[ids] = p[ids] - lr * g[ids] / (s[ids].sqrt() + eps)
    return p, s


def derived(P, Q, W, weu, wei, content, cold_user):
    """(user_emb, item_emb) = the reference's forward()."""
    if cold_user:
        return torch.cat([P, content @ W], 1) @ weu, Q @ wei
    return P @ weu, torch.cat([Q, content @ W], 1) @ wei


def run(data, dtype, cold_user, width=64, epochs=2, bs=512, seed=2024, p_emb=P_EMB, p_ctx=P_CTX, p_proj=P_PROJ):
    """The whole training run (no evaluation) on the global random streams: set_seed, ``init``, then per epoch the
    pairwise sampler's triples; torch.optim.Adagrad over P, Q, Adam over [W, weu] and over [wei].  Returns dict(init = the
    five initial tensors (float32), terms (steps, 6) = [L_i, L_f, L_if, L_fi, regs, batch_loss] with regs = R_emb + R_w,
    trained = the five tensors at the end, snaps = per epoch (user_emb, item_emb), touched = (user mask, item mask))."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    set_seed(seed, False)
    content = np.asarray(data.mapped_user_content if cold_user else data.mapped_item_content)
    first = init(data.user_num, data.item_num, content.shape[1], width, cold_user)
    content = torch.as_tensor(content, dtype=torch.float32).to(dtype)
    P, Q, W, weu, wei = (nn.Parameter(t.to(dtype).clone()) for t in first)
    (lr1, wd1), (lr2, wd2), (lr3, wd3) = p_emb, p_ctx, p_proj
    opts = [torch.optim.Adagrad([P, Q], lr=lr1), torch.optim.Adam([W, weu], lr=lr2), torch.optim.Adam([wei], lr=lr3)]
    touched = (np.zeros(P.shape[0], bool), np.zeros(Q.shape[0], bool))
    terms, snaps = [], []
    for _ in range(epochs):
        eu, ei, ej = (torch.from_numpy(x).long() for x in epoch_triples(data, bs))
        touched[0][eu.numpy()] = True
        touched[1][ei.numpy()] = True
        touched[1][ej.numpy()] = True
        for lo in range(0, eu.shape[0], bs):
            u, p, n = eu[lo:lo + bs], ei[lo:lo + bs], ej[lo:lo + bs]
            h = content[u] @ W if cold_user else content[torch.cat([p, n])] @ W
            t = loss_terms(P, Q, h, weu, wei, u, p, n, wd1, cold_user)
            rw = wd2 * ((W ** 2).sum() + (weu ** 2).sum()) + wd3 * (wei ** 2).sum()
            total = t[5] + rw
            for o in opts:
                o.zero_grad()
            total.backward()
            for o in opts:
                o.step()
            terms.append([float(x.detach()) for x in t[:4]] + [float((t[4] + rw).detach()), float(total.detach())])
        with torch.no_grad():
            snaps.append(tuple(x.double().numpy().copy() for x in derived(P, Q, W, weu, wei, content, cold_user)))
    trained = tuple(x.detach().double().numpy().copy() for x in (P, Q, W, weu, wei))
    return dict(init=tuple(t.numpy().copy() for t in first), terms=np.array(terms, np.float64), trained=trained, snaps=snaps,
                touched=touched)


# ---- the cases of the kernel tests (tests/test_mtpr.py measures the float32 formula at them, tests/test_mtpr_gpu.py the
# kernel) --------------------------------------------------------------------------------------------------------------

# B, d, nu, ni; "chunks": as GAR's case -- 3 users with 2 chunk + 1 records each, four of 5 items with 2 chunk + 1 of the 2B
# occurrences and the fifth with 4 chunk + 2.  (16417, 4): one record more than 512 tiles and a tile: two tiles per workgroup
CASES = [(1, 4, 11, 11), (2, 4, 11, 13), (33, 20, 11, 30), (32, 32, 40, 40), (63, 64, 50, 400), (65, 124, 300, 500),
         (300, 128, 11, 500), ("chunks", 64, 3, 5), (2048, 64, 300, 500), (16417, 4, 300, 500)]
CASE_IDS = lambda c: "B%s-d%d" % c[:2]
WD1 = 0.01


def inputs(case, cold_user, chunk=256, seed=0, scale=1.0):
    """(P, Q, h, weu, wei, users, pos, neg) on the CPU; ids drawn with repeats; tables and projections xavier-sized times
    ``scale``."""
    B, d, nu, ni = case
    g = torch.Generator().manual_seed(2500 + seed + d + 7 * (B if B != "chunks" else 513) + int(cold_user))
    if B == "chunks":
        B = 3 * (2 * chunk + 1)
        users = torch.arange(3).repeat_interleave(2 * chunk + 1)[torch.randperm(B, generator=g)]
        occ = torch.cat([torch.arange(4).repeat_interleave(2 * chunk + 1), torch.full((4 * chunk + 2,), 4)])
        occ = occ[torch.randperm(2 * B, generator=g)]
        pos, neg = occ[:B].clone(), occ[B:].clone()
    else:
        users = torch.randint(nu, (B,), generator=g)
        pos, neg = torch.randint(ni, (B,), generator=g), torch.randint(ni, (B,), generator=g)
    wp, wq, hr = (d, 2 * d, B) if cold_user else (2 * d, d, 2 * B)
    P, Q = torch.randn(nu, wp, generator=g) * (0.5 * scale), torch.randn(ni, wq, generator=g) * (0.5 * scale)
    h = torch.randn(hr, d, generator=g) * (0.5 * scale)
    weu = torch.randn(2 * d, d, generator=g) * (scale / d ** 0.5)
    wei = torch.randn(2 * d, d, generator=g) * (scale / d ** 0.5)
    return P, Q, h, weu, wei, users, pos, neg


def edge_cases(cold_user):
    """(tag, inputs, wd1) of the edges."""
    out = []
    base = (33, 20, 11, 30)
    inp = list(inputs(base, cold_user, seed=1))
    inp[7] = inp[7].clone()
    inp[7][5] = inp[6][5]                                             # a record with pos == neg
    out.append(("pos-is-neg", inp, WD1))
    inp = list(inputs(base, cold_user, seed=2))
    inp[6], inp[7] = inp[6].clone(), inp[7].clone()
    inp[6][0], inp[7][0], inp[6][1], inp[7][1] = 7, 8, 9, 7           # item 7: a positive in record 0, a negative in 1
    out.append(("pos-and-neg", inp, WD1))
    inp = list(inputs(base, cold_user, seed=3))
    inp[5] = torch.full_like(inp[5], 4)                               # one user owns every record
    out.append(("one-user", inp, WD1))
    out.append(("wd0", list(inputs(base, cold_user, seed=4)), 0.0))
    inp = list(inputs((65, 64, 50, 400), cold_user, seed=5))
    inp[2] = torch.zeros_like(inp[2])                                 # H = 0: every z is 0 in item mode
    out.append(("h-zero", inp, WD1))
    inp = list(inputs((65, 64, 50, 400), cold_user, seed=6))
    inp[3] = torch.zeros_like(inp[3])                                 # weu = 0: all scores 0, table gradients 0, dweu != 0
    out.append(("weu-zero", inp, 0.0))
    out.append(("scores-beyond-30", list(inputs((65, 64, 50, 400), cold_user, seed=7, scale=2.0)), WD1))
    inp = list(inputs((63, 64, 50, 400), cold_user, seed=8))
    for k in (5, 6, 7):
        inp[k] = inp[k].clone()
    inp[5][0], inp[5][1], inp[6][0], inp[6][1], inp[7][2], inp[7][3] = 0, 49, 0, 399, 0, 399
    out.append(("first-and-last-rows", inp, WD1))
    return out


def distances(got, want):
    """(worst error of the six loss terms over the total, [error / maximum of each gradient]) of numpy tuples."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]).max() / abs(want[0][5])
    errs = []
    for g, w in zip(got[1:], want[1:]):
        top = np.abs(w).max()
        errs.append(np.abs(np.asarray(g, np.float64) - w).max() / top if top > 0 else np.abs(g).max())
    return rel, errs


ADAGRAD_CASES = [(d, zero_acc) for d in (4, 20, 64, 256) for zero_acc in (True, False)]
ADAGRAD_LR = 0.05


def adagrad_inputs(d, zero_acc, rows=50):
    """(p, g, s, ids): 23 distinct of the 50 rows in no order, three of them with a zero gradient; |g| of order 1; the
    accumulator zero (the first step) or positive."""
    gen = torch.Generator().manual_seed(2600 + d + int(zero_acc))
    p, g = torch.randn(rows, d, generator=gen) * 0.1, torch.randn(rows, d, generator=gen)
    s = torch.zeros(rows, d) if zero_acc else torch.rand(rows, d, generator=gen) * 4
    ids = torch.randperm(rows, generator=gen)[:23].to(torch.int32)
    g[ids[:3].long()] = 0.0
    return p, g, s, ids


def run_distances(fx, terms, best, trained):
    """Against G25: (worst |term - G25's| / G25's batch_loss over the steps, [|best table - G25's| / its scale for user_emb,
    item_emb], [the same for the trained P, Q, W, weu, wei])."""
    want = fx["terms"]
    assert terms.shape == want.shape
    rel = float((np.abs(terms - want) / np.abs(want[:, 5:6])).max())
    dist = lambda t, k: float(np.abs(np.asarray(t, np.float64) - fx[k]).max() / np.abs(fx[k]).max())
    return (rel, [dist(t, k) for t, k in zip(best, ("user_emb", "item_emb"))],
            [dist(t, "trained_" + k) for t, k in zip(trained, ("P", "Q", "W", "weu", "wei"))])
