"""Restatement of CCFCRec's loss and of a whole CCFCRec run in plain torch (any dtype, runs anywhere), written from the
formulas.  With c(q, v) = <q, v> / (tau |q| |v|) (no epsilon) and per record b the user u_b, item i_b, negative user k_b,
positives pos_bp, negatives neg_bpn, self-negatives sneg_bs and q_b = the content encoder's output for i_b:

    L_c  = (1/P) sum_b sum_p [logsumexp(c(q_b, V[pos_bp]), c(q_b, V[neg_bp.])) - c(q_b, V[pos_bp])]
    L_s  =       sum_b       [logsumexp(c(q_b, V[i_b]),    c(q_b, V[sneg_b.])) - c(q_b, V[i_b])]
    L_r1 = sum_b softplus(-(<V[i_b], U[u_b]> - <V[i_b], U[k_b]>))     L_r2 = the same with q_b in V[i_b]'s place
    total = lambda1 (L_c + L_s) + (1 - lambda1)(L_r1 + L_r2)

Sums over the batch, not means; no regulariser.  Gradients come from autograd.
"""
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def crc(*arrays) -> int:
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def loss_terms(U, V, Q, users, items, neg_users, pos, neg, sneg, tau, lam, divide_by_p=True):
    """U (nu, d), V (ni, d), Q (B, d); users, items, neg_users (B,), pos (B, P), neg (B, P, N), sneg (B, S) int64.
    Returns (L_c, L_s, L_r1, L_r2, total).  ``divide_by_p=False`` leaves the 1/P out (what a test tells apart)."""

    def c(q, v):
        return (q * v).sum(-1) / (tau * q.norm(dim=-1) * v.norm(dim=-1))

    def nce(cpos, cneg):
        return (torch.logsumexp(torch.cat([cpos.unsqueeze(-1), cneg], -1), -1) - cpos).sum()

    L_c = nce(c(Q[:, None], V[pos]), c(Q[:, None, None], V[neg]))
    if divide_by_p:
        L_c = L_c / pos.shape[1]
    L_s = nce(c(Q, V[items]), c(Q[:, None], V[sneg]))
    uu, uk, vi = U[users], U[neg_users], V[items]
    L_r1 = F.softplus(-((vi * uu).sum(1) - (vi * uk).sum(1))).sum()
    L_r2 = F.softplus(-((Q * uu).sum(1) - (Q * uk).sum(1))).sum()
    return L_c, L_s, L_r1, L_r2, lam * (L_c + L_s) + (1 - lam) * (L_r1 + L_r2)


def step(U, V, Q, users, items, neg_users, pos, neg, sneg, tau, lam, dtype=torch.float64, divide_by_p=True):
    """One step on leaf copies of the fp32 inputs in ``dtype``.  Returns (terms (5,), dU, dV, dQ) as numpy float64."""
    U, V, Q = (t.detach().cpu().to(dtype).requires_grad_() for t in (U, V, Q))
    ids = [t.cpu().long() for t in (users, items, neg_users, pos, neg, sneg)]
    terms = loss_terms(U, V, Q, *ids, tau, lam, divide_by_p)
    gU, gV, gQ = torch.autograd.grad(terms[4], (U, V, Q), allow_unused=True)
    z = lambda g, t: (torch.zeros_like(t) if g is None else g).double().numpy()
    return np.array([float(t.detach()) for t in terms]), z(gU, U), z(gV, V), z(gQ, Q)


class Learner(nn.Module):
    """The parameters in the reference's construction order (the global generator's stream fixes the tables): the
    attribute tensors and both tables uninitialised, the two Linear layers (whose constructors draw), then xavier_normal_
    over the attribute tensors, the tables and the two Linear weights."""

    EPS = 1e-8

    def __init__(self, data, width=64, attr_dim=64, hidden=64):
        super().__init__()
        content = torch.as_tensor(np.asarray(data.mapped_item_content), dtype=torch.float32)
        self.sentinel = float((content == -1).float().mean()) > 0.01
        self.attr_matrix = nn.Parameter(torch.empty(data.item_content_dim, attr_dim))
        self.attr_W1 = nn.Parameter(torch.empty(attr_dim, attr_dim))
        self.attr_b1 = nn.Parameter(torch.empty(attr_dim, 1))
        self.attr_W2 = nn.Parameter(torch.empty(attr_dim, 1))
        self.user_emb = nn.Parameter(torch.empty(data.user_num, width))
        self.item_emb = nn.Parameter(torch.empty(data.item_num, width))
        self.gen_layer1 = nn.Linear(attr_dim, hidden)
        self.gen_layer2 = nn.Linear(hidden, width)
        for p in (self.attr_matrix, self.attr_W1, self.attr_W2, self.attr_b1, self.user_emb, self.item_emb,
                  self.gen_layer1.weight, self.gen_layer2.weight):
            nn.init.xavier_normal_(p)

    def encoder(self, attribute):
        """Attention over the item's attributes (a -1 marks a missing value when more than 1 % are), gated by their
        magnitude; an item without an active attribute falls back to the plain attention weights."""
        valid = attribute != -1 if self.sentinel else torch.ones_like(attribute, dtype=torch.bool)
        value = attribute.masked_fill(~valid, 0.0)
        z = torch.matmul(torch.matmul(self.attr_matrix, self.attr_W1) + self.attr_b1.squeeze(), self.attr_W2).squeeze(1)
        mag = value.abs()
        active = valid & (mag > self.EPS)
        has = active.any(1, keepdim=True)
        logits = z.unsqueeze(0).expand(attribute.shape[0], -1) + torch.log(mag.clamp_min(self.EPS))
        w = torch.softmax(logits.masked_fill(~torch.where(has, active, valid), -1e6), 1)
        emb = torch.matmul(torch.where(has, w * value, w), self.attr_matrix)
        return self.gen_layer2(F.leaky_relu(self.gen_layer1(emb)))


def run(data, dtype, width=64, epochs=2, bs=512, P=3, N=8, S=8, tau=0.1, lam=0.6, lr=1e-3, seed=2024):
    """The whole training run (no evaluation) on the global random streams: set_seed, the modules, then per epoch the
    samples from CPython's stream (the positives from NumPy's).  Returns dict(losses (steps, 5), U0_crc, V0_crc, snaps =
    per epoch (U, V, cold = the generated rows of the cold items) as the trainer would snapshot them)."""
    from coldrec_amd.util.utils import set_seed
    set_seed(seed, False)
    m = Learner(data, width, width, width)
    rec = dict(U0_crc=crc(m.user_emb.detach().numpy()), V0_crc=crc(m.item_emb.detach().numpy()))
    m = m.to(dtype)
    content = torch.as_tensor(np.asarray(data.mapped_item_content), dtype=torch.float32).to(dtype)
    opt = torch.optim.Adam(m.parameters(), lr=lr)
    losses, snaps, s = [], [], data.sampler
    for _ in range(epochs):
        s.pull_python_state()
        s.pull_numpy_state()                            # (the positives come from NumPy's global stream)
        ep = s.epoch_ccfcrec(P, N, S)
        s.push_numpy_state()
        s.push_python_state()
        for lo in range(0, ep[0].shape[0], bs):
            u, i, k, pos, neg, sneg = (torch.from_numpy(a[lo:lo + bs]).long() for a in ep)
            terms = loss_terms(m.user_emb, m.item_emb, m.encoder(content[i]), u, i, k, pos, neg, sneg, tau, lam)
            opt.zero_grad()
            terms[4].backward()
            opt.step()
            losses.append([float(t.detach()) for t in terms])
        with torch.no_grad():
            cold = m.encoder(content[torch.as_tensor(data.mapped_cold_item_idx, dtype=torch.long)])
        snaps.append((m.user_emb.detach().double().numpy().copy(), m.item_emb.detach().double().numpy().copy(),
                      cold.double().numpy()))
    rec.update(losses=np.array(losses, np.float64), snaps=snaps)
    return rec
