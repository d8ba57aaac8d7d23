"""Restatement of ALDI's loss and of a whole ALDI run in plain torch (any dtype, runs anywhere), written from the
formulas, the B x B product of the identification term included.  Per record the teacher rows Ur = U[u], Pr = V[p],
Nr = V[n], the student towers' outputs gu, gp, gn and the weight wi = w[p]; every mean over the B records:

    L_bpr  = mean(-log(1e-5 + sigmoid(<gu, gp> - <gu, gn>)))
    L_rate = gamma mean(|<Ur, Pr> - <gu, gp>| + |<Ur, Nr> - <gu, gn>|)
    L_rank = alpha mean(wi bce(<gu, gp> - <gu, gn>, sigmoid(<Ur, Pr> - <Ur, Nr>)))
    L_iden = beta  mean(wi bce(|gp|^2 - (gp gn^T).mean(1), sigmoid(|Pr|^2 - (Pr Nr^T).mean(1))))
    total  = L_bpr + L_rate + L_rank + L_iden

Gradients come from autograd; the teacher tables get none.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


def loss_terms(U, V, users, pos, neg, gu, gp, gn, w, alpha, beta, gamma):
    """U (nu, d), V (ni, d), users / pos / neg (B,) int64, gu / gp / gn (B, d), w (ni,).  Returns the five terms."""
    Ur, Pr, Nr, wi = U[users], V[pos], V[neg], w[pos]
    sp, sn = (gu * gp).sum(1), (gu * gn).sum(1)
    tp, tn = (Ur * Pr).sum(1), (Ur * Nr).sum(1)
    bce = lambda x, t: F.binary_cross_entropy_with_logits(x, torch.sigmoid(t), reduction='none')
    L_bpr = torch.mean(-torch.log(10e-6 + torch.sigmoid(sp - sn)))
    L_rate = gamma * torch.mean(torch.abs(tp - sp) + torch.abs(tn - sn))
    L_rank = alpha * (wi * bce(sp - sn, tp - tn)).mean()
    x_iden = (gp * gp).sum(1) - (gp @ gn.t()).mean(1)
    t_iden = (Pr * Pr).sum(1) - (Pr @ Nr.t()).mean(1)
    L_iden = beta * (wi * bce(x_iden, t_iden)).mean()
    return L_bpr, L_rate, L_rank, L_iden, L_bpr + L_rate + L_rank + L_iden


def step(U, V, users, pos, neg, gu, gp, gn, w, alpha, beta, gamma, dtype=torch.float64):
    """One step on leaf copies of the fp32 inputs in ``dtype``.  Returns (terms (5,), d gu, d gp, d gn) as numpy float64."""
    U, V, w = (t.detach().cpu().to(dtype) for t in (U, V, w))
    gu, gp, gn = (t.detach().cpu().to(dtype).requires_grad_() for t in (gu, gp, gn))
    ids = [t.cpu().long() for t in (users, pos, neg)]
    terms = loss_terms(U, V, *ids, gu, gp, gn, w, alpha, beta, gamma)
    grads = torch.autograd.grad(terms[4], (gu, gp, gn), allow_unused=True)
    z = lambda g, t: (torch.zeros_like(t) if g is None else g).double().numpy()
    return (np.array([float(t.detach()) for t in terms]),) + tuple(z(g, t) for g, t in zip(grads, (gu, gp, gn)))


def min_rate_gap(U, V, users, pos, neg, gu, gp, gn):
    """min over the records of min(|tp - sp|, |tn - sn|) in float64: how far L_rate's two signs are from flipping."""
    U, V, gu, gp, gn = (t.double() for t in (U, V, gu, gp, gn))
    Ur, Pr, Nr = U[users.long()], V[pos.long()], V[neg.long()]
    r1 = (Ur * Pr).sum(1) - (gu * gp).sum(1)
    r2 = (Ur * Nr).sum(1) - (gu * gn).sum(1)
    return float(torch.minimum(r1.abs(), r2.abs()).min())


class Tower(nn.Module):
    """Linear -> BatchNorm1d -> tanh -> Linear; both Linear layers draw their default initialisation at construction,
    then the weights are redrawn truncated-normal(std 0.01) and the biases zeroed, first layer first."""

    def __init__(self, n_in, hidden, n_out):
        super().__init__()
        self.fc1, self.bn, self.fc2 = nn.Linear(n_in, hidden), nn.BatchNorm1d(hidden), nn.Linear(hidden, n_out)
        for layer in (self.fc1, self.fc2):
            nn.init.trunc_normal_(layer.weight, std=0.01)
            nn.init.zeros_(layer.bias)

    def forward(self, x):
        return self.fc2(torch.tanh(self.bn(self.fc1(x))))


def item_weights(data, M, tws):
    """The weight table from the builder's DICTS (the trainer restates it on the arrays): per training item the sum over
    its users of 1 / |the user's items|, 1 for an item without training pairs; then min(tanh(a f), tanh(M))."""
    freq = np.ones(data.item_num, np.float32)
    for item, raters in data.training_set_i.items():
        freq[data.item[item]] = sum(1.0 / max(len(data.training_set_u[u]), 1) for u in raters)
    if not tws:
        return freq, np.ones(data.item_num, np.float32)
    n = max(len(data.training_data), 1)
    a = float(M) / ((n / max(data.item_num, 1)) * (1.0 / max(n / max(data.user_num, 1), 1e-12)))
    w = torch.clamp(torch.tanh(a * torch.tensor(freq)), 0.0, float(np.tanh(float(M))))
    return freq, w.numpy()


def run(data, teacher_U, teacher_V, dtype, width=64, hidden=200, epochs=2, bs=512, alpha=0.9, beta=0.05, gamma=0.1, tws=1,
        M=4.0, lr=1e-3, reg=1e-4, seed=2024):
    """The whole training run (no evaluation) on the global random streams: set_seed, the user tower, the item tower, then
    per epoch the pairwise sampler's triples.  Returns dict(losses (steps, 5), snaps = per epoch (cold_user_emb, item_emb)
    as the trainer would snapshot them, towers in eval mode)."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    set_seed(seed, False)
    ut, it = Tower(width, hidden, width), Tower(data.item_content_dim, hidden, width)
    ut, it = ut.to(dtype), it.to(dtype)
    U, V = torch.as_tensor(teacher_U).to(dtype), torch.as_tensor(teacher_V).to(dtype)
    content = torch.as_tensor(np.asarray(data.mapped_item_content), dtype=torch.float32).to(dtype)
    w = torch.as_tensor(item_weights(data, M, tws)[1]).to(dtype)
    decay = [p for t in (ut, it) for p in (t.fc1.weight, t.fc1.bias, t.fc2.weight, t.fc2.bias)]
    plain = [p for t in (ut, it) for p in (t.bn.weight, t.bn.bias)]
    opt = torch.optim.Adam([dict(params=plain, weight_decay=0.0), dict(params=decay, weight_decay=reg)], lr=lr)
    cold = torch.as_tensor(np.asarray(data.mapped_cold_item_idx), dtype=torch.long)
    losses, snaps = [], []
    for _ in range(epochs):
        ut.train(), it.train()
        eu, ei, ej = (torch.from_numpy(x).long() for x in epoch_triples(data, bs))
        for lo in range(0, eu.shape[0], bs):
            u, p, n = eu[lo:lo + bs], ei[lo:lo + bs], ej[lo:lo + bs]
            terms = loss_terms(U, V, u, p, n, ut(U[u]), it(content[p]), it(content[n]), w, alpha, beta, gamma)
            opt.zero_grad()
            terms[4].backward()
            opt.step()
            losses.append([float(t.detach()) for t in terms])
        with torch.no_grad():
            ut.eval(), it.eval()
            items = V.clone()
            items[cold] = it(content[cold])
            snaps.append((ut(U).double().numpy().copy(), items.double().numpy().copy()))
    return dict(losses=np.array(losses, np.float64), snaps=snaps)
