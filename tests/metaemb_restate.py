"""Restatement of MetaEmbedding's loss and of a whole MetaEmbedding run in plain torch (runs anywhere), twice: the closed
form in float64, written from the formulas, and the reference's way in any dtype, with autograd and ``autograd.grad``.
One frozen table T (rows, d), N ids into it, N generated rows E, targets t_n = 1 for n < n_pos and 0 after; o_n = T[id_n],
bce(y, t) = max(y, 0) - t y + log1p(exp(-|y|)), s = sigmoid:

    y_a,n = <o_n, E_n>                       L_a = (1/N) sum bce(y_a,n, t_n)
    g_n   = (s(y_a,n) - t_n) o_n / N         (a constant)
    y_b,n = <o_n, E_n - cold_lr g_n>         L_b = (1/N) sum bce(y_b,n, t_n)
    ME    = alpha L_a + (1 - alpha) L_b
    dME/dE_n = [alpha (s(y_a,n) - t_n) + (1 - alpha) (s(y_b,n) - t_n)] o_n / N

Also here: the toy split of G27, the GPU tests' cases and edges, the distance helpers.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gar_restate import toy_data  # noqa: F401  (G27's splits are G24's: make_dataset("toy", cold, seed=1))

ALPHA = 0.3
# (N, d, rows)
CASES = [(1, 4, 11), (2, 4, 11), (37, 20, 30), (63, 64, 50), (65, 252, 300), (300, 256, 11), (2048, 64, 300)]
IDS = lambda c: "N%d-d%d" % c[:2]


def inputs(case, seed=0, scale=0.3):
    """(T, ids, E) on the CPU; ids drawn with repeats."""
    N, d, rows = case
    g = torch.Generator().manual_seed(2700 + seed + d + 7 * N)
    ids = torch.randint(rows, (N,), generator=g)
    return torch.randn(rows, d, generator=g) * scale, ids, torch.randn(N, d, generator=g) * scale


def case_runs():
    """(tag, (T, ids, E), n_pos, alpha, cold_lr) of the cases: n_pos = N / 2 (N = 1: 0 and 1); cold_lr = N / 4, so that the
    inner step moves a score by (s(y_a) - t) |o|^2 / 4, the order of the score itself."""
    out = []
    for c in CASES:
        for n_pos in ((0, 1) if c[0] == 1 else (c[0] // 2,)):
            out.append((IDS(c) + ("-pos%d" % n_pos if c[0] == 1 else ""), inputs(c), n_pos, ALPHA, c[0] / 4.))
    return out


def mean_oo(T, ids):
    return float((T.double()[ids] ** 2).sum(1).mean())


def edge_cases():
    """(tag, (T, ids, E), n_pos, alpha, cold_lr) of the edges."""
    out = []
    base = (37, 20, 30)
    for a in (0.0, 1.0):
        out.append((f"alpha{a:g}", inputs(base, seed=1), 18, a, 37 / 4.))
    out.append(("coldlr0", inputs(base, seed=2), 18, ALPHA, 0.0))
    for order in (1, 10):                                             # cold_lr mean|o|^2 / N = 1, 10
        inp = inputs((63, 64, 50), seed=3)
        out.append((f"step-order-{order}", inp, 31, ALPHA, order * 63 / mean_oo(inp[0], inp[1])))
    out.append(("scores-beyond-30", inputs((65, 64, 50), seed=4, scale=2.0), 32, ALPHA, 1e-2))
    out.append(("scores-beyond-90", inputs((65, 64, 50), seed=5, scale=4.0), 32, ALPHA, 1e-2))
    T, ids, E = inputs(base, seed=6)
    out.append(("emb-zero", (T, ids, torch.zeros_like(E)), 18, ALPHA, 37 / 4.))
    out.append(("npos-0", inputs(base, seed=7), 0, ALPHA, 37 / 4.))
    out.append(("npos-N", inputs(base, seed=8), 37, ALPHA, 37 / 4.))
    T, ids, E = inputs((63, 64, 50), seed=9)
    ids = ids.clone()
    ids[0], ids[1], ids[61], ids[62] = 0, 49, 49, 0
    out.append(("first-and-last-rows", (T, ids, E), 31, ALPHA, 63 / 4.))
    T, ids, E = inputs((65, 64, 50), seed=10)
    out.append(("ids-equal", (T, torch.full_like(ids, 17), E), 32, ALPHA, 65 / 4.))
    return out


def _bce64(y, t):
    return torch.clamp(y, min=0) - t * y + torch.log1p(torch.exp(-y.abs()))


def closed_form(T, ids, E, n_pos, alpha, cold_lr):
    """The formulas above in float64, no autograd.  Returns (loss3 = [L_a, L_b, ME], dME/dE (N, d), scores (2, N)) as numpy."""
    T, E = T.detach().cpu().double(), E.detach().cpu().double()
    o = T[ids.cpu().long()]
    N = o.shape[0]
    t = (torch.arange(N) < n_pos).double()
    ya = (o * E).sum(1)
    ka = torch.sigmoid(ya) - t
    g = ka[:, None] * o / N
    yb = (o * (E - cold_lr * g)).sum(1)
    kb = torch.sigmoid(yb) - t
    la, lb = _bce64(ya, t).mean(), _bce64(yb, t).mean()
    grad = (alpha * ka + (1 - alpha) * kb)[:, None] * o / N
    return np.array([float(la), float(lb), float(alpha * la + (1 - alpha) * lb)]), grad.numpy(), torch.stack([ya, yb]).numpy()


def loss_terms(o, E, n_pos, alpha, cold_lr):
    """The reference's way (model/MetaEmbedding.py:28-44, 168-203) on gathered rows o (N, d) and generated rows E with a
    graph: two forward passes, ``autograd.grad`` without create_graph in between.  Returns (L_a, L_b, ME, y_a, y_b)."""
    N = o.shape[0]
    t = (torch.arange(N, device=o.device) < n_pos).to(E.dtype)
    ya = torch.sum(o * E, 1)
    la = torch.mean(F.binary_cross_entropy_with_logits(ya, t))
    g = torch.autograd.grad(la, E, retain_graph=True)[0]
    yb = torch.sum(o * (E - cold_lr * g), 1)
    lb = torch.mean(F.binary_cross_entropy_with_logits(yb, t))
    return la, lb, la * alpha + lb * (1 - alpha), ya, yb


def step(T, ids, E, n_pos, alpha, cold_lr, dtype=torch.float64):
    """One step the reference's way on leaf copies of the fp32 inputs in ``dtype``; ``closed_form``'s returns."""
    T, E = T.detach().cpu().to(dtype), E.detach().cpu().to(dtype).requires_grad_()
    la, lb, me, ya, yb = loss_terms(T[ids.cpu().long()], E, n_pos, alpha, cold_lr)
    grad, = torch.autograd.grad(me, E)
    return (np.array([float(la.detach()), float(lb.detach()), float(me.detach())]), grad.double().numpy(),
            torch.stack([ya, yb]).detach().double().numpy())


def distances(got, want):
    """(worst error of the three loss terms over the total, gradient error / its maximum, score error / the largest score)."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]).max() / abs(want[0][2])
    out = [rel]
    for g, w in zip(got[1:], want[1:]):
        top = np.abs(w).max()
        out.append(float(np.abs(np.asarray(g, np.float64) - w).max() / top if top > 0 else np.abs(g).max()))
    return tuple(out)


def generator(content_dim, width):
    return nn.Linear(content_dim, width)


def run(data, loaded_U, loaded_V, dtype, cold_user, closed=False, width=64, epochs=2, bs=512, alpha=0.5, lr=1e-3,
        seed=2024):
    """The whole training run (no evaluation) on the global random streams: set_seed, the generator, then per epoch the
    pairwise sampler's triples; Adam over the generator.  closed: the loss and dME/dE from ``closed_form``'s formulas
    (written out in ``dtype``, no autograd after the generator) instead of the reference's way.  Returns dict(losses
    (steps, 3), init / params = the generator's parameters before / after, snaps = per epoch (user_emb, item_emb) as the
    trainer would snapshot them)."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    set_seed(seed, False)
    content = data.mapped_user_content if cold_user else data.mapped_item_content
    gen = generator(data.user_content_dim if cold_user else data.item_content_dim, width)
    init = [p.detach().numpy().copy() for p in gen.parameters()]
    gen = gen.to(dtype)
    content = torch.as_tensor(np.asarray(content), dtype=torch.float32).to(dtype)
    U, V = torch.as_tensor(loaded_U).to(dtype), torch.as_tensor(loaded_V).to(dtype)
    opt = torch.optim.Adam(gen.parameters(), lr=lr)
    cold = torch.as_tensor(np.asarray(data.mapped_cold_user_idx if cold_user else data.mapped_cold_item_idx), dtype=torch.long)
    cold_lr = lr / 10.
    losses, snaps = [], []
    for _ in range(epochs):
        eu, ei, ej = (torch.from_numpy(x).long() for x in epoch_triples(data, bs))
        for lo in range(0, eu.shape[0], bs):
            uu, ii = torch.cat([eu[lo:lo + bs]] * 2), torch.cat([ei[lo:lo + bs], ej[lo:lo + bs]])
            o, own, n_pos = (V[ii], uu, uu.shape[0] // 2) if cold_user else (U[uu], ii, uu.shape[0] // 2)
            E = gen(content[own]) / 5.
            opt.zero_grad()
            if closed:
                N = o.shape[0]
                t = (torch.arange(N) < n_pos).to(dtype)
                with torch.no_grad():
                    ya = (o * E).sum(1)
                    ka = torch.sigmoid(ya) - t
                    yb = (o * (E - cold_lr * (ka[:, None] * o / N))).sum(1)
                    kb = torch.sigmoid(yb) - t
                    la, lb = _bce64(ya, t).mean(), _bce64(yb, t).mean()
                    me = alpha * la + (1 - alpha) * lb
                    grad = (alpha * ka + (1 - alpha) * kb)[:, None] * o / N
                E.backward(grad)
            else:
                la, lb, me, _, _ = loss_terms(o, E, n_pos, alpha, cold_lr)
                me.backward()
            opt.step()
            losses.append([float(la.detach()), float(lb.detach()), float(me.detach())])
        with torch.no_grad():
            users, items = U.clone(), V.clone()
            if cold.numel():
                (users if cold_user else items)[cold] = gen(content[cold]) / 5.
            snaps.append((users.double().numpy().copy(), items.double().numpy().copy()))
    return dict(losses=np.array(losses, np.float64), init=init, params=[p.detach().double().numpy() for p in gen.parameters()],
                snaps=snaps)


def param_distances(fx, params):
    """|parameter - G27's| / G27's scale of every trained generator parameter."""
    return [float(np.abs(np.asarray(p, np.float64) - fx[f"gen_final_{k}"]).max() / np.abs(fx[f"gen_final_{k}"]).max())
            for k, p in enumerate(params)]
