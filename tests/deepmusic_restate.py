"""Restatement of DeepMusic's loss and of a whole DeepMusic run in plain torch (runs anywhere), twice: the closed form in
float64, written from the formulas, and the reference's way in any dtype, with ``F.mse_loss``, ``torch.norm`` and autograd.
One frozen table T (rows, d), B ids into it, B generated rows G:

    L_mse = sum |T[id_b] - G_b|^2 / (B d)        R = reg |G|_F / B        total = L_mse + R
    dtotal/dG_b = 2 (G_b - T[id_b]) / (B d) + reg G_b / (B |G|_F)         (second part 0 when |G|_F = 0)

Also here: the GPU tests' cases and edges, the distance helpers.  The toy split of G27 is tests/gar_restate.py's toy_data.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests.gar_restate import toy_data  # noqa: F401  (G27's splits are G24's: make_dataset("toy", cold, seed=1))

REG = 1e-2
# (B, d, rows)
CASES = [(1, 4, 11), (2, 4, 11), (37, 20, 30), (63, 64, 50), (65, 252, 300), (300, 256, 11), (2048, 64, 300)]
IDS = lambda c: "B%d-d%d" % c[:2]


def inputs(case, seed=0, scale=0.3):
    """(T, ids, G) on the CPU; ids drawn with repeats."""
    B, d, rows = case
    g = torch.Generator().manual_seed(2750 + seed + d + 7 * B)
    ids = torch.randint(rows, (B,), generator=g)
    return torch.randn(rows, d, generator=g) * scale, ids, torch.randn(B, d, generator=g) * scale


def case_runs():
    """(tag, (T, ids, G), reg) of the cases; reg = 1e-2 x B keeps R a visible share of the total at every B."""
    return [(IDS(c), inputs(c), REG * c[0]) for c in CASES]


def edge_cases():
    """(tag, (T, ids, G), reg) of the edges."""
    out = []
    base = (37, 20, 30)
    out.append(("reg0", inputs(base, seed=1), 0.0))
    T, ids, G = inputs((65, 64, 50), seed=2)
    out.append(("gen-zero", (T, ids, torch.zeros_like(G)), REG * 65))
    T, ids, G = inputs((65, 64, 50), seed=3)
    out.append(("gen-is-table", (T, ids, T[ids].clone()), REG * 65))
    T, ids, G = inputs((63, 64, 50), seed=4)
    ids = ids.clone()
    ids[0], ids[1], ids[61], ids[62] = 0, 49, 49, 0
    out.append(("first-and-last-rows", (T, ids, G), REG * 63))
    T, ids, G = inputs((65, 64, 50), seed=5)
    out.append(("ids-equal", (T, torch.full_like(ids, 17), G), REG * 65))
    return out


def closed_form(T, ids, G, reg):
    """The formulas above in float64, no autograd.  Returns (loss3 = [L_mse, R, total], dtotal/dG (B, d)) as numpy."""
    T, G = T.detach().cpu().double(), G.detach().cpu().double()
    B, d = G.shape
    df = G - T[ids.cpu().long()]
    nrm = float(torch.sqrt((G * G).sum()))
    mse, r = float((df * df).sum()) / (B * d), reg * nrm / B
    grad = 2 * df / (B * d)
    if nrm > 0:
        grad = grad + reg * G / (B * nrm)
    return np.array([mse, r, mse + r]), grad.numpy()


def loss_terms(real, made, reg):
    """The reference's way (model/DeepMusic.py:25, util/utils.py:32-48) on gathered rows and generated rows."""
    mse = F.mse_loss(real, made)
    r = torch.norm(made, p=2) / made.shape[0] * reg
    return mse, r, mse + r


def step(T, ids, G, reg, dtype=torch.float64):
    """One step the reference's way on leaf copies of the fp32 inputs in ``dtype``; ``closed_form``'s returns."""
    T, G = T.detach().cpu().to(dtype), G.detach().cpu().to(dtype).requires_grad_()
    terms = loss_terms(T[ids.cpu().long()], G, reg)
    grad, = torch.autograd.grad(terms[2], G)
    return np.array([float(t.detach()) for t in terms]), grad.double().numpy()


def distances(got, want):
    """(worst error of the three loss terms over the total, gradient error / its maximum)."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]).max() / abs(want[0][2])
    top = np.abs(want[1]).max()
    return rel, float(np.abs(np.asarray(got[1], np.float64) - want[1]).max() / top if top > 0 else np.abs(got[1]).max())


def generator(content_dim, width):
    """Linear -> ReLU -> Linear, both Linear layers with their default initialisation, first layer first."""
    return nn.Sequential(nn.Linear(content_dim, 2 * width), nn.ReLU(), nn.Linear(2 * width, width))


def run(data, loaded_U, loaded_V, dtype, cold_user, closed=False, width=64, epochs=2, bs=512, lr=1e-3, reg=1e-4, seed=2024):
    """The whole training run (no evaluation) on the global random streams: set_seed, the MLP, then per epoch the pairwise
    sampler's triples; Adam over the MLP.  closed: the loss and dtotal/dG from the formulas (written out in ``dtype``, no
    autograd after the MLP) instead of the reference's way.  Returns dict(losses (steps, 3), init / params = the MLP's
    parameters before / after, snaps = per epoch (user_emb, item_emb) as the trainer would snapshot them)."""
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
    losses, snaps = [], []
    for _ in range(epochs):
        eu, ei, _ej = (torch.from_numpy(x).long() for x in epoch_triples(data, bs))
        for lo in range(0, eu.shape[0], bs):
            ids = (eu if cold_user else ei)[lo:lo + bs]
            real, made = (U if cold_user else V)[ids], gen(content[ids])
            opt.zero_grad()
            if closed:
                with torch.no_grad():
                    B, d = made.shape
                    df = made - real
                    nrm = torch.sqrt((made * made).sum())
                    terms = ((df * df).sum() / (B * d), reg * nrm / B)
                    terms = terms + (terms[0] + terms[1],)
                    grad = 2 * df / (B * d) + (reg * made / (B * nrm) if float(nrm) > 0 else 0)
                made.backward(grad)
            else:
                terms = loss_terms(real, made, reg)
                terms[2].backward()
            opt.step()
            losses.append([float(t.detach()) for t in terms])
        with torch.no_grad():
            users, items = U.clone(), V.clone()
            if cold.numel():
                (users if cold_user else items)[cold] = gen(content[cold])
            snaps.append((users.double().numpy().copy(), items.double().numpy().copy()))
    return dict(losses=np.array(losses, np.float64), init=init, params=[p.detach().double().numpy() for p in gen.parameters()],
                snaps=snaps)
