"""Restatement of DUIF's step and of a whole DUIF run in plain torch (any dtype, runs anywhere), written from the
formulas.  T (n_free, d) the trained table of the side without content, C (n_content, c) the content rows, W (d, c) the
projection (nn.Linear's layout); bpr(x) = -log(1e-5 + sigmoid(x)); every mean over the B records:

    item mode  U = T[users],  H = C[pos ++ neg] W^T,  P = H[:B],  N = H[B:]
    user mode  U = H = C[users] W^T,  P = T[pos],  N = T[neg]
    x = <U, P> - <U, N>,  L_bpr = mean bpr(x),  R = reg (|U|_F + |P|_F + |N|_F) / B,  total = L_bpr + R

Gradients come from autograd: dense for T (index_put accumulates duplicate ids), (d, c) for W.
"""
import functools
import json

import numpy as np
import torch
import torch.nn as nn

from tests.gar_restate import bpr, toy_data        # noqa: F401  (G28 uses G24's splits: make_dataset("toy", cold, seed=1))

REG = 1e-4                                          # the reference's default, G28's


def loss_terms(T, C, W, users, pos, neg, reg, cold_user):
    """(L_bpr, R, total, H)."""
    B = users.shape[0]
    if cold_user:
        H = C[users] @ W.T
        U, P, N = H, T[pos], T[neg]
    else:
        H = C[torch.cat([pos, neg])] @ W.T
        U, P, N = T[users], H[:B], H[B:]
    L = bpr((U * P).sum(1) - (U * N).sum(1)).mean()
    R = reg * sum(torch.norm(t, p=2) / t.shape[0] for t in (U, P, N))
    return L, R, L + R, H


def step(T, C, W, users, pos, neg, reg, cold_user, dtype=torch.float64):
    """One step on leaf copies of the fp32 inputs in ``dtype``.  Returns (loss3, d T, d W, H) as numpy float64."""
    T, C, W = (t.detach().cpu().to(dtype) for t in (T, C, W))
    T, W = T.requires_grad_(), W.requires_grad_()
    ids = [t.cpu().long() for t in (users, pos, neg)]
    terms = loss_terms(T, C, W, *ids, reg, cold_user)
    grads = torch.autograd.grad(terms[2], (T, W), allow_unused=True)
    z = lambda g, t: (torch.zeros_like(t) if g is None else g).double().numpy()
    return (np.array([float(t.detach()) for t in terms[:3]]),) + tuple(z(g, t) for g, t in zip(grads, (T, W))) + \
        (terms[3].detach().double().numpy(),)


def init(nu, ni, content_dim, d):
    """(user table, item table, W) in the reference's draw order on the global CPU stream: xavier_uniform_ for the user
    table, then for the item table, then the nn.Linear's default initialisation."""
    user = nn.init.xavier_uniform_(torch.empty(nu, d))
    item = nn.init.xavier_uniform_(torch.empty(ni, d))
    return user, item, nn.Linear(content_dim, d, bias=False).weight.detach().clone()


def run(data, dtype, cold_user, width=64, epochs=2, bs=512, lr=1e-3, reg=REG, seed=2024):
    """The whole training run (no evaluation) on the global random streams.  One torch.optim.Adam over the free table and
    W (dense: a row no batch touches still moves by its moments).  Returns dict(init = (user table, item table, W)
    (float32), terms (steps, 3) = [bpr, reg, batch_loss], trained = (free table, W) at the end, snaps = per epoch (free
    table, W), touched = the free table's rows some batch gathered)."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    set_seed(seed, False)
    content = np.asarray(data.mapped_user_content if cold_user else data.mapped_item_content)
    first = init(data.user_num, data.item_num, content.shape[1], width)
    content = torch.as_tensor(content, dtype=torch.float32).to(dtype)
    T = nn.Parameter(first[1 if cold_user else 0].to(dtype).clone())
    W = nn.Parameter(first[2].to(dtype).clone())
    opt = torch.optim.Adam([T, W], lr=lr)
    touched = np.zeros(T.shape[0], bool)
    terms, snaps = [], []
    for _ in range(epochs):
        eu, ei, ej = (torch.from_numpy(x).long() for x in epoch_triples(data, bs))
        for t in ((ei, ej) if cold_user else (eu,)):
            touched[t.numpy()] = True
        for lo in range(0, eu.shape[0], bs):
            t = loss_terms(T, content, W, eu[lo:lo + bs], ei[lo:lo + bs], ej[lo:lo + bs], reg, cold_user)
            opt.zero_grad()
            t[2].backward()
            opt.step()
            terms.append([float(x.detach()) for x in t[:3]])
        snaps.append(tuple(x.detach().double().numpy().copy() for x in (T, W)))
    return dict(init=tuple(t.numpy().copy() for t in first), terms=np.array(terms, np.float64), trained=snaps[-1], snaps=snaps,
                touched=touched)


@functools.lru_cache(maxsize=None)
def restated_run(cold, dtype):
    """The restatement's whole run, computed once per cold object and dtype and shared (callers leave it unchanged).  On
    one thread: torch's multi-threaded CPU reductions change their order from run to run; one thread gives the same bits."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return run(toy_data(cold), dtype, cold == "user")
    finally:
        torch.set_num_threads(threads)


# ---- the G28 fixtures ---------------------------------------------------------------------------------------------------

def keys_of(fx, cold_user):
    """(index of the free table, index of W) among the fixture's parameters (named_parameters() order)."""
    names = json.loads(str(fx["param_names"]))
    return (names.index("embedding_dict." + ("item_emb" if cold_user else "user_emb")),
            names.index(("user" if cold_user else "item") + "_projector.weight"))


def init_of(fx, cold_user):
    """The fixture's initial (user table, item table, W)."""
    names = json.loads(str(fx["param_names"]))
    return tuple(fx[f"init_{names.index(n)}"] for n in ("embedding_dict.user_emb", "embedding_dict.item_emb",
                                                          ("user" if cold_user else "item") + "_projector.weight"))


def trained_of(fx, cold_user):
    return tuple(fx[f"trained_{k}"] for k in keys_of(fx, cold_user))


def best_of(fx, cold_user):
    """The best epoch's (free table, W) of the fixture: stored apart only where the best epoch is not the last."""
    return tuple(fx[("trained_" if bool(fx["best_is_last"]) else "best_") + str(k)] for k in keys_of(fx, cold_user))


def ranked_of(fx, cold_user):
    """dict(user_emb, item_emb) = the fixture's best-epoch pair beside the fixture's lists: what
    tests.test_gar_gpu.lists_vs_reference takes."""
    free, proj = best_of(fx, cold_user)[0], fx["best_proj"]
    out = {k: fx[k] for k in fx.files}
    out.update(user_emb=proj if cold_user else free, item_emb=free if cold_user else proj)
    return out


def run_distances(fx, cold_user, terms, best, trained):
    """Against G28: (worst |term - G28's| / G28's batch_loss over the steps, [|best tensor - G28's| / its scale for the free
    table and W], [the same for the trained two])."""
    want = fx["terms"]
    assert terms.shape == want.shape
    rel = float((np.abs(terms - want) / np.abs(want[:, -1:])).max())
    dist = lambda t, w: float(np.abs(np.asarray(t, np.float64) - w).max() / np.abs(w).max())
    return (rel, [dist(t, w) for t, w in zip(best, best_of(fx, cold_user))],
            [dist(t, w) for t, w in zip(trained, trained_of(fx, cold_user))])


# ---- the cases of the kernel tests (tests/test_duif.py measures the float32 formula at them, tests/test_duif_gpu.py the
# kernel) --------------------------------------------------------------------------------------------------------------

# B, d, c, nu, ni.  "chunks": item mode 3 users with 2 chunk + 1 records each; user mode four of 5 items with 2 chunk + 1 of
# the 2 B occurrences and the fifth with 4 chunk + 2.  ("parts", k): B such that the weight gradient has k partials, k = 1,
# 2 and one more than a first-stage chunk of them, asked of the library (``parts_batch``).
CASES = [(1, 4, 1, 11, 11), (7, 256, 7, 11, 13), (33, 68, 33, 11, 30), (2048, 64, 16, 300, 500), (512, 64, 206, 300, 500),
         (512, 128, 300, 300, 500), ("chunks", 64, 16, 40, 60), (("parts", "1"), 8, 5, 40, 60), (("parts", "2"), 8, 5, 40, 60),
         (("parts", "chunk+1"), 8, 5, 40, 60)]
MODES = [False, True]                                # cold_user
CASE_REG = 0.01                                      # the cases' reg: G28's 1e-4 would leave R's gradients near rounding
MODE_IDS = lambda m: "user" if m else "item"


def CASE_IDS(c):
    return ("parts-%s" % c[0][1] if isinstance(c[0], tuple) else "B%s" % c[0]) + "-d%d-c%d" % c[1:3]


def parts_batch(which, d, c, cold_user):
    """The largest B with one weight-gradient partial ("1"), the smallest with two ("2") or with one more than a
    first-stage chunk of partials ("chunk+1"): the library's own count decides."""
    from coldrec_amd import ops
    per = 1 if cold_user else 2
    want = {"1": 1, "2": 2, "chunk+1": ops.duif_part_chunk() + 1}[which]
    B = 1
    while ops.duif_parts(per * B, d, c) < want:
        B += 1
    if which == "1":
        while ops.duif_parts(per * (B + 1), d, c) == 1:
            B += 1
    assert ops.duif_parts(per * B, d, c) == want
    return B


def inputs(case, cold_user, chunk=256, seed=0, scale=1.0):
    """(T, C, W, users, pos, neg) on the CPU; ids drawn with repeats; scores of order one at every width."""
    B, d, c, nu, ni = case
    tag = B if isinstance(B, int) else (513 if B == "chunks" else 1000 + len(B[1]))
    g = torch.Generator().manual_seed(2800 + seed + d + 3 * c + 7 * tag + int(cold_user))
    if B == "chunks":
        B = 3 * (2 * chunk + 1)
        users = torch.randint(nu, (B,), generator=g)
        pos, neg = torch.randint(ni, (B,), generator=g), torch.randint(ni, (B,), generator=g)
        if cold_user:
            occ = torch.cat([torch.arange(4).repeat_interleave(2 * chunk + 1), torch.full((4 * chunk + 2,), 4)])
            occ = occ[torch.randperm(2 * B, generator=g)]
            pos, neg = occ[:B].clone(), occ[B:].clone()
        else:
            users = torch.arange(3).repeat_interleave(2 * chunk + 1)[torch.randperm(B, generator=g)]
    else:
        if not isinstance(B, int):
            B = parts_batch(B[1], d, c, cold_user)
        users = torch.randint(nu, (B,), generator=g)
        pos, neg = torch.randint(ni, (B,), generator=g), torch.randint(ni, (B,), generator=g)
    size = scale * (8.0 / d) ** 0.5 * 0.5
    T = torch.randn(ni if cold_user else nu, d, generator=g) * size
    C = torch.randn(nu if cold_user else ni, c, generator=g)
    W = torch.randn(d, c, generator=g) * (size / c ** 0.5)
    return T, C, W, users, pos, neg


EDGE_BASE = (33, 20, 9, 11, 30)


def edge_cases(cold_user):
    """(tag, inputs, reg) of the edges."""
    out = []
    inp = list(inputs(EDGE_BASE, cold_user, seed=1))
    inp[5] = inp[4].clone()                                           # pos == neg in every record: x = 0
    out.append(("pos-is-neg", inp, 0.01))
    out.append(("scores-beyond-30", list(inputs((65, 64, 16, 50, 400), cold_user, seed=2, scale=9.0)), 0.01))
    inp = list(inputs(EDGE_BASE, cold_user, seed=3))
    inp[2] = torch.zeros_like(inp[2])                                 # W = 0: H and its norms are zero
    out.append(("w-zero", inp, 0.01))
    inp = list(inputs(EDGE_BASE, cold_user, seed=4))
    inp[0] = torch.zeros_like(inp[0])                                 # an all-zero free block
    out.append(("free-zero", inp, 0.01))
    inp = list(inputs(EDGE_BASE, cold_user, seed=5))
    nu, ni = EDGE_BASE[3:]
    for t, n in ((inp[3], nu), (inp[4], ni), (inp[5], ni)):           # ids at the first and the last row of both tables
        t[0], t[1] = 0, n - 1
    inp[5][0], inp[5][1] = ni - 1, 0
    out.append(("first-and-last", inp, 0.01))
    inp = list(inputs(EDGE_BASE, cold_user, seed=6))
    inp[4][0], inp[5][0], inp[4][1], inp[5][1] = 7, 8, 9, 7           # item 7: a positive in record 0, a negative in 1
    out.append(("pos-and-neg", inp, 0.01))
    return out


EDGE_TAGS = [(m, k, e[0]) for m in MODES for k, e in enumerate(edge_cases(m))]


def distances(got, want):
    """(worst error of the three loss terms over the total, [error / maximum of d T, d W and H; None where got has none])."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]).max() / abs(want[0][2])
    errs = []
    for g, w in zip(got[1:], want[1:]):
        if g is None:
            errs.append(None)
            continue
        top = np.abs(w).max()
        errs.append(float(np.abs(np.asarray(g, np.float64) - w).max() / top) if top > 0 else float(np.abs(g).max()))
    return float(rel), errs
