"""Float64 restatements for the SimGCL / XSimGCL tests (pure numpy / torch, runs anywhere): the Philox4x32-10 uniforms of
crh_noise_uniform_f32, the row perturbation of crh_perturb_rows_f32, and one training step / a whole run of both models
written from their formulas:

    encoder   x_k = A x_{k-1};  perturbed: x_k += sign(x_k) * normalize(r_k, dim=-1) * eps (r_k uniform, the perturbed
              x_k feeds the next layer);  output = mean(x_1 .. x_L)
    bpr       mean(-log(1e-5 + sigmoid(u.p - u.n)))         l2 = reg * (|u|_F / B + |p|_F / B)
    InfoNCE   -mean(diag(log_softmax(normalize(v1) normalize(v2)^T / tau, dim=1)))
    SimGCL    bpr + l2 on the clean pass + cl_rate * (nce(V1[uu], V2[uu]) + nce(V1[ii], V2[ii])), V1, V2 two perturbed passes
    XSimGCL   one perturbed pass; bpr + l2 on its mean OUT; cl_rate * (nce(OUT[uu], CL[uu]) + nce(OUT[ii], CL[ii])), CL = x_{l_cl}
    Adam      torch.optim.Adam(lr) on the (U + I, d) table

Gradients come from autograd in float64 (sign() has no gradient, the noise is a constant).
"""
import zlib

import numpy as np
import torch

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox_uniform(n_rows: int, d: int, seed: int, draw: int) -> np.ndarray:
    """(n_rows, d) float32 uniforms in [0, 1): Philox4x32-10, key = (seed lo, seed hi), counter = (g lo, g hi, draw lo,
    draw hi) with g = row * (d/4) + c/4; output word j -> column 4 * (c/4) + j; u = (word >> 8) * 2^-24."""
    g = np.arange(n_rows * (d // 4), dtype=np.uint64)
    c = [g & MASK, g >> np.uint64(32), np.full_like(g, draw & MASK), np.full_like(g, (draw >> 32) & MASK)]
    k0, k1 = seed & MASK, (seed >> 32) & MASK
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(M0), c[2] * np.uint64(M1)          # 32 x 32 -> 64 bit products
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & MASK, p1 >> np.uint64(32), p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    words = np.stack(c, 1).reshape(n_rows, d)
    return ((words >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def perturb_f64(y: np.ndarray, r: np.ndarray, eps: float) -> np.ndarray:
    """y + sign(y) * r / max(|r|_2, 1e-12) * eps per row, in float64."""
    y, r = y.astype(np.float64), r.astype(np.float64)
    nrm = np.maximum(np.sqrt((r * r).sum(1, keepdims=True)), 1e-12)
    return y + np.sign(y) * (r / nrm) * eps


def crc(*arrays) -> int:
    c = 0
    for a in arrays:
        c = zlib.crc32(np.ascontiguousarray(a).tobytes(), c)
    return c


def dense_adj(data) -> torch.Tensor:
    return torch.from_numpy(np.asarray(data.norm_adj.todense(), dtype=np.float64))


def _nce(v1, v2, tau):
    z1, z2 = torch.nn.functional.normalize(v1, dim=1), torch.nn.functional.normalize(v2, dim=1)
    return -torch.diag(torch.log_softmax(z1 @ z2.T / tau, dim=1)).mean()


def _encode(A, E, L, noise=None, eps=0.0):
    """Returns (mean of the layers, list of the layer outputs); ``noise``: a callable giving the next (N, d) uniforms."""
    x, layers = E, []
    for _ in range(L):
        x = A @ x
        if noise is not None:
            r = noise().double()
            x = x + torch.sign(x).detach() * torch.nn.functional.normalize(r, dim=-1) * eps
        layers.append(x)
    return torch.stack(layers, 0).mean(0), layers


def step_f64(E, A, U, mode, L, l_cl, eps, tau, cl_rate, reg, u, p, n, noise):
    """One step's loss terms and dE0: E (N, d) float64 with requires_grad; u, p, n int64 index tensors (p, n item ids);
    ``noise()`` gives the next layer's uniforms in the reference's order.  Returns ([bpr, l2, cl_user, cl_item], total)."""
    uu, ii = torch.unique(u), torch.unique(p) + U
    if mode == 'simgcl':
        rec, _ = _encode(A, E, L)
        v1, _ = _encode(A, E, L, noise, eps)
        v2, _ = _encode(A, E, L, noise, eps)
    else:
        rec, layers = _encode(A, E, L, noise, eps)
        v1, v2 = rec, layers[l_cl - 1]
    ue, pe, ne = rec[u], rec[p + U], rec[n + U]
    bpr = (-torch.log(1e-5 + torch.sigmoid((ue * pe).sum(1) - (ue * ne).sum(1)))).mean()
    l2 = reg * (torch.linalg.norm(ue) / ue.shape[0] + torch.linalg.norm(pe) / pe.shape[0])
    cl_u, cl_i = _nce(v1[uu], v2[uu], tau), _nce(v1[ii], v2[ii], tau)
    return [bpr, l2, cl_u, cl_i], bpr + l2 + cl_rate * (cl_u + cl_i)


def host_noise(n_rows, d, record=None):
    """The reference's stream: torch.rand((N, d), float32) from the CPU's global generator, one call per perturbed layer."""
    def f():
        r = torch.rand((n_rows, d), dtype=torch.float32)
        if record is not None and record.get("noise_crc") is None:
            record["noise_crc"] = crc(r.numpy())
        return r
    return f


def run_f64(data, mode, layers, emb_size, epochs, bs, cl_rate, tau, eps, l_cl=1, lr=1e-3, reg=1e-4, seed=2024):
    """The whole training run in float64 on the global random streams (set_seed first, then the xavier tables user
    first, then per epoch the triples from NumPy's stream and per perturbed layer the noise from torch's).  Returns
    dict(losses (steps, 4), noise_crc, U0_crc, V0_crc)."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    set_seed(seed, False)
    init = torch.nn.init.xavier_uniform_
    U0, V0 = init(torch.empty(data.user_num, emb_size)), init(torch.empty(data.item_num, emb_size))
    rec = dict(noise_crc=None, U0_crc=crc(U0.numpy()), V0_crc=crc(V0.numpy()))
    E = torch.cat([U0, V0], 0).double().requires_grad_()
    A = dense_adj(data)
    opt = torch.optim.Adam([E], lr=lr)
    noise = host_noise(E.shape[0], emb_size, rec)
    losses = []
    for _ in range(epochs):
        u, i, j = (torch.from_numpy(np.asarray(t)).long() for t in epoch_triples(data, bs))
        for lo in range(0, u.shape[0], bs):
            terms, total = step_f64(E, A, data.user_num, mode, layers, l_cl, eps, tau, cl_rate, reg, u[lo:lo + bs],
                                    i[lo:lo + bs], j[lo:lo + bs], noise)
            opt.zero_grad()
            total.backward()
            opt.step()
            losses.append([float(t.detach()) for t in terms])
    rec["losses"] = np.array(losses, np.float64)
    return rec
