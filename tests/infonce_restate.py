"""Restatement of InfoNCE (util/utils.py:61-76) and of its closed-form gradients in plain torch, in the form that never
subtracts two numbers of nearly the same size -- the form csrc/infonce.hip promises to compute.  Any dtype, runs anywhere,
dense N x N matrices.

    Z1 = normalize(V1), Z2 = normalize(V2) (b_cos), S = Z1 Z2^T / tau, D_ij = S_ij - S_ii
    term_i = LSE_i - S_ii = log1p(l_off_i / p_ii),   l_off_i = sum_{j != i} exp(D_ij - m_i),  p_ii = exp(-m_i),
                                                     m_i = max_j D_ij >= 0 (only there to keep exp in range)
    loss   = mean_i term_i
    dZ1_i  = (O_off_i - l_off_i Z2_i) / (l_off_i + p_ii) / (N tau),   O_off_i = sum_{j != i} exp(D_ij - m_i) Z2_j
    dZ2_j  = sum_i Q_ij Z1_i / (N tau),   Q_ij = exp(D_ij - term_i) (i != j),   Q_jj = P_jj - 1 = expm1(-term_j)

and then F.normalize's backward, (g - z (z.g)) / |v| where |v| >= 1e-12 and g / 1e-12 below the clamp (the clamp_min mask
of tests/test_infonce.py::infonce64).  The diagonal never enters l_off or O_off, so where P_ii is within 1e-7 of 1 the row's
gradient -- millions of times smaller than a flat row's -- still carries the relative error of its own products.  Where
p_ii underflows (a diagonal more than ~100 binades under the row's maximum) the term is m_i + log(l_off_i + p_ii), which
cancels nothing there.

float64 is the reference of the GPU tests and of the fuzzer; float32 is their measuring stick: a bar is 8x the distance of
the float32 evaluation from the float64 one on the same inputs.  ``peaked_cases`` are the inputs of the row-by-row tests.
"""
import numpy as np
import torch

EPS = 1e-12            # F.normalize's clamp_min
PII_MIN = 1e-30        # below it l_off / p_ii is not formed (the kernel's row finish switches at the same value)


def _cpu(x, dtype):
    return torch.as_tensor(x).detach().cpu().to(dtype)


def _normalize(v):
    nr = v.norm(dim=1)
    return v / nr.clamp_min(EPS)[:, None], nr


def _normalize_backward(g, z, nr):
    live = (nr >= EPS)[:, None]
    proj = torch.where(live, z * (z * g).sum(1, keepdim=True), torch.zeros_like(g))
    return (g - proj) / nr.clamp_min(EPS)[:, None]


def infonce(v1, v2, tau, b_cos=True, dtype=torch.float64):
    """v1, v2 (N, d): tensors or arrays of any float type.  Returns (row_terms (N,), loss (0-d), g1, g2 (N, d)), CPU
    tensors of ``dtype``: row_terms_i = LSE_i - S_ii, loss their mean, g = d loss / d v."""
    v1, v2 = _cpu(v1, dtype), _cpu(v2, dtype)
    n = v1.shape[0]
    if b_cos:
        (z1, n1), (z2, n2) = _normalize(v1), _normalize(v2)
    else:
        z1, z2 = v1, v2
    s = z1 @ z2.T / tau
    dd = s - s.diagonal()[:, None]
    eye = torch.eye(n, dtype=torch.bool)
    m = dd.max(1).values
    e = torch.exp(dd - m[:, None]).masked_fill(eye, 0.0)
    l_off = e.sum(1)
    pii = torch.exp(-m)
    l = l_off + pii
    safe = pii > PII_MIN
    term = torch.where(safe, torch.log1p(l_off / torch.where(safe, pii, torch.ones_like(pii))), m + torch.log(l))
    loss = term.mean()
    coef = 1.0 / (n * tau)
    g1 = (e @ z2 - l_off[:, None] * z2) / l[:, None] * coef
    q = torch.exp(dd - term[:, None]).masked_fill(eye, 0.0) + torch.diag(torch.expm1(-term))
    g2 = q.T @ z1 * coef
    if b_cos:
        g1, g2 = _normalize_backward(g1, z1, n1), _normalize_backward(g2, z2, n2)
    return term, loss, g1, g2


def autograd(v1, v2, tau, b_cos=True, dtype=torch.float64):
    """The formula as the reference writes it, through torch autograd on the CPU: (loss, g1, g2).  In float32 this is the
    naive evaluation the peaked cases are there to tell from the stable one."""
    import torch.nn.functional as F
    a, b = _cpu(v1, dtype).requires_grad_(), _cpu(v2, dtype).requires_grad_()
    z1, z2 = (F.normalize(a, dim=1), F.normalize(b, dim=1)) if b_cos else (a, b)
    loss = -torch.diag(F.log_softmax((z1 @ z2.T) / tau, dim=1)).mean()
    loss.backward()
    return loss.detach(), a.grad, b.grad


def row_rho(got, ref):
    """max over rows of max|got_row - ref_row| / max|ref_row|; a row the reference leaves all zero counts with its own
    largest entry (so it has to be zero)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    top = np.abs(ref).max(1)
    err = np.abs(got - ref).max(1)
    return float((err / np.where(top > 0, top, 1.0)).max())


def one_minus_pii(v1, v2, tau, b_cos=True):
    """1 - P_ii per row from the float64 restatement: -expm1(-term_i)."""
    term = infonce(v1, v2, tau, b_cos)[0]
    return (-torch.expm1(-term)).numpy()


def diag_binades_under_max(v1, v2, tau, b_cos=True):
    """(max_j S_ij - S_ii) / ln 2 per row, from the float64 logits."""
    v1, v2 = _cpu(v1, torch.float64), _cpu(v2, torch.float64)
    if b_cos:
        v1, v2 = _normalize(v1)[0], _normalize(v2)[0]
    s = v1 @ v2.T / tau
    return ((s.max(1).values - s.diagonal()) / np.log(2.0)).numpy()


def _mixed(n, d, seed, share, scale=0.3):
    """The first ``share`` of the rows: v2 = v1 + 0.02 |scale| noise (P_ii ~ 1 at a small tau); the rest independent."""
    g = torch.Generator().manual_seed(seed)
    v1 = torch.randn(n, d, generator=g) * scale
    near = v1 + torch.randn(n, d, generator=g) * (0.02 * abs(scale))
    indep = torch.randn(n, d, generator=g) * scale
    k = int(round(n * share))
    v2 = torch.cat([near[:k], indep[k:]])
    return v1.contiguous(), v2.contiguous()


def peaked_cases():
    """name -> (v1, v2, tau, peaked rows (bool mask)): the batches judged row by row (b_cos on)."""
    out = {}
    for name, n, d, tau, share, seed in (("mixed-256x64", 256, 64, 0.04, 0.5, 4), ("mixed-130x132", 130, 132, 0.05, 0.5, 1),
                                         ("peaked-256x64", 256, 64, 0.04, 1.0, 7), ("peaked-64x32", 64, 32, 0.05, 1.0, 5)):
        v1, v2 = _mixed(n, d, seed, share)
        out[name] = (v1, v2, tau, torch.arange(n) < int(round(n * share)))
    # anti-aligned: independent rows, 8 of them with v2_i = -v1_i: S_ii = -1 / tau = -100 against a row maximum of about +40
    v1, v2 = _mixed(64, 32, 105, 0.0)
    anti = torch.arange(40, 48)
    v2[anti] = -v1[anti]
    out["anti-64x32"] = (v1, v2.contiguous(), 0.01, torch.zeros(64, dtype=torch.bool))
    return out
