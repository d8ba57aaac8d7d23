"""float64 restatement of NGCF (NumPy, CPU), written from the formulas and not from any implementation:

  x_0 = [user table; item table] (N x d), c = 1 / (L + 1); for k = 1..L
      s_k = A x_{k-1}
      z_k = s_k Wgc_k^T + bgc_k + (x_{k-1} * s_k) Wbi_k^T + bbi_k         (nn.Linear layout: W is (out, in))
      x_k = leaky_relu(z_k, 0.01)
  OUT = c (x_0 + ... + x_L)

  backward, g_L = c dOUT, slope(z) = 1 if z > 0 else 0.01 (z == 0 takes 0.01; sign(x_k) = sign(z_k)):
      dz = g_k * slope ; dWgc = dz^T s_k ; dWbi = dz^T (x_{k-1} * s_k) ; dbgc = dbbi = column sums of dz
      T = dz Wbi ; ds = dz Wgc + x_{k-1} * T ; g_{k-1} = c dOUT + s_k * T + A ds        (A symmetric) ; dE_0 = g_0

  loss = mean_b -log(1e-5 + sigmoid(<u_b, p_b> - <u_b, n_b>)) + reg (|U_B|_F + |P_B|_F + |N_B|_F) / B on OUT's rows.

``weights``: L tuples (Wgc, bgc, Wbi, bbi).  ``A``: anything with ``@`` (dense ndarray or scipy sparse), symmetric."""
import numpy as np

SLOPE = 0.01


def f64(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float64)


def layer_fwd(x, s, wgc, bgc, wbi, bbi):
    z = s @ wgc.T + bgc + (x * s) @ wbi.T + bbi
    return np.where(z > 0, z, SLOPE * z)


def layer_bwd(x, s, xk, g, dout, c, wgc, wbi):
    """(ds, local, dWgc, dWbi, db) with local = c dout + s * T; g None = c dout (the top layer)."""
    if g is None:
        g = c * dout
    dz = g * np.where(xk > 0, 1.0, SLOPE)
    t = dz @ wbi
    return dz @ wgc + x * t, c * dout + s * t, dz.T @ s, dz.T @ (x * s), dz.sum(0)


def encoder_fwd(e0, a, weights):
    """OUT and the kept (x_{k-1}, s_k, x_k) per layer."""
    c = 1.0 / (len(weights) + 1)
    x, acc, kept = e0, e0.copy(), []
    for wgc, bgc, wbi, bbi in weights:
        s = np.asarray(a @ x)
        xk = layer_fwd(x, s, wgc, bgc, wbi, bbi)
        kept.append((x, s, xk))
        acc = acc + xk
        x = xk
    return acc * c, kept


def encoder_bwd(dout, a, weights, kept):
    """(dE_0, [(dWgc, db, dWbi, db)] per layer) from dOUT."""
    c = 1.0 / (len(weights) + 1)
    g, grads = None, [None] * len(weights)
    for k in range(len(weights) - 1, -1, -1):
        x, s, xk = kept[k]
        ds, local, dwgc, dwbi, db = layer_bwd(x, s, xk, g, dout, c, weights[k][0], weights[k][2])
        grads[k] = (dwgc, db, dwbi, db)
        g = local + np.asarray(a @ ds)
    return g, grads


def bpr_l2(out, n_users, users, pos, neg, reg):
    """((bpr, l2), dOUT) of the batch on OUT's rows."""
    users, pos, neg = (np.asarray(t, np.int64) for t in (users, pos, neg))
    b = len(users)
    u, p, n = out[users], out[n_users + pos], out[n_users + neg]
    sg = 1.0 / (1.0 + np.exp(-((u * p).sum(1) - (u * n).sum(1))))
    bpr = float(np.mean(-np.log(1e-5 + sg)))
    norms = [np.sqrt((t * t).sum()) for t in (u, p, n)]
    l2 = float(reg * sum(norms) / b)
    dx = (-(sg * (1.0 - sg)) / (1e-5 + sg) / b)[:, None]
    dout = np.zeros_like(out)
    np.add.at(dout, users, dx * (p - n) + reg / b * u / norms[0])
    np.add.at(dout, n_users + pos, dx * u + reg / b * p / norms[1])
    np.add.at(dout, n_users + neg, -dx * u + reg / b * n / norms[2])
    return (bpr, l2), dout


def step(e0, a, weights, n_users, users, pos, neg, reg):
    """((bpr, l2), dE_0, per-layer (dWgc, dbgc, dWbi, dbbi)) of one batch."""
    out, kept = encoder_fwd(e0, a, weights)
    losses, dout = bpr_l2(out, n_users, users, pos, neg, reg)
    de0, grads = encoder_bwd(dout, a, weights, kept)
    return losses, de0, grads
