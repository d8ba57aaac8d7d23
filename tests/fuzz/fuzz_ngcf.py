#!/usr/bin/env python3
"""Randomised parity fuzzing of the fused NGCF layer (csrc/ngcf.hip: ops.ngcf_layer_fwd, ops.ngcf_layer_bwd) against the
float64 restatement (tests/ngcf_restate.py).

Per case: a width d from every multiple of 4 in [4, 256]; N in [1, 2200] with extra weight on 32 k - 1, 32 k, 32 k + 1 (the
tile edges) and on 1024 k, 1024 k + 1 (a full last chunk of 32 partials, and one more partial), and in one case in twenty
N in [65 537, 70 000] at d <= 32 (two tiles per wave); a scale from {0.05, 0.5, 1.5} for each of x, s and the
incoming gradients; a form for each direction:
  forward   bias or none; acc_in or none; y wanted or not; acc_out given or not (always, where y is not wanted); s_in, s_out
            from {1, 0.75, 0.5, 1/3}
  backward  g given or the top layer (g = c dout formed in the kernel)
Then
  * every output against float64, by the rule of tests/test_ngcf_gpu.py: largest error over the float64 value's largest
    magnitude, within 8x the same distance of the float32 torch formula on the same device at the same case (x_k, the
    backward's input, is the float64 forward rounded to float32 in all three arms: the same signs, the same slopes);
  * a second, identical call: every output bit-equal;
  * the permitted aliasing -- acc_out over acc_in; ds over s and / or local over g, each by a coin -- bit-equal to the
    unaliased call.
On a mismatch the seed and the drawn parameters are printed and the exit status is 1.  Count-based: a run reproduces.

    python tests/fuzz/fuzz_ngcf.py --cases 200 [--seed 0]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from coldrec_amd import ops  # noqa: E402
from tests import ngcf_restate as R  # noqa: E402
from tests.test_ngcf_gpu import _bwd_torch32, _dist, _fwd_torch32  # noqa: E402

DEV = torch.device("cuda:0")
SCALES = [0.05, 0.5, 1.5]
FACTORS = [1.0, 0.75, 0.5, 1.0 / 3.0]
SEED = None


def fail(what, **kw):
    print("MISMATCH", what, "seed", SEED, kw, flush=True)
    sys.exit(1)


def draw_shape(rng):
    """(N, d, tiles per wave)."""
    u = rng.random()
    if u < 0.05:
        n, d = int(rng.integers(65537, 70001)), 4 * int(rng.integers(1, 9))
    else:
        d = 4 * int(rng.integers(1, 65))
        if u < 0.35:
            n = 32 * int(rng.integers(1, 69)) + int(rng.integers(-1, 2))
        elif u < 0.50:
            n = 1024 * int(rng.integers(1, 3)) + int(rng.integers(0, 2))
        else:
            n = int(rng.integers(1, 2201))
    tiles = -(-n // 32)
    return n, d, max(1, -(-tiles // 2048))


def judge(what, params, names, fused, t32, want):
    for name, f, t, w in zip(names, fused, t32, want):
        if not torch.isfinite(f).all():
            fail(f"{what}: {name} not finite", **params)
        mine, ref = _dist(f, w), _dist(t, w)
        if not mine <= 8 * ref:
            fail(f"{what}: {name} against the float64 restatement", kernel=mine, float32_torch=ref, **params)


def same_bits(what, params, a, b):
    torch.cuda.synchronize()
    for p, q in zip(a, b):
        if (p is None) != (q is None) or (p is not None and not torch.equal(p, q)):
            fail(what, **params)


def draw(rng):
    """The case's parameters and host tensors (x, s, w, b, acc, g, dout): no device work."""
    n, d, tpw = draw_shape(rng)
    sx, ss, sg = (float(rng.choice(SCALES)) for _ in range(3))
    bias, acc_in, want_y = bool(rng.random() < 0.7), bool(rng.random() < 0.6), bool(rng.random() < 0.7)
    want_out = bool(rng.random() < 0.7) or not want_y
    s_in, s_out = float(rng.choice(FACTORS)), float(rng.choice(FACTORS))
    top = bool(rng.random() < 0.4)
    ds_over_s, local_over_g = bool(rng.random() < 0.5), bool(rng.random() < 0.5) and not top
    c = float(rng.choice(FACTORS[1:]))
    params = dict(N=n, d=d, tpw=tpw, scales=(sx, ss, sg), bias=bias, acc_in=acc_in, y=want_y, acc_out=want_out,
                  factors=(s_in, s_out, c), top=top, ds_over_s=ds_over_s, local_over_g=local_over_g)
    r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    return params, (r(n, d) * sx, r(n, d) * ss, r(2 * d, d) * (0.7 / d ** 0.5), r(2, d) * 0.1, r(n, d), r(n, d) * sg, r(n, d) * sg)


def case(rng):
    params, (x, s, w, b, acc, g, dout) = draw(rng)
    n, d, tpw, bias, acc_in, want_y, want_out, top = (params[k] for k in ("N", "d", "tpw", "bias", "acc_in", "y", "acc_out", "top"))
    (s_in, s_out, c), ds_over_s, local_over_g = params["factors"], params["ds_over_s"], params["local_over_g"]
    x64, s64, w64, b64 = R.f64(x), R.f64(s), R.f64(w), R.f64(b) * (1.0 if bias else 0.0)
    xd, sd, wd, accd, gd, doutd = (t.to(DEV) for t in (x, s, w, acc, g, dout))
    bd = b.to(DEV) if bias else None

    # ---- forward
    xk64 = R.layer_fwd(x64, s64, w64[:d], b64[0], w64[d:], b64[1])
    out64 = ((R.f64(acc) * s_in if acc_in else 0.0) + xk64) * s_out

    def fwd(a_in, alias=False):
        out = a_in if alias else (torch.empty_like(xd) if want_out else None)
        return ops.ngcf_layer_fwd(xd, sd, wd, bd, acc_in=a_in, s_in=s_in, acc_out=out, s_out=s_out, want_y=want_y)

    a_in = accd if acc_in else None
    y, out = fwd(a_in)
    if (y is None) == want_y or (out is None) == want_out:
        fail("forward: the outputs returned are not the outputs asked for", **params)
    t_xk, t_out = _fwd_torch32(xd, sd, wd, bd if bias else torch.zeros(2, d, device=DEV), a_in, s_in, s_out)
    got = [(nm, f, t, w_) for nm, f, t, w_ in (("x_k", y, t_xk, xk64), ("acc_out", out, t_out, out64)) if f is not None]
    judge("forward", params, *zip(*got))
    same_bits("forward: two identical calls differ in their bits", params, (y, out), fwd(a_in))
    if acc_in and want_out:
        same_bits("forward: acc_out over acc_in differs from the unaliased call", params, (y, out), fwd(accd.clone(), alias=True))

    # ---- backward, on the float64 forward's x_k rounded to float32: the same signs in every arm
    xk32 = torch.from_numpy(xk64).float()
    xkd = xk32.to(DEV)
    g_dev, g64 = (None, None) if top else (gd, R.f64(g))
    want = R.layer_bwd(x64, s64, R.f64(xk32), g64, R.f64(dout), c, w64[:d], w64[d:])
    want = (want[0], want[1], np.concatenate([want[2], want[3]]), want[4])
    plain = ops.ngcf_layer_bwd(xd, sd, xkd, g_dev, doutd, c, wd)
    judge("backward", params, ("ds", "local", "dw", "db"), plain, _bwd_torch32(xd, sd, xkd, g_dev, doutd, c, wd), want)
    same_bits("backward: two identical calls differ in their bits", params, plain, ops.ngcf_layer_bwd(xd, sd, xkd, g_dev, doutd, c, wd))
    if ds_over_s or local_over_g:
        s2, g2 = sd.clone(), (gd.clone() if not top else None)
        ali = ops.ngcf_layer_bwd(xd, s2, xkd, g2, doutd, c, wd, ds=s2 if ds_over_s else None, local=g2 if local_over_g else None)
        if (ds_over_s and ali[0] is not s2) or (local_over_g and ali[1] is not g2):
            fail("backward: the aliased buffers were not the ones written", **params)
        same_bits("backward: ds over s / local over g differs from the unaliased call", params, plain, ali)
    return tpw


def main():
    global SEED
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    SEED = args.seed
    rng = np.random.default_rng(args.seed)
    deep = 0
    for _ in range(args.cases):
        deep += case(rng) > 1
    print(f"fuzz ok: {args.cases} random ngcf cases within parity ({deep} with more than one tile per wave), seed {args.seed}")


if __name__ == "__main__":
    main()
