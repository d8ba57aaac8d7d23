"""GPU: the fused NGCF layer (csrc/ngcf.hip) against the float64 restatement (tests/ngcf_restate.py, itself pinned to
torch autograd by tests/test_ngcf.py) at the shapes that cross every tile edge, its exact zeros, its determinism, bounds,
workspace and aliasing contracts; one ``NGCFEngine.step`` against the restatement; the built-in trainer against G17 -- the
reference's own ``NGCF.run()`` -- under the assertions and tolerances of the plug-in test; and the CLI chain NGCF -> GAR.

Bars.  Every output is measured as its largest error over the largest magnitude of the float64 value; the bar is 8x the
same distance of the float32 torch formula, run on the same device at the same shape (measured in the test, printed with
the kernel's).  The backward takes x_k as an input, so all three (kernel, float32 formula, float64) take the slope from the
same signs.  Measured on the MI355X: the kernel's worst ratio to the torch formula's own distance is 2.74 over the layer
cases (N17-d12 bwd, ds: 1.4e-7 against 5.0e-8) and 0.94 in the engine step; its largest distance 8.8e-7 (x_k, N1003-d256,
torch 5.9e-7).  The G17 run ends 1.0e-7 (bpr), 3.5e-7 (l2), 1.5e-8 (epoch norms), 1.7e-8 (parameter norms) and 2.4e-7
(sampled rows) from the reference's, every test metric equal (the NGCF section)."""
import argparse
import json
import types
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import ngcf_restate as R
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# (N, d): every N in {1, 15, 16, 17, 63, 65, 257, 1003} and every d in {4, 12, 16, 60, 64, 100, 128, 256} at least once;
# d <= 64 takes the one-kernel backward (weights in LDS), wider ones the two-launch form.  These widths reach the
# instantiations DP = 32, 64, 128, 256 (1, 1, 4, 16 slabs), at most 32 partials (one chunk) and one tile per wave.
# tests/test_ngcf_edges_gpu.py adds DP = 96, 160, 192, 224 (3, 10, 12, 14 slabs; 160 and 224 with an odd tile count), 2 .. 64
# chunks of partials and 2 and 3 tiles per wave.
PAIRS = [(1, 4), (15, 12), (16, 16), (17, 12), (63, 60), (65, 64), (257, 100), (1003, 64), (257, 128), (1003, 256), (17, 256),
         (65, 4), (1003, 100), (63, 128)]
IDS = lambda p: "N%d-d%d" % p
C = 1.0 / 3.0


def _inputs(n, d, seed=0):
    g = torch.Generator().manual_seed(1900 + 31 * n + d + seed)
    r = lambda *s: torch.randn(*s, generator=g)
    inp = dict(x=r(n, d) * 0.5, s=r(n, d) * 0.5, w=r(2 * d, d) * (0.7 / d ** 0.5), b=r(2, d) * 0.1, acc=r(n, d),
               g=r(n, d) * 0.1, dout=r(n, d) * 0.1)
    return inp


def _dist(got, want):
    top = np.abs(want).max()
    err = np.abs(np.asarray(got.detach().cpu().numpy() if torch.is_tensor(got) else got, np.float64) - want).max()
    return float(err / top) if top > 0 else float(err)


def _check(tag, names, fused, torch32, want):
    worst = 0.0
    parts = []
    for name, f, t, w in zip(names, fused, torch32, want):
        assert torch.isfinite(f).all(), name
        mine, ref = _dist(f, w), _dist(t, w)
        ratio = mine / ref if ref > 0 else (0.0 if mine == 0 else float("inf"))
        worst = max(worst, ratio)
        parts.append(f"{name} {mine:.1e} (torch {ref:.1e})")
    print(f"{tag}: " + ", ".join(parts) + f"; worst kernel / torch ratio {worst:.2f}")
    for name, f, t, w in zip(names, fused, torch32, want):
        assert _dist(f, w) <= 8 * _dist(t, w), (tag, name, _dist(f, w), _dist(t, w))
    return worst


def _fwd_torch32(x, s, w, b, acc, s_in, s_out):
    d = x.shape[1]
    xk = F.leaky_relu(F.linear(s, w[:d], b[0]) + F.linear(x * s, w[d:], b[1]))
    return xk, ((acc * s_in if acc is not None else 0) + xk) * s_out


def _bwd_torch32(x, s, xk, g, dout, c, w):
    d = x.shape[1]
    dz = (c * dout if g is None else g) * torch.where(xk > 0, 1.0, 0.01)
    t = dz @ w[d:]
    return dz @ w[:d] + x * t, c * dout + s * t, torch.cat([dz.T @ s, dz.T @ (x * s)]), dz.sum(0)


@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_layer_forward_matches_float64_restatement(pair):
    from coldrec_amd import ops
    n, d = pair
    inp = _inputs(n, d)
    x, s, w, b, acc = (inp[k].to(DEV) for k in ("x", "s", "w", "b", "acc"))
    x64, s64, w64, b64, acc64 = (R.f64(inp[k]) for k in ("x", "s", "w", "b", "acc"))
    xk64 = R.layer_fwd(x64, s64, w64[:d], b64[0], w64[d:], b64[1])
    # form A: y and acc_in given, both scales off 1, acc_out a buffer of its own
    y, out = torch.empty_like(x), torch.empty_like(x)
    ops.ngcf_layer_fwd(x, s, w, b, y=y, acc_in=acc, s_in=0.75, acc_out=out, s_out=0.5)
    t_xk, t_out = _fwd_torch32(x, s, w, b, acc, 0.75, 0.5)
    _check(IDS(pair) + " fwd", ("x_k", "acc_out"), (y, out), (t_xk, t_out), (xk64, (acc64 * 0.75 + xk64) * 0.5))
    # form B: no y, no acc_in
    y2, out2 = ops.ngcf_layer_fwd(x, s, w, b, acc_out=torch.empty_like(x), s_out=C, want_y=False)
    assert y2 is None
    _check(IDS(pair) + " fwd, no y, no acc_in", ("acc_out",), (out2,), (_fwd_torch32(x, s, w, b, None, 1.0, C)[1],),
           (xk64 * C,))
    # form C: y alone, no bias; acc_out over acc_in
    y3, none = ops.ngcf_layer_fwd(x, s, w)
    assert none is None
    nb = R.layer_fwd(x64, s64, w64[:d], 0.0, w64[d:], 0.0)
    _check(IDS(pair) + " fwd, y alone, no bias", ("x_k",), (y3,), (_fwd_torch32(x, s, w, b * 0, None, 1.0, 1.0)[0],), (nb,))
    acc_io = acc.clone()
    ops.ngcf_layer_fwd(x, s, w, b, acc_in=acc_io, s_in=0.75, acc_out=acc_io, s_out=0.5, want_y=False)
    assert torch.equal(acc_io, out)


@pytest.mark.parametrize("top", [False, True], ids=["g", "top-layer"])
@pytest.mark.parametrize("pair", PAIRS, ids=IDS)
def test_layer_backward_matches_float64_restatement(pair, top):
    from coldrec_amd import ops
    n, d = pair
    inp = _inputs(n, d, seed=1)
    x64, s64, w64, b64 = (R.f64(inp[k]) for k in ("x", "s", "w", "b"))
    xk32 = torch.from_numpy(R.layer_fwd(x64, s64, w64[:d], b64[0], w64[d:], b64[1])).float()    # the signs all three use
    assert (xk32 > 0).any() or n * d < 8
    x, s, w, g, dout = (inp[k].to(DEV) for k in ("x", "s", "w", "g", "dout"))
    xk = xk32.to(DEV)
    g_dev, g64 = (None, None) if top else (g, R.f64(inp["g"]))
    ds, local, dw, db = ops.ngcf_layer_bwd(x, s, xk, g_dev, dout, C, w)
    want = R.layer_bwd(x64, s64, R.f64(xk32), g64, R.f64(inp["dout"]), C, w64[:d], w64[d:])
    want = (want[0], want[1], np.concatenate([want[2], want[3]]), want[4])
    _check(IDS(pair) + (" bwd top" if top else " bwd"), ("ds", "local", "dw", "db"), (ds, local, dw, db),
           _bwd_torch32(x, s, xk, g_dev, dout, C, w), want)


@pytest.mark.parametrize("pair", [(17, 12), (257, 128)], ids=IDS)
def test_exact_zeros_take_torchs_rule(pair):
    """s = 0 and zero biases: z == 0 exactly, x_k = 0, and the backward takes the slope 0.01."""
    from coldrec_amd import ops
    n, d = pair
    inp = _inputs(n, d, seed=2)
    x, w, g, dout, acc = (inp[k].to(DEV) for k in ("x", "w", "g", "dout", "acc"))
    s, b = torch.zeros_like(x), torch.zeros(2, d, device=DEV)
    y, out = ops.ngcf_layer_fwd(x, s, w, b, acc_in=acc, s_in=1.0, acc_out=torch.empty_like(x), s_out=1.0)
    assert (y == 0).all() and not torch.signbit(y).any() and torch.equal(out, acc)
    z = torch.zeros(n, d, device=DEV, requires_grad=True)
    F.leaky_relu(z).backward(g)
    assert torch.allclose(z.grad, g * 0.01, rtol=1e-6, atol=0)          # torch's rule, on this device
    ds, local, dw, db = ops.ngcf_layer_bwd(x, s, y, g, dout, C, w)
    assert (dw == 0).all()
    x64, w64, dz = R.f64(inp["x"]), R.f64(inp["w"]), 0.01 * R.f64(inp["g"])
    t = dz @ w64[d:]
    for name, got, want in (("db", db, dz.sum(0)), ("ds", ds, dz @ w64[:d] + x64 * t), ("local", local, C * R.f64(inp["dout"]))):
        assert _dist(got, want) <= 2e-6, (name, _dist(got, want))


@pytest.mark.parametrize("pair", [(1003, 64), (2049, 132)], ids=IDS)
def test_two_identical_backward_calls_give_identical_bits(pair):
    from coldrec_amd import ops
    n, d = pair
    inp = _inputs(n, d, seed=3)
    x, s, w, g, dout, xk = (inp[k].to(DEV) for k in ("x", "s", "w", "g", "dout", "acc"))
    a = ops.ngcf_layer_bwd(x, s, xk, g, dout, C, w)
    b = ops.ngcf_layer_bwd(x, s, xk, g, dout, C, w)
    for p, q in zip(a, b):
        assert torch.equal(p, q)
    fa, fb = ops.ngcf_layer_fwd(x, s, w)[0], ops.ngcf_layer_fwd(x, s, w)[0]
    assert torch.equal(fa, fb)


CANARY = -7.25


def _guarded(rows, cols, pad=8):
    """(whole buffer, the (rows, cols) view in its middle): ``pad`` canary rows on both sides."""
    shape = (rows + 2 * pad, cols) if cols else (rows + 2 * pad,)
    buf = torch.full(shape, CANARY, dtype=torch.float32, device=DEV)
    return buf, buf[pad:pad + rows]


def _intact(buf, rows, pad=8):
    return bool((buf[:pad] == CANARY).all() and (buf[pad + rows:] == CANARY).all())


@pytest.mark.parametrize("pair", [(17, 12), (1003, 256), (2049, 132)], ids=IDS)
def test_nothing_is_written_outside_the_outputs_and_the_workspace(pair):
    from coldrec_amd import ops
    n, d = pair
    inp = _inputs(n, d, seed=4)
    x, s, w, b, g, dout, acc = (inp[k].to(DEV) for k in ("x", "s", "w", "b", "g", "dout", "acc"))
    ybuf, y = _guarded(n, d)
    obuf, out = _guarded(n, d)
    ops.ngcf_layer_fwd(x, s, w, b, y=y, acc_in=acc, acc_out=out)
    torch.cuda.synchronize()
    assert _intact(ybuf, n) and _intact(obuf, n) and (y != CANARY).any() and (out != CANARY).any()
    need = ops.ngcf_workspace_bytes(n, d)
    wsbuf = torch.full((need + 512,), 0x5A, dtype=torch.uint8, device=DEV)
    assert wsbuf.data_ptr() % 256 == 0
    bufs = [_guarded(n, d), _guarded(n, d), _guarded(2 * d, d), _guarded(d, 0)]
    ds, local, dw, db = (v for _, v in bufs)
    ops.ngcf_layer_bwd(x, s, y, g, dout, C, w, ds=ds, local=local, dw=dw, db=db, workspace=wsbuf[256:256 + need])
    torch.cuda.synchronize()
    for (buf, v), rows in zip(bufs, (n, n, 2 * d, d)):
        assert _intact(buf, rows) and (v != CANARY).all()
    assert (wsbuf[:256] == 0x5A).all() and (wsbuf[256 + need:] == 0x5A).all()
    # and the same answer as with buffers the op makes itself
    for got, want in zip((ds, local, dw, db), ops.ngcf_layer_bwd(x, s, y, g, dout, C, w)):
        assert torch.equal(got, want)


def test_a_workspace_one_byte_short_is_refused():
    from coldrec_amd import ops
    n, d = 65, 64
    inp = _inputs(n, d, seed=5)
    x, s, w, g, dout, xk = (inp[k].to(DEV) for k in ("x", "s", "w", "g", "dout", "acc"))
    need = ops.ngcf_workspace_bytes(n, d)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    bufs = [_guarded(n, d), _guarded(n, d), _guarded(2 * d, d), _guarded(d, 0)]
    ds, local, dw, db = (v for _, v in bufs)
    with pytest.raises(RuntimeError, match=r"code -3.*workspace"):
        ops.ngcf_layer_bwd(x, s, xk, g, dout, C, w, ds=ds, local=local, dw=dw, db=db, workspace=ws[:need - 1])
    torch.cuda.synchronize()
    assert all((buf == CANARY).all() for buf, _ in bufs) and (ws == 0).all()       # nothing was launched
    ops.ngcf_layer_bwd(x, s, xk, g, dout, C, w, ds=ds, local=local, dw=dw, db=db, workspace=ws)


@pytest.mark.parametrize("pair", [(1003, 64), (257, 128), (17, 256), (63, 60), (2049, 132)], ids=IDS)
def test_permitted_aliasing_gives_the_same_bits(pair):
    """local over g and ds over s (include/coldrec_hip.h), in the one-kernel form (d <= 64) and the two-launch form."""
    from coldrec_amd import ops
    n, d = pair
    inp = _inputs(n, d, seed=6)
    x, s, w, g, dout, xk = (inp[k].to(DEV) for k in ("x", "s", "w", "g", "dout", "acc"))
    plain = ops.ngcf_layer_bwd(x, s, xk, g, dout, C, w)
    g2, s2 = g.clone(), s.clone()
    ds, local, dw, db = ops.ngcf_layer_bwd(x, s2, xk, g2, dout, C, w, ds=s2, local=g2)
    assert ds is s2 and local is g2
    for got, want in zip((ds, local, dw, db), plain):
        assert torch.equal(got, want)
    # the forward's acc_out over acc_in is covered by the forward test; the top layer (g = None) with ds over s
    plain = ops.ngcf_layer_bwd(x, s, xk, None, dout, C, w)
    s3 = s.clone()
    for got, want in zip(ops.ngcf_layer_bwd(x, s3, xk, None, dout, C, w, ds=s3), plain):
        assert torch.equal(got, want)


# ---- the engine -------------------------------------------------------------------------------------------------------

def _toy():
    from tests.test_g17_ngcf_plugin_gpu import _toy_builder
    return _toy_builder()


def _engine(data, init, layers=2):
    from coldrec_amd.train import NGCFEngine
    rowptr, col, val = data.norm_adj_csr()
    eng = NGCFEngine(init["u"], init["v"], rowptr, col, val, layers, 1e-3, 1e-4, DEV, init["w"])
    eng.keep_grad = True
    return eng


def test_one_engine_step_matches_the_restatement_and_repeats_bit_for_bit():
    from coldrec_amd import ops
    data = _toy()
    U, I, d, L, B, reg = data.user_num, data.item_num, 64, 2, 512, 1e-4
    g = torch.Generator().manual_seed(77)
    init = dict(u=torch.randn(U, d, generator=g) * 0.1, v=torch.randn(I, d, generator=g) * 0.1,
                w=[tuple(torch.randn(sh, generator=g) * sc for sh, sc in (((d, d), 0.1), ((d,), 0.05), ((d, d), 0.1), ((d,), 0.05)))
                   for _ in range(L)])
    users = torch.randint(U, (B,), generator=g, dtype=torch.int32)
    pos = torch.randint(I, (B,), generator=g, dtype=torch.int32)
    neg = torch.randint(I, (B,), generator=g, dtype=torch.int32)
    u_d, p_d, n_d = users.to(DEV), pos.to(DEV), neg.to(DEV)
    plan = ops.build_plans_device(u_d, p_d, n_d, B)[0]
    runs = []
    for _ in range(2):
        eng = _engine(data, init, L)
        eng.step(u_d, p_d, n_d, plan)
        torch.cuda.synchronize()
        runs.append(eng)
    a, b = runs
    assert torch.equal(a.G, b.G) and torch.equal(a.E, b.E) and torch.equal(a.loss, b.loss)
    for k in range(L):
        assert torch.equal(a.dWst[k], b.dWst[k]) and torch.equal(a.dbst[k], b.dbst[k])
        assert torch.equal(a.Wst[k], b.Wst[k]) and torch.equal(a.bst[k], b.bst[k])
        assert not torch.equal(a.Wst[k], torch.cat([init["w"][k][0], init["w"][k][2]]).to(DEV))      # the layers moved
    assert not torch.equal(a.E[:U].cpu(), init["u"])
    # float64 restatement, and the float32 torch formula under autograd on this device
    e0 = torch.cat([init["u"], init["v"]])
    w64 = [tuple(R.f64(t) for t in w) for w in init["w"]]
    (bpr, l2), de0, grads = R.step(R.f64(e0), data.norm_adj.tocsr().astype(np.float64), w64, U, users.numpy(), pos.numpy(),
                                   neg.numpy(), reg)
    adj = torch.from_numpy(data.norm_adj.toarray().astype(np.float32)).to(DEV)
    from tests.test_ngcf import torch_step
    (t_bpr, t_l2), _, t_de0, t_grads = torch_step(e0.to(DEV), adj, [tuple(t.to(DEV) for t in w) for w in init["w"]], U,
                                                 users.long().to(DEV), pos.long().to(DEV), neg.long().to(DEV), reg)
    loss = a.loss.cpu().numpy()
    print(f"engine step: bpr {loss[0]:.7f} (float64 {bpr:.7f}), l2 {loss[1]:.3e} (float64 {l2:.3e})")
    np.testing.assert_allclose(loss, [bpr, l2], rtol=1e-5)
    names, fused, t32, want = ["dE0"], [a.G], [t_de0], [de0]
    for k in range(L):
        d_ = d
        for j, (nm, f) in enumerate((("dWgc", a.dWst[k][:d_]), ("dbgc", a.dbst[k]), ("dWbi", a.dWst[k][d_:]), ("dbbi", a.dbst[k]))):
            names.append(f"{nm}{k}")
            fused.append(f)
            t32.append(t_grads[k][j])
            want.append(grads[k][j])
    _check("engine step", names, fused, t32, want)
    # the parameters' .grad are the kernel's buffers
    for k in range(L):
        assert a.W_gc[k].grad.data_ptr() == a.dWst[k].data_ptr() and a.b_bi[k].grad.data_ptr() == a.dbst[k].data_ptr()


def test_engine_refuses_what_is_not_built():
    from coldrec_amd.train import DPContext
    data = _toy()
    g = torch.Generator().manual_seed(78)
    d = 16
    init = dict(u=torch.randn(data.user_num, d, generator=g), v=torch.randn(data.item_num, d, generator=g),
                w=[(torch.randn(d, d, generator=g), torch.zeros(d), torch.randn(d, d, generator=g), torch.zeros(d))])
    eng = _engine(data, init, 1)
    with pytest.raises(RuntimeError, match="data-parallel training is not built"):
        eng.enable_data_parallel(DPContext(2, 0))
    with pytest.raises(RuntimeError, match="row-sharded propagation is not built"):
        eng.enable_row_sharding(DPContext(2, 0))
    u, v = eng.forward()                                               # the evaluation forward: no x_L is stored
    assert u.shape == (data.user_num, d) and v.shape == (data.item_num, d) and torch.isfinite(u).all()


# ---- G17: the reference's own NGCF.run() --------------------------------------------------------------------------------

def test_builtin_ngcf_matches_the_references_run_g17(monkeypatch, capsys):
    from coldrec_amd import ops
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    g = load_golden("g17_ngcf.npz")
    data = _toy()
    L, epochs, B = int(g["layers"]), int(g["epochs"]), int(g["batch_size"])
    a = dict(dataset="toy", model="NGCF", epochs=epochs, layers=L, topN="10,20", bs=B, emb_size=int(g["d"]), lr=float(g["lr"]),
             reg=float(g["reg"]), runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF",
             early_stop=10, eval_every=1, optimizer="adam", lazy_adam="auto")
    calls = dict(spmm=0, adam=0, fused=0, save=0, fwd=0, bwd=0)
    seen = dict(crc=0, epoch_norm=[])
    real = dict(spmm=ops.spmm_csr, adam=ops.spmm_csr_adam, rank=ops.score_topk, plans=ops.build_plans_device,
                fwd=ops.ngcf_layer_fwd, bwd=ops.ngcf_layer_bwd)

    def counted(key, fn):
        def f(*x, **kw):
            calls[key] += 1
            return fn(*x, **kw)
        return f

    def plans_seen(u, i, j, batch, **kw):                              # once per epoch: the epoch's triples
        hu, hi_, hj = (t.cpu().numpy().astype(np.int32) for t in (u, i, j))
        for lo in range(0, len(hu), batch):
            c = 0
            for arr in (hu, hi_, hj):
                c = zlib.crc32(arr[lo:lo + batch].tobytes(), c)
            seen["crc"] = c ^ (seen["crc"] * 31 & 0xFFFFFFFF)
        return real["plans"](u, i, j, batch, **kw)

    monkeypatch.setattr(ops, "spmm_csr", counted("spmm", real["spmm"]))
    monkeypatch.setattr(ops, "spmm_csr_adam", counted("adam", real["adam"]))
    monkeypatch.setattr(ops, "score_topk", counted("fused", real["rank"]))
    monkeypatch.setattr(ops, "ngcf_layer_fwd", counted("fwd", real["fwd"]))
    monkeypatch.setattr(ops, "ngcf_layer_bwd", counted("bwd", real["bwd"]))
    monkeypatch.setattr(ops, "build_plans_device", plans_seen)
    set_seed(2024, True)
    tr = AVAILABLE_MODELS["NGCF"](types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=DEV))
    sd = {k[len("init__"):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("init__")}
    tr.model.load_state_dict(sd, strict=True)                          # the reference's initial state: loaded, not re-drawn
    real_eval, real_save = tr.fast_evaluation, tr.save

    def eval_seen(*x, **kw):
        seen["epoch_norm"].append([float(torch.linalg.norm(tr.user_emb.double())), float(torch.linalg.norm(tr.item_emb.double()))])
        return real_eval(*x, **kw)

    def save_seen(*x, **kw):
        calls["save"] += 1
        return real_save(*x, **kw)

    tr.fast_evaluation, tr.save = eval_seen, save_seen
    seen["crc"] = 0                                                    # (the constructor's warm-up launches are not the run's)
    for k in calls:
        calls[k] = 0
    tr.run()
    capsys.readouterr()
    n = len(g["bpr"])
    bpr, l2 = tr.batch_losses[:, 0], tr.batch_losses[:, 1]
    assert seen["crc"] == int(g["triples_crc"]), "the sampler's triples differ from the reference's NumPy stream"
    assert len(bpr) == n
    np.testing.assert_allclose(bpr, g["bpr"], rtol=1e-5, err_msg="bpr loss per batch")
    np.testing.assert_allclose(bpr + l2, g["bpr"] + g["l2"], rtol=1e-5)
    np.testing.assert_allclose(l2, g["l2"], rtol=1e-4)
    np.testing.assert_allclose(np.array(seen["epoch_norm"]), g["epoch_norm"], rtol=1e-5, err_msg="propagated tables per epoch")
    fin = {k: v.detach().cpu().numpy() for k, v in tr.model.state_dict().items()}
    names = json.loads(str(g["param_names"]))
    assert sorted(fin) == names
    norms = np.array([np.linalg.norm(fin[k].astype(np.float64)) for k in names])
    np.testing.assert_allclose(norms, g["final_param_norm"], rtol=1e-5)
    assert tr.epochs_ran == int(g["epochs_ran"]) and tr.bestPerformance[0] == int(g["best_epoch"])
    for k, v in json.loads(str(g["best_metrics"])).items():
        assert abs(tr.bestPerformance[1][k] - v) <= 2e-4, (k, tr.bestPerformance[1][k], v)
    U, V = tr.user_emb.detach().cpu().numpy(), tr.item_emb.detach().cpu().numpy()
    np.testing.assert_allclose([np.linalg.norm(U.astype(np.float64)), np.linalg.norm(V.astype(np.float64))], g["final_norm"], rtol=1e-5)
    rows_worst = 0.0
    for got, ref in ((U[g["rows_u"]], g["final_U"]), (V[g["rows_v"]], g["final_V"])):
        assert np.abs(got - ref).max() <= 2e-4 * np.abs(ref).max()
        rows_worst = max(rows_worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
    worst = 0.0
    for name, got in (("test_overall", tr.overall_test_results), ("test_cold", tr.cold_test_results), ("test_warm", tr.warm_test_results)):
        np.testing.assert_allclose(np.array(got), g[name], atol=2e-4, rtol=0, err_msg=name)
        worst = max(worst, float(np.abs(np.array(got) - g[name]).max()))
    # exactly L SpMM launches per propagation: per step L forward and L backward (the last with Adam in its epilogue), L per
    # epoch-end forward, L per save(); one fused layer per SpMM and direction
    props = n + tr.epochs_ran + calls["save"]
    assert calls["adam"] == n and calls["spmm"] == props * L + n * (L - 1), calls
    assert calls["fwd"] == props * L and calls["bwd"] == n * L, calls
    assert calls["fused"] >= epochs + 3, calls                         # every validation and the three tests ranked by the fused kernel
    err = np.abs(bpr - g["bpr"]) / np.abs(g["bpr"])
    print("g17 ngcf built-in: %d batches, worst relative bpr error %.1e, l2 %.1e, norms %.1e, parameter norms %.1e, sampled rows "
          "%.1e of the maximum, test metrics within %.1e; %d + %d SpMM launches, %d + %d fused layers, %d fused rankings"
          % (n, err.max(), float(np.abs(l2 / g["l2"] - 1).max()), float(np.abs(np.array(seen["epoch_norm"]) / g["epoch_norm"] - 1).max()),
             float(np.abs(norms / g["final_param_norm"] - 1).max()), rows_worst, worst, calls["spmm"], calls["adam"], calls["fwd"],
             calls["bwd"], calls["fused"]))


# ---- the CLI chain ------------------------------------------------------------------------------------------------------

def test_cli_trains_ngcf_and_a_cold_start_trainer_loads_its_tables(tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "MF", "--make_synthetic", "toy"] + common) is None
    with pytest.raises(FileNotFoundError):                             # an untrained backbone still has no tables
        main(["--model", "DropoutNet", "--backbone", "NGCF", "--epochs", "1"] + common)
    pay = main(["--model", "NGCF", "--epochs", "1"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "NGCF" / "history.txt").is_file()
    saved = {s: torch.load(tmp_path / "emb" / f"toy_cold_item_NGCF_{s}_emb.pt", map_location="cpu") for s in ("user", "item")}
    for t in saved.values():
        assert torch.is_tensor(t) and not isinstance(t, torch.nn.Parameter) and t.shape[1] == 64 and torch.isfinite(t).all()
    pay = main(["--model", "GAR", "--backbone", "NGCF", "--epochs", "1"] + common)
    assert set(pay) == {"10", "20"}
    out = torch.load(tmp_path / "emb" / "toy_cold_item_GAR_item_emb.pt", map_location="cpu")
    assert out.shape == saved["item"].shape and torch.isfinite(out).all() and not torch.equal(out, saved["item"])
