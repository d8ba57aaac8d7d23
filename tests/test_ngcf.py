"""CPU-only: the float64 restatement tests/ngcf_restate.py equals torch autograd on the formula of the G17 plug-in
(tests/test_g17_ngcf_plugin_gpu.py) in float64; the built-in NGCF trainer resolves by name without changing what the
registry lists; its flag errors fire before anything touches a device; its encoder draws the reference's random streams;
crh_ngcf_layer_*'s argument errors and workspace rule need no GPU.

Draw order.  The reference (model/NGCF.py:84-88) appends W_gc[k] and W_bi[k] layer by layer, so its stream is gc0, bi0, gc1,
bi1, ...; the plug-in's Encoder builds the two ModuleLists one after the other: gc0, gc1, ..., bi0, bi1, ....  The names
agree, the streams agree for one layer only.  The built-in follows the reference (a seeded run starts from the reference's
state); against the plug-in it is therefore checked bit for bit at L = 1, and at L = 2 against the plug-in's draws re-ordered
-- the same tensors, bit for bit, under the reference's assignment."""
import argparse
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from coldrec_amd import _lib
from tests import ngcf_restate as R
from tests.test_host_logic import builder

CORE = ["DropoutNet", "LightGCN", "MF"]


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="NGCF", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=1e-3, reg=1e-4,
             early_stop=10, eval_every=1, cold_object="item", save_emb=False, seed=2024, optimizer="adam", lazy_adam="auto")
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def random_problem(n=37, d=12, layers=2, n_users=15, batch=23, seed=0):
    """(E0, dense symmetric A, weights, users, pos, neg) in float64 torch tensors / int64 arrays."""
    g = torch.Generator().manual_seed(1700 + seed)
    upper = torch.triu((torch.rand(n, n, generator=g) < 0.15).double() * torch.rand(n, n, generator=g, dtype=torch.float64), 1)
    a = upper + upper.T                                               # sparse, symmetric, zero diagonal
    e0 = torch.randn(n, d, generator=g, dtype=torch.float64) * 0.5
    weights = [tuple(torch.randn(s, generator=g, dtype=torch.float64) * 0.4 for s in ((d, d), (d,), (d, d), (d,)))
               for _ in range(layers)]
    users = torch.randint(n_users, (batch,), generator=g).numpy()
    pos = torch.randint(n - n_users, (batch,), generator=g).numpy()
    neg = torch.randint(n - n_users, (batch,), generator=g).numpy()
    return e0, a, weights, n_users, users, pos, neg


def torch_step(e0, a, weights, n_users, users, pos, neg, reg):
    """The plug-in's forward and the reference's bpr_loss + l2_reg_loss under autograd, in the dtype of the inputs."""
    e0 = e0.clone().requires_grad_(True)
    ws = [tuple(t.clone().requires_grad_(True) for t in w) for w in weights]
    ego, outs = e0, [e0]
    for wgc, bgc, wbi, bbi in ws:
        side = a @ ego
        ego = F.leaky_relu(F.linear(side, wgc, bgc) + F.linear(ego * side, wbi, bbi))
        outs.append(ego)
    out = torch.mean(torch.stack(outs, dim=1), dim=1)
    u, p, n = out[:n_users][users], out[n_users:][pos], out[n_users:][neg]
    bpr = torch.mean(-torch.log(10e-6 + torch.sigmoid((u * p).sum(1) - (u * n).sum(1))))
    l2 = (torch.norm(u, p=2) / u.shape[0] + torch.norm(p, p=2) / p.shape[0] + torch.norm(n, p=2) / n.shape[0]) * reg
    (bpr + l2).backward()
    return (bpr.item(), l2.item()), out.detach(), e0.grad, [tuple(t.grad for t in w) for w in ws]


def test_restatement_equals_autograd_in_float64():
    prob = random_problem()
    e0, a, weights, n_users, users, pos, neg = prob
    reg = 1e-2
    (bpr, l2), out, de0, dws = torch_step(*prob, reg)
    np_w = [tuple(R.f64(t) for t in w) for w in weights]
    out_r, _ = R.encoder_fwd(R.f64(e0), R.f64(a), np_w)
    (bpr_r, l2_r), de0_r, dws_r = R.step(R.f64(e0), R.f64(a), np_w, n_users, users, pos, neg, reg)
    np.testing.assert_allclose(out_r, out.numpy(), rtol=1e-10)
    np.testing.assert_allclose([bpr_r, l2_r], [bpr, l2], rtol=1e-10)
    np.testing.assert_allclose(de0_r, de0.numpy(), rtol=1e-10)
    assert np.abs(de0.numpy()).max() > 0 and (out.numpy() < 0).any() and (out.numpy() > 0).any()
    for k in range(len(weights)):
        for got, want in zip(dws_r[k], dws[k]):
            np.testing.assert_allclose(got, want.numpy(), rtol=1e-10)


def test_restated_layer_at_exact_zeros():
    """z == 0 gives x_k = 0 and takes the slope 0.01, torch's rule."""
    x = np.arange(12.0).reshape(3, 4)
    s = np.zeros((3, 4))
    w = np.ones((4, 4))
    b = np.zeros(4)
    xk = R.layer_fwd(x, s, w, b, w, b)
    assert (xk == 0).all()
    g = np.ones((3, 4))
    z = torch.zeros(3, 4, dtype=torch.float64, requires_grad=True)
    F.leaky_relu(z).backward(torch.from_numpy(g))
    assert (z.grad.numpy() == 0.01).all()
    ds, local, dwgc, dwbi, db = R.layer_bwd(x, s, xk, g, np.zeros((3, 4)), 1 / 3, w, w)
    np.testing.assert_allclose(db, 0.03 * np.ones(4), rtol=1e-15)
    np.testing.assert_allclose(ds, 0.04 + x * 0.04, rtol=1e-15)


def test_ngcf_resolves_by_name_and_the_listings_stay():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    keys, names = sorted(AVAILABLE_MODELS.keys()), sorted(AVAILABLE_MODELS.names())
    assert "NGCF" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["NGCF"]
    assert isinstance(cls, type) and issubclass(cls, BaseColdStartTrainer) and cls.__name__ == "NGCF" and cls.fused_eval
    assert AVAILABLE_MODELS.get("NGCF") is cls
    assert sorted(AVAILABLE_MODELS.keys()) == keys and sorted(AVAILABLE_MODELS.names()) == names
    assert "NGCF" not in keys and "NGCF" not in names and "NGCF" in resolvable()
    assert [n for n in keys if n in CORE] == CORE


def test_cli_parser_takes_ngcf_without_new_flags():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "NGCF", "--layers", "3"])
    b = parse_args(["--model", "LightGCN", "--layers", "3"])
    assert a.layers == 3 and set(vars(a)) == set(vars(b))
    with pytest.raises(ValueError, match="NGCF"):                # the error message lists every name that resolves
        parse_args(["--model", "NoSuchModel"])


def test_flag_errors_and_cpu_refusal():
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.train import NGCFEngine
    _, data = builder()
    with pytest.raises(ValueError, match="--optimizer sgd is not built"):
        AVAILABLE_MODELS["NGCF"](_cfg(data, optimizer="sgd"))
    with pytest.raises(ValueError, match="--lazy_adam on is not built"):
        AVAILABLE_MODELS["NGCF"](_cfg(data, lazy_adam="on"))
    with pytest.raises(ValueError, match=r"--emb_size 6 must be a multiple of 4 in \[4, 256\]"):
        AVAILABLE_MODELS["NGCF"](_cfg(data, emb_size=6))
    with pytest.raises(ValueError, match="multiple of 4"):
        AVAILABLE_MODELS["NGCF"](_cfg(data, emb_size=260))
    with pytest.raises(RuntimeError, match="MI355X only"):
        AVAILABLE_MODELS["NGCF"](_cfg(data)).train()
    # the engine itself refuses the same before it touches the device
    u, v = torch.zeros(5, 6), torch.zeros(7, 6)
    with pytest.raises(ValueError, match="emb_size 6 must be a multiple of 4"):
        NGCFEngine(u, v, None, None, None, 1, 1e-3, 1e-4, "cuda:0", [None])
    with pytest.raises(ValueError, match="sgd is not built"):
        NGCFEngine(u, v, None, None, None, 1, 1e-3, 1e-4, "cuda:0", [None], optimizer="sgd")


def _plugin_encoder_class():
    from tests.test_g17_ngcf_plugin_gpu import _make_plugin
    cells = [c.cell_contents for c in _make_plugin().__init__.__closure__]
    (enc,) = [c for c in cells if isinstance(c, type) and c.__name__ == "Encoder"]
    return enc


@pytest.mark.parametrize("layers", [1, 2])
def test_encoder_draws_the_references_streams(layers):
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    set_seed(2024, False)
    tr = AVAILABLE_MODELS["NGCF"](_cfg(data, layers=layers))
    mine = tr.model.state_dict()
    set_seed(2024, False)
    theirs = {k: v for k, v in _plugin_encoder_class()(data, 64, layers, torch.device("cpu")).state_dict().items()
              if "norm_adj" not in k}
    assert sorted(mine) == sorted(theirs)
    if layers == 1:
        for k in theirs:
            assert torch.equal(mine[k], theirs[k]), k
        return
    # L = 2: the plug-in's stream is gc0, gc1, bi0, bi1; the reference's -- and the built-in's -- gc0, bi0, gc1, bi1
    same = {"embedding_dict.user_emb": "embedding_dict.user_emb", "embedding_dict.item_emb": "embedding_dict.item_emb",
            "W_gc.0": "W_gc.0", "W_bi.0": "W_gc.1", "W_gc.1": "W_bi.0", "W_bi.1": "W_bi.1"}
    for k in mine:
        stem, _, leaf = k.rpartition(".")
        other = same[k] if k in same else same[stem] + "." + leaf
        assert torch.equal(mine[k], theirs[other]), (k, other)
    # and written out: the reference's own order of construction
    set_seed(2024, False)
    init = torch.nn.init.xavier_uniform_
    u, i = init(torch.empty(data.user_num, 64)), init(torch.empty(data.item_num, 64))
    lin = [torch.nn.Linear(64, 64) for _ in range(4)]                 # gc0, bi0, gc1, bi1
    assert torch.equal(mine["embedding_dict.user_emb"], u) and torch.equal(mine["embedding_dict.item_emb"], i)
    for name, m in zip(("W_gc.0", "W_bi.0", "W_gc.1", "W_bi.1"), lin):
        assert torch.equal(mine[name + ".weight"], m.weight) and torch.equal(mine[name + ".bias"], m.bias)


def test_g17_initial_state_loads_by_name():
    import json
    from coldrec_amd.model import AVAILABLE_MODELS
    from tests.conftest import load_golden
    g = load_golden("g17_ngcf.npz")
    _, data = builder()
    tr = AVAILABLE_MODELS["NGCF"](_cfg(data, layers=int(g["layers"]), emb_size=int(g["d"])))
    sd = {k[len("init__"):]: torch.from_numpy(g[k].copy()) for k in g.files if k.startswith("init__")}
    res = tr.model.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert sorted(tr.model.state_dict()) == json.loads(str(g["param_names"]))
    assert len(tr.model.weights()) == int(g["layers"])


def test_workspace_rule_and_argument_errors_without_gpu():
    L = _lib.lib()
    # at most 2048 partials of (2 dp + 1) dp floats, and their chunk sums: far below one table at catalogue scale
    pe = (2 * 64 + 1) * 64 * 4
    assert 0 < L.crh_ngcf_workspace_bytes(1_000_000, 64) <= (2048 + 64) * (pe + 256)
    assert L.crh_ngcf_workspace_bytes(1, 4) >= 2 * (2 * 32 + 1) * 32 * 4
    assert L.crh_ngcf_workspace_bytes(0, 64) == 0 and L.crh_ngcf_workspace_bytes(10, 6) == 0
    assert L.crh_ngcf_workspace_bytes(10, 260) == 0
    p, q, r = 256, 512, 768                                           # non-NULL, aligned addresses: nothing is launched

    def fwd(x=p, s=q, w=r, b=None, n=10, d=8, y=1024, acc_in=None, acc_out=None):
        return L.crh_ngcf_layer_fwd_f32(x, s, w, b, n, d, y, acc_in, 1.0, acc_out, 1.0, None)

    for kw, word in ((dict(x=None), "NULL x, s or w"), (dict(y=None), "nothing to compute"), (dict(d=6), "multiple of 4"),
                     (dict(d=260), "multiple of 4"), (dict(n=0), "n_rows"), (dict(w=772), "16-byte aligned"),
                     (dict(y=p), "aliases"), (dict(acc_out=q), "aliases"), (dict(y=1024, acc_out=1024), "aliases")):
        assert fwd(**kw) == -1, kw
        assert word in L.crh_last_error().decode(), (kw, L.crh_last_error())

    need = L.crh_ngcf_workspace_bytes(10, 8)

    def bwd(x=p, s=q, xk=r, g=None, dout=1024, w=1280, n=10, d=8, ds=1536, local=1792, dw=2048, db=2304, ws=4096,
            ws_bytes=need):
        return L.crh_ngcf_layer_bwd_f32(x, s, xk, g, dout, 0.5, w, n, d, ds, local, dw, db, ws, ws_bytes, None)

    for kw, word in ((dict(xk=None), "NULL x, s, xk"), (dict(db=None), "NULL ds, local"), (dict(d=6), "multiple of 4"),
                     (dict(n=0), "n_rows"), (dict(dout=1028), "16-byte aligned"), (dict(ds=p), "alias"),
                     (dict(local=q), "alias"), (dict(ds=1792), "alias"), (dict(local=1024), "alias")):
        assert bwd(**kw) == -1, kw
        assert word in L.crh_last_error().decode(), (kw, L.crh_last_error())
    # one byte too small, NULL and misaligned workspaces are refused with the workspace code, not overrun
    for kw in (dict(ws_bytes=need - 1), dict(ws=None), dict(ws=4096 + 64)):
        assert bwd(**kw) == -3, kw                                    # CRH_ERR_WS
        assert "workspace" in L.crh_last_error().decode()


def test_ops_refuse_cpu_tensors_and_wrong_shapes():
    from coldrec_amd import ops
    x, w = torch.zeros(5, 8), torch.zeros(16, 8)
    with pytest.raises(RuntimeError):
        ops.ngcf_layer_fwd(x, x.clone(), w)
    with pytest.raises(RuntimeError):
        ops.ngcf_layer_bwd(x, x.clone(), x.clone(), None, x.clone(), 0.5, w)
