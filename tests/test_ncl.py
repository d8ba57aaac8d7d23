"""CPU-only: the built-in NCL trainer resolves by name without changing what the registry lists, its flags parse, its
argument rules hold; crh_table_nce_f32's workspace stays linear in the table and its argument errors need no GPU; the float64
restatement tests/ncl_restate.py reproduces G23 -- the reference's own ssl_layer_loss and its own NCL.run() on the toy split
(tests/golden/make_golden_g23.py); and the prototype phase's k-means (train.lloyd_kmeans, the project's own) agrees with its
numpy restatement."""
import argparse
import types

import numpy as np
import pytest
import torch

from coldrec_amd import _lib
from tests import ncl_restate
from tests.conftest import load_golden
from tests.test_host_logic import builder

CORE = ["DropoutNet", "LightGCN", "MF"]


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="NCL", epochs=2, layers=3, topN="10,20", bs=512, emb_size=64, lr=1e-3, reg=1e-4,
             early_stop=10, eval_every=1, cold_object="item", save_emb=False, seed=2024, tau=0.2, ssl_reg=1e-6,
             proto_reg=1e-7, alpha=1.0, hyper_layers=1, num_clusters=20, proto_start=20)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def test_ncl_resolves_by_name_and_the_listings_stay():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    keys, names = sorted(AVAILABLE_MODELS.keys()), sorted(AVAILABLE_MODELS.names())
    assert "NCL" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["NCL"]
    assert isinstance(cls, type) and issubclass(cls, BaseColdStartTrainer) and cls.__name__ == "NCL" and cls.fused_eval
    assert AVAILABLE_MODELS.get("NCL") is cls
    assert sorted(AVAILABLE_MODELS.keys()) == keys and sorted(AVAILABLE_MODELS.names()) == names
    assert "NCL" not in keys and "NCL" not in names and "NCL" in resolvable()
    assert [n for n in keys if n in CORE] == CORE


def test_cli_parser_knows_the_ncl_flags():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "NCL"])
    assert (a.tau, a.ssl_reg, a.proto_reg, a.alpha, a.hyper_layers, a.num_clusters, a.proto_start) == \
        (0.2, 1e-6, 1e-7, 1.0, 1, 20, 20)
    a = parse_args(["--model", "NCL", "--proto_start", "3", "--hyper_layers", "0", "--ssl_reg", "1e-4"])
    assert (a.proto_start, a.hyper_layers, a.ssl_reg) == (3, 0, 1e-4)
    with pytest.raises(ValueError, match="NCL"):                 # the error message lists every name that resolves
        parse_args(["--model", "NoSuchModel"])


def test_hyper_layers_rule_width_rule_and_cpu_refusal():
    from coldrec_amd.model import AVAILABLE_MODELS
    _, data = builder()
    with pytest.raises(ValueError, match=r"need hyper_layers\*2 <= layers, got hyper_layers=2, layers=3"):
        AVAILABLE_MODELS["NCL"](_cfg(data, hyper_layers=2, layers=3))
    with pytest.raises(RuntimeError, match="above 256"):
        AVAILABLE_MODELS["NCL"](_cfg(data, emb_size=260))
    with pytest.raises(RuntimeError, match="MI355X only"):
        AVAILABLE_MODELS["NCL"](_cfg(data)).train()


def test_workspace_stays_linear_in_the_table():
    L = _lib.lib()
    table = 1_000_032 * 64 * 4
    assert 0 < L.crh_table_nce_workspace_bytes(2048, 1_000_000, 64) <= 2 * table + (64 << 20)
    assert L.crh_table_nce_workspace_bytes(2048, 1_000_000, 64) < 2048 * 1_000_000 * 4 // 8      # nothing of size B x N
    assert L.crh_table_nce_workspace_bytes(0, 10, 8) == 0 and L.crh_table_nce_splits(0, 10, 0) == -1
    # the row pass fills the grid with column splits where the batch is small (infonce's cap of 32 would starve it)
    assert L.crh_table_nce_splits(512, 1_000_000, 0) > 32 and L.crh_table_nce_splits(2048, 1_000_000, 1) == 1


def test_argument_errors_without_gpu():
    L = _lib.lib()
    f = L.crh_table_nce_f32
    p = 256                                                           # any non-NULL, aligned address: nothing is launched

    def call(ctx=p, table=p, n_rows=10, idx=p, batch=4, d=8, tau=0.2, g1=p, g2=p, loss=p, ws=p, ws_bytes=1 << 30):
        return f(ctx, table, n_rows, idx, None, batch, d, tau, 1.0, 0, g1, g2, loss, ws, ws_bytes, None)

    for kw, word in ((dict(table=None), "NULL ctx or table"), (dict(d=6), "multiple of 4"), (dict(d=260), "multiple of 4"),
                     (dict(g1=None, g2=None, loss=None), "nothing to compute"), (dict(idx=None), "NULL idx"),
                     (dict(batch=0), "batch_max"), (dict(n_rows=0), "n_rows"), (dict(tau=0.0), "tau")):
        assert call(**kw) == -1, kw
        assert word in L.crh_last_error().decode(), (kw, L.crh_last_error())
    assert call(ws_bytes=16) != 0 and "workspace" in L.crh_last_error().decode()


def test_ops_refuse_cpu_tensors():
    from coldrec_amd import ops
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.table_nce(torch.zeros(4, 8), torch.zeros(4, 8), torch.zeros(2, dtype=torch.int32), 0.2)


def test_float64_restatement_reproduces_the_references_ssl_g23():
    """Loss within 1e-6 relative, gradients within 1e-6 of their maximum, in both forms: the reference's formula under
    float64 autograd and the cancellation-free closed form the kernel is held to."""
    g = load_golden("g23_ssl.npz")
    for name in g["cases"]:
        name = str(name)
        U, tau = int(g[f"{name}_U"]), float(g[f"{name}_tau"])
        w_u = float(g[f"{name}_ssl_reg"])
        w_i = w_u * float(g[f"{name}_alpha"])
        init, alias = g[f"{name}_initial"], bool(g[f"{name}_alias"])
        ctx = init if alias else g[f"{name}_context"]
        user, item = g[f"{name}_user"], g[f"{name}_item"]
        want = float(g[f"{name}_loss"])
        for form in ("closed", "autograd"):
            g_ctx, g_init = np.zeros(init.shape), np.zeros(init.shape)
            loss = 0.0
            for lo, hi, idx, w in ((0, U, user, w_u), (U, init.shape[0], item, w_i)):
                if form == "closed":
                    _, l, gc, gt = ncl_restate.table_nce(ctx[lo:hi], init[lo:hi], idx, tau)
                elif alias:
                    l, gt, _ = ncl_restate.table_nce_autograd(init[lo:hi], init[lo:hi], idx, tau, alias=True)
                    gc = torch.zeros_like(gt)
                else:
                    l, gc, gt = ncl_restate.table_nce_autograd(ctx[lo:hi], init[lo:hi], idx, tau)
                loss += w * float(l)
                g_ctx[lo:hi] += w * gc.numpy()
                g_init[lo:hi] += w * gt.numpy()
            assert abs(loss - want) <= 1e-6 * abs(want), (name, form, loss, want)
            pairs = [(g_ctx + g_init, g[f"{name}_g_initial"])] if alias else \
                [(g_ctx, g[f"{name}_g_context"]), (g_init, g[f"{name}_g_initial"])]
            for got, ref in pairs:
                err = np.abs(got - ref).max() / np.abs(ref).max()
                print(f"g23_ssl {name} {form}: gradient error / max {err:.2e}")
                assert err <= 1e-6, (name, form, err)


def test_float64_restatement_reproduces_the_references_run_g23():
    """Every loss term of the reference's warm-up run within 1e-5 relative, from outside: same xavier tables (checksums), same
    triples.  Measured when the fixture was made: see the printed figure."""
    fx = load_golden("g23_ncl.npz")
    _, data = builder()
    got = ncl_restate.run_f64(data, int(fx["layers"]), int(fx["hyper_layers"]), int(fx["d"]), int(fx["epochs"]),
                              int(fx["batch_size"]), float(fx["tau"]), float(fx["ssl_reg"]), float(fx["alpha"]),
                              lr=float(fx["lr"]), reg=float(fx["reg"]), seed=int(fx["seed"]))
    assert got["U0_crc"] == int(fx["U0_crc"]) and got["V0_crc"] == int(fx["V0_crc"])
    want = fx["losses"]
    assert got["losses"].shape == want.shape == (int(fx["n_steps"]), 4)
    rel = np.abs(got["losses"] - want) / np.abs(want)
    print(f"g23_ncl: worst relative loss difference {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5
    weighted = float(fx["ssl_reg"]) * (want[0, 2] + float(fx["alpha"]) * want[0, 3])
    assert 0.1 * want[0, 0] <= weighted <= 10 * want[0, 0]           # the structure term is visible next to BPR


def _blobs(seed=0):
    rng = np.random.default_rng(seed)
    centres = np.array([[0.0, 0.0, 0.0, 0.0], [10.0, 0.0, 0.0, 0.0], [0.0, 10.0, 0.0, 10.0]], np.float32)
    x = np.concatenate([c + 0.3 * rng.standard_normal((40, 4)).astype(np.float32) for c in centres])
    return x[rng.permutation(x.shape[0])]


def test_kmeans_matches_its_numpy_restatement_on_separated_blobs():
    from coldrec_amd.train import lloyd_kmeans
    x = _blobs()
    for seed in range(3):
        start = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(seed))[:3]
        c, a = lloyd_kmeans(torch.from_numpy(x), start)
        c_np, a_np = ncl_restate.kmeans(x, start.numpy())
        assert a.dtype == torch.int64 and np.array_equal(a.numpy(), a_np)
        assert np.abs(c.numpy() - c_np).max() <= 1e-5
    # a start with one row per blob recovers the blobs: 40 rows each, centroids at the blob means
    d0 = ((x[:, None, :] - np.array([[0, 0, 0, 0], [10, 0, 0, 0], [0, 10, 0, 10]], np.float32)[None]) ** 2).sum(2).argmin(1)
    start = torch.tensor([int(np.flatnonzero(d0 == b)[0]) for b in range(3)])
    c, a = lloyd_kmeans(torch.from_numpy(x), start)
    assert np.array_equal(a.numpy(), d0)
    for b in range(3):
        assert np.abs(c[b].numpy() - x[d0 == b].mean(0)).max() <= 1e-5


def test_kmeans_empty_cluster_keeps_its_centroid():
    """k = 5 over two distinct points: the clusters that get no row keep the centroid they started from, and the global
    random stream is not touched by the engine's private generator."""
    from coldrec_amd.train import lloyd_kmeans
    x = torch.tensor([[0.0, 0.0]] * 4 + [[1.0, 1.0]] * 4)
    start = torch.tensor([0, 1, 2, 4, 5])
    c, a = lloyd_kmeans(x, start)
    c_np, a_np = ncl_restate.kmeans(x.numpy(), start.numpy())
    assert np.array_equal(a.numpy(), a_np) and np.array_equal(c.numpy(), c_np)
    assert sorted(set(a.tolist())) == [0, 3]                          # the first of equal centroids wins every tie
    assert torch.equal(c, x[start])                                    # the empty clusters 1, 2, 4 kept their start rows
