"""GPU: the NCL engine (train.NCLEngine) against the float64 restatement of tests/ncl_restate.py, and the built-in trainer
end to end against G23 -- the reference's own NCL.run() on the toy split (tests/golden/make_golden_g23.py).  Bars of the
step tests: tests/test_contrastive_gpu.py's -- loss terms within 1e-5 relative, dE0 within 1e-4 of its maximum."""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import cl_restate, ncl_restate
from tests.conftest import load_golden
from tests.test_e2e_gpu import _lists_vs_reference, _metrics_vs_reference
from tests.test_host_logic import builder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# ssl_reg / proto_reg far above the reference's defaults: every term has to show in dE0 next to BPR's
HYPER = dict(tau=0.2, ssl_reg=1e-4, alpha=0.7, proto_reg=1e-5, num_clusters=5, batch_size=512)


def _cfg(data, **kw):
    a = dict(dataset="toy", model="NCL", epochs=2, layers=3, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, tau=0.2, ssl_reg=1e-4, proto_reg=1e-7, alpha=1.0, hyper_layers=1, num_clusters=20, proto_start=20)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=DEV)


@pytest.fixture(scope="module")
def toy():
    """The toy graph, seeded xavier tables and one batch of 512 triples, shared by the step tests (never modified)."""
    from coldrec_amd import ops
    from coldrec_amd.util.utils import epoch_triples, set_seed
    _, data = builder()
    set_seed(7, False)
    init = torch.nn.init.xavier_uniform_
    U0, V0 = init(torch.empty(data.user_num, 64)), init(torch.empty(data.item_num, 64))
    u, i, j = (np.asarray(t)[:512] for t in epoch_triples(data, 512))
    dev = tuple(torch.from_numpy(t).to(DEV) for t in (u, i, j))
    return dict(data=data, U0=U0, V0=V0, u=u, i=i, j=j, A=cl_restate.dense_adj(data), csr=data.norm_adj_csr(), dev=dev,
                plan=ops.build_plans_device(*dev, 512)[0])


def _engine(toy, L, h, **kw):
    from coldrec_amd.train import NCLEngine
    eng = NCLEngine(toy["U0"], toy["V0"], *toy["csr"], L, 1e-3, 1e-4, DEV, hyper_layers=h, **{**HYPER, **kw})
    eng.keep_grad = True
    return eng


def _restate(toy, L, h, proto=None, E0=None):
    E0 = torch.cat([toy["U0"], toy["V0"]], 0) if E0 is None else E0
    terms, _, g = ncl_restate.ncl_step(E0, toy["A"], toy["data"].user_num, toy["u"], toy["i"], toy["j"], L, h, 1e-4,
                                       HYPER["tau"], HYPER["ssl_reg"], HYPER["alpha"], proto)
    return terms.numpy(), g.numpy()


def _check(loss, g, want_l, want_g, label, n_terms=4):
    rel = np.abs(loss[:n_terms] - want_l[:n_terms]) / np.abs(want_l[:n_terms])
    gerr = np.abs(g - want_g).max() / np.abs(want_g).max()
    print(f"{label}: loss rel {rel.max():.2e}, dE0 err / max {gerr:.2e}")
    assert rel.max() <= 1e-5, (label, rel)
    assert gerr <= 1e-4, (label, gerr)


@pytest.mark.parametrize("L, h", [(1, 0), (2, 1), (3, 1), (4, 1), (4, 2)])
def test_one_step_matches_float64_restatement(toy, L, h, monkeypatch):
    """The optimiser in the last SpMM's epilogue and the separate gradient table + Adam launch give the same bits."""
    want_l, want_g = _restate(toy, L, h)
    # without the structure terms dE0 is another gradient: the bar below would see them missing
    no_ssl = ncl_restate.ncl_step(torch.cat([toy["U0"], toy["V0"]], 0), toy["A"], toy["data"].user_num, toy["u"], toy["i"],
                                  toy["j"], L, h, 1e-4, HYPER["tau"], 0.0, HYPER["alpha"])[2].numpy()
    assert np.abs(no_ssl - want_g).max() > 1e-2 * np.abs(want_g).max()
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("CRH_LGCN_FUSED", fused)
        eng = _engine(toy, L, h)
        assert eng.fuse_adam == (fused == "1")
        eng.step(*toy["dev"], toy["plan"])
        got[fused] = (eng.loss.cpu().numpy().astype(np.float64), eng.G.cpu().numpy(), eng.E.cpu().numpy())
        assert eng.step_count == 1
    loss, g, e_new = got["1"]
    _check(loss, g, want_l, want_g, f"L={L} h={h}")
    assert loss[4] == 0.0 and loss[5] == 0.0                           # warm-up: no prototype terms
    assert np.array_equal(got["0"][0], loss) and np.array_equal(got["0"][1], g) and np.array_equal(got["0"][2], e_new)
    e0 = torch.cat([toy["U0"], toy["V0"]], 0).numpy()
    assert np.abs(e_new - e0).max() <= 1.001 * 1e-3 and not np.array_equal(e_new, e0)    # one Adam step moves by <= lr


def test_second_step_sees_clean_gradient_tables(toy):
    """Two steps of one engine equal the second step of a fresh engine started from the first step's tables."""
    from coldrec_amd.train import NCLEngine
    for L, h in ((1, 0), (2, 1), (3, 1)):
        eng = _engine(toy, L, h)
        eng.step(*toy["dev"], toy["plan"])
        ref = NCLEngine(eng.user_emb.cpu(), eng.item_emb.cpu(), *toy["csr"], L, 1e-3, 1e-4, DEV, hyper_layers=h, **HYPER)
        ref.keep_grad = True
        eng.step(*toy["dev"], toy["plan"])
        ref.step(*toy["dev"], toy["plan"])
        assert torch.equal(eng.G, ref.G) and torch.equal(eng.loss, ref.loss), (L, h)


def test_a_prototype_phase_step_with_given_clusters(toy):
    """Centroids and assignments handed to the engine: all six terms and dE0 against the restatement."""
    data = toy["data"]
    U, I, k = data.user_num, data.item_num, 5
    g = torch.Generator().manual_seed(11)
    proto = dict(proto_reg=HYPER["proto_reg"], batch_size=512,
                 user_centroids=torch.randn(k, 64, generator=g) * 0.1, user_2cluster=torch.randint(0, k, (U,), generator=g),
                 item_centroids=torch.randn(k, 64, generator=g) * 0.1, item_2cluster=torch.randint(0, k, (I,), generator=g))
    want_l, want_g = _restate(toy, 3, 1, proto)
    base_g = _restate(toy, 3, 1)[1]
    assert np.abs(base_g - want_g).max() > 1e-2 * np.abs(want_g).max()     # the prototype terms show in dE0
    eng = _engine(toy, 3, 1)
    eng.proto = tuple(proto[n].to(DEV) for n in ("user_centroids", "user_2cluster", "item_centroids", "item_2cluster"))
    eng.step(*toy["dev"], toy["plan"])
    loss, got_g = eng.loss.cpu().numpy().astype(np.float64), eng.G.cpu().numpy()
    _check(loss, got_g, want_l, want_g, "proto step", n_terms=6)
    total = want_l[0] + want_l[1] + HYPER["ssl_reg"] * (want_l[2] + HYPER["alpha"] * want_l[3]) \
        + HYPER["proto_reg"] * 512 * (want_l[4] + want_l[5])
    assert abs(eng.last_loss() - total) <= 1e-5 * abs(total)


def test_width_that_is_no_multiple_of_four():
    """--emb_size 50: the tables carry two zero columns; they stay exactly zero in E, G and CTX, and the step matches."""
    from coldrec_amd import ops
    from coldrec_amd.train import NCLEngine
    from coldrec_amd.util.utils import epoch_triples, set_seed
    _, data = builder()
    set_seed(3, False)
    init = torch.nn.init.xavier_uniform_
    U0, V0 = init(torch.empty(data.user_num, 50)), init(torch.empty(data.item_num, 50))
    u, i, j = (np.asarray(t)[:300] for t in epoch_triples(data, 512))
    eng = NCLEngine(U0, V0, *data.norm_adj_csr(), 2, 1e-3, 1e-4, DEV, hyper_layers=1, **HYPER)
    eng.keep_grad = True
    ud, idd, jd = (torch.from_numpy(t).to(DEV) for t in (u, i, j))
    eng.step(ud, idd, jd, ops.build_plans_device(ud, idd, jd, 300)[0])
    assert eng.E.shape[1] == 52
    for t in (eng.E, eng.G, eng.CTX, eng.G0, eng.GC):
        assert float(t[:, 50:].abs().max()) == 0.0
    terms, _, g = ncl_restate.ncl_step(torch.cat([U0, V0], 0), cl_restate.dense_adj(data), data.user_num, u, i, j, 2, 1, 1e-4,
                                       HYPER["tau"], HYPER["ssl_reg"], HYPER["alpha"])
    _check(eng.loss.cpu().numpy().astype(np.float64), eng.G[:, :50].cpu().numpy(), terms.numpy(), g.numpy(), "width 50")


def _run(**kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle)."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    set_seed(2024, True)
    tr = AVAILABLE_MODELS["NCL"](_cfg(data, **kw))
    tr.run()
    return tr


def test_run_matches_reference_g23():
    fx = load_golden("g23_ncl.npz")
    tr = _run(ssl_reg=float(fx["ssl_reg"]), layers=int(fx["layers"]), hyper_layers=int(fx["hyper_layers"]))
    assert cl_restate.crc(tr.model.user0.numpy()) == int(fx["U0_crc"])
    assert cl_restate.crc(tr.model.item0.numpy()) == int(fx["V0_crc"])
    want = fx["losses"]
    assert tr.batch_losses.shape == (want.shape[0], 6) and (tr.batch_losses[:, 4:] == 0).all()
    rel = np.abs(tr.batch_losses[:, :4] - want) / np.abs(want)
    print(f"NCL: worst relative loss difference to G23 {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    U, V = fx["U"], fx["V"]
    eu = np.abs(tr.user_emb.cpu().numpy() - U).max() / np.abs(U).max()
    ev = np.abs(tr.item_emb.cpu().numpy() - V).max() / np.abs(V).max()
    print(f"NCL: final tables differ by {eu:.2e} / {ev:.2e} of their scale")
    assert eu < 2e-4 and ev < 2e-4
    assert tr.best_user_emb.data_ptr() != tr.engine.OUT.data_ptr()            # save() is a real snapshot
    same, det, total = _lists_vs_reference(tr, fx, U, V, min_frac=0.5)
    print(f"NCL: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    ref = dict(overall=fx["test_overall"], cold=fx["test_cold"], warm=fx["test_warm"],
               best=[int(fx["best_epoch"]), json.loads(str(fx["best_metrics"]))])
    _metrics_vs_reference(tr, ref, same == total)


def test_run_that_reaches_the_prototype_phase(capsys):
    kw = dict(proto_start=1, epochs=3, num_clusters=5, proto_reg=1e-5)
    a = _run(**kw)
    out = capsys.readouterr().out
    assert "warm_up batch_loss:" in out and "batch 0 batch_loss:" in out
    b = _run(**kw)
    steps = a.batch_losses.shape[0] // 3
    assert a.batch_losses.shape == (3 * steps, 6) and np.isfinite(a.batch_losses).all()
    assert (a.batch_losses[:steps, 4:] == 0).all() and (a.batch_losses[steps:, 4:] > 0).all()
    assert a.engine.proto[0].shape == (5, 64) and a.engine.proto[1].shape == (a.data.user_num,)
    assert np.array_equal(a.batch_losses, b.batch_losses)
    assert torch.equal(a.user_emb, b.user_emb) and torch.equal(a.item_emb, b.item_emb)


def test_cli_trains_ncl_end_to_end(tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "NCL", "--make_synthetic", "toy"] + common) is None
    pay = main(["--model", "NCL", "--layers", "2", "--epochs", "2", "--proto_start", "1", "--num_clusters", "5"] + common)
    assert set(pay) == {"10", "20"} and set(pay["20"]) == {"all", "cold", "warm"}
    assert (tmp_path / "result" / "NCL" / "history.txt").is_file()
    for side in ("user", "item"):
        t = torch.load(tmp_path / "emb" / f"toy_cold_item_NCL_{side}_emb.pt", map_location="cpu")
        assert torch.is_tensor(t) and t.shape[1] == 64 and torch.isfinite(t).all()
    with pytest.raises(ValueError, match="hyper_layers"):
        main(["--model", "NCL", "--layers", "1", "--hyper_layers", "1", "--epochs", "1"] + common)
