"""GPU: the SimGCL / XSimGCL engine (train.CLEngine) against the float64 restatement of tests/cl_restate.py fed the same
noise, and the built-in trainers end to end against G19 -- the reference's own SimGCL.run() / XSimGCL.run() on the toy
split (tests/golden/make_golden_g19.py)."""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import cl_restate
from tests.conftest import load_golden
from tests.test_e2e_gpu import _lists_vs_reference, _metrics_vs_reference
from tests.test_host_logic import builder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
HYPER = dict(eps=0.1, tau=0.2, cl_rate=0.5)
FIXTURE = {"SimGCL": "g19_simgcl.npz", "XSimGCL": "g19_xsimgcl.npz"}


def _cfg(data, model, **kw):
    a = dict(dataset="toy", model=model, epochs=2, layers=3, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, l_cl=2, cl_noise="host", **HYPER)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=DEV)


@pytest.fixture(scope="module")
def toy():
    """The toy graph, seeded xavier tables and one batch of 512 triples, shared by the step tests (never modified)."""
    from coldrec_amd.util.utils import epoch_triples, set_seed
    _, data = builder()
    set_seed(7, False)
    init = torch.nn.init.xavier_uniform_
    U0, V0 = init(torch.empty(data.user_num, 64)), init(torch.empty(data.item_num, 64))
    u, i, j = (np.asarray(t)[:512] for t in epoch_triples(data, 512))
    return dict(data=data, U0=U0, V0=V0, u=u, i=i, j=j, A=cl_restate.dense_adj(data))


CASES = [("simgcl", 1, 1), ("simgcl", 2, 1), ("simgcl", 3, 1),
         ("xsimgcl", 1, 1), ("xsimgcl", 2, 1), ("xsimgcl", 2, 2), ("xsimgcl", 3, 1), ("xsimgcl", 3, 3)]


@pytest.mark.parametrize("mode, L, l_cl", CASES)
def test_one_step_matches_float64_restatement(toy, mode, L, l_cl, monkeypatch):
    """Loss terms within 1e-5 relative, max|dE0 - dE0_f64| <= 1e-4 max|dE0_f64| (the bar tests/test_infonce_gpu.py holds
    the least exact ingredient to).  The optimiser in the last SpMM's epilogue and the separate gradient table + Adam
    launch give the same bits."""
    from coldrec_amd import ops
    from coldrec_amd.train import CLEngine
    data, lr, reg = toy["data"], 1e-3, 1e-4
    rowptr, col, val = data.norm_adj_csr()
    # float64, drawing the noise first from the same seeded CPU stream
    torch.manual_seed(99)
    E = torch.cat([toy["U0"], toy["V0"]], 0).double().requires_grad_()
    u, i, j = (torch.from_numpy(toy[k]).long() for k in ("u", "i", "j"))
    terms, total = cl_restate.step_f64(E, toy["A"], data.user_num, mode, L, l_cl, HYPER["eps"], HYPER["tau"],
                                       HYPER["cl_rate"], reg, u, i, j, cl_restate.host_noise(E.shape[0], 64))
    total.backward()
    want_g, want_l = E.grad.numpy(), np.array([float(t.detach()) for t in terms])
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("CRH_LGCN_FUSED", fused)
        eng = CLEngine(toy["U0"], toy["V0"], rowptr, col, val, L, lr, reg, DEV, mode=mode, l_cl=l_cl, noise="host", **HYPER)
        assert eng.fuse_adam == (fused == "1")
        eng.keep_grad = True
        ud, idd, jd = (torch.from_numpy(toy[k]).to(DEV) for k in ("u", "i", "j"))
        plan = ops.build_plans_device(ud, idd, jd, 512)[0]
        torch.manual_seed(99)
        eng.step(ud, idd, jd, plan)
        got[fused] = (eng.loss.cpu().numpy().astype(np.float64), eng.G.cpu().numpy(), eng.E.cpu().numpy())
        assert eng.step_count == 1
    loss, g, e_new = got["1"]
    rel = np.abs(loss - want_l) / np.abs(want_l)
    gerr = np.abs(g - want_g).max() / np.abs(want_g).max()
    print(f"{mode} L={L} l_cl={l_cl}: loss rel {rel.max():.2e}, dE0 err / max {gerr:.2e}")
    assert rel.max() <= 1e-5
    assert gerr <= 1e-4
    assert np.array_equal(got["0"][0], loss) and np.array_equal(got["0"][1], g) and np.array_equal(got["0"][2], e_new)
    e0 = torch.cat([toy["U0"], toy["V0"]], 0).numpy()
    assert np.abs(e_new - e0).max() <= 1.001 * lr and not np.array_equal(e_new, e0)      # one Adam step moves by <= lr


def test_second_step_sees_a_clean_gradient_table(toy):
    """The gradient table is cleared by the fused epilogue (L >= 2) or by the next step: two steps equal two engines' steps."""
    from coldrec_amd import ops
    from coldrec_amd.train import CLEngine
    data = toy["data"]
    rowptr, col, val = data.norm_adj_csr()
    ud, idd, jd = (torch.from_numpy(toy[k]).to(DEV) for k in ("u", "i", "j"))
    plan = ops.build_plans_device(ud, idd, jd, 512)[0]
    for mode, L, l_cl in (("simgcl", 1, 1), ("simgcl", 2, 1), ("xsimgcl", 2, 2), ("xsimgcl", 1, 1)):
        eng = CLEngine(toy["U0"], toy["V0"], rowptr, col, val, L, 1e-3, 1e-4, DEV, mode=mode, l_cl=l_cl, noise="device",
                       seed=5, **HYPER)
        eng.keep_grad = True
        eng.step(ud, idd, jd, plan)
        # same parameters, same draws, fresh buffers
        ref = CLEngine(eng.user_emb.cpu(), eng.item_emb.cpu(), rowptr, col, val, L, 1e-3, 1e-4, DEV, mode=mode, l_cl=l_cl,
                       noise="device", seed=5, **HYPER)
        ref.keep_grad, ref.draw = True, eng.draw
        eng.step(ud, idd, jd, plan)
        ref.step(ud, idd, jd, plan)
        assert torch.equal(eng.G, ref.G) and torch.equal(eng.loss, ref.loss), (mode, L, l_cl)


def _run(name, **kw):
    """A whole run on a FRESH builder: the sampler keeps the reference's cumulative in-place shuffle of the training
    records, so a second run on the same builder would see other batches."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    set_seed(2024, True)
    tr = AVAILABLE_MODELS[name](_cfg(data, name, **kw))
    tr.run()
    return tr


@pytest.mark.parametrize("name", ["SimGCL", "XSimGCL"])
def test_run_with_host_noise_matches_reference_g19(name):
    fx = load_golden(FIXTURE[name])
    tr = _run(name, cl_noise="host")
    assert cl_restate.crc(tr.model.user0.numpy()) == int(fx["U0_crc"])
    assert cl_restate.crc(tr.model.item0.numpy()) == int(fx["V0_crc"])
    assert tr.engine.first_noise_crc == int(fx["noise_crc"]), "torch's CPU uniform stream differs from the fixture's"
    want = fx["losses"]
    assert tr.batch_losses.shape == want.shape
    rel = np.abs(tr.batch_losses - want) / np.abs(want)
    print(f"{name}: worst relative loss difference to G19 {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    U, V = fx["U"], fx["V"]
    eu = np.abs(tr.user_emb.cpu().numpy() - U).max() / np.abs(U).max()
    ev = np.abs(tr.item_emb.cpu().numpy() - V).max() / np.abs(V).max()
    print(f"{name}: final tables differ by {eu:.2e} / {ev:.2e} of their scale")
    assert eu < 2e-4 and ev < 2e-4
    assert tr.best_user_emb.data_ptr() != tr.engine.OUT.data_ptr()            # save() is a real snapshot of the clean pass
    same, det, total = _lists_vs_reference(tr, fx, U, V, min_frac=0.5)
    print(f"{name}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    ref = dict(overall=fx["test_overall"], cold=fx["test_cold"], warm=fx["test_warm"],
               best=[int(fx["best_epoch"]), json.loads(str(fx["best_metrics"]))])
    _metrics_vs_reference(tr, ref, same == total)


@pytest.mark.parametrize("name", ["SimGCL", "XSimGCL"])
def test_run_with_device_noise(name):
    """Other noise, same distribution: the run completes, every loss is finite, the first batch's contrastive terms are
    within 5 % of G19's, and the same seed gives the same losses bit for bit."""
    fx = load_golden(FIXTURE[name])
    a = _run(name, cl_noise="device")
    b = _run(name, cl_noise="device")
    assert a.batch_losses.shape == fx["losses"].shape and np.isfinite(a.batch_losses).all()
    rel = np.abs(a.batch_losses[0, 2:] - fx["losses"][0, 2:]) / fx["losses"][0, 2:]
    print(f"{name}: first-batch contrastive terms differ from G19's by {rel}")
    assert (rel <= 0.05).all()
    assert np.array_equal(a.batch_losses, b.batch_losses)
    assert torch.equal(a.user_emb, b.user_emb) and torch.equal(a.item_emb, b.item_emb)
    c = _run(name, cl_noise="device", seed=2025)                         # (set_seed stays 2024: only the noise key moves)
    assert not np.array_equal(a.batch_losses[:, 2:], c.batch_losses[:, 2:])
    if name == "SimGCL":                                                       # its BPR / L2 terms come from the clean pass
        assert np.array_equal(a.batch_losses[0, :2], c.batch_losses[0, :2])


def test_cli_trains_both_models_end_to_end(tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "SimGCL", "--make_synthetic", "toy"] + common) is None
    pay = main(["--model", "SimGCL", "--layers", "2", "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "SimGCL" / "history.txt").is_file()
    pay = main(["--model", "XSimGCL", "--layers", "3", "--l_cl", "2", "--epochs", "2", "--cl_noise", "host"] + common)
    assert set(pay["20"]) == {"all", "cold", "warm"} and (tmp_path / "result" / "XSimGCL" / "history.txt").is_file()
    for model in ("SimGCL", "XSimGCL"):
        for side in ("user", "item"):
            t = torch.load(tmp_path / "emb" / f"toy_cold_item_{model}_{side}_emb.pt", map_location="cpu")
            assert torch.is_tensor(t) and t.shape[1] == 64 and torch.isfinite(t).all()
    with pytest.raises(ValueError, match="1 <= l_cl <= layers"):
        main(["--model", "XSimGCL", "--layers", "2", "--l_cl", "3", "--epochs", "1"] + common)


@pytest.mark.parametrize("mode, noise", [("simgcl", "host"), ("xsimgcl", "host"), ("simgcl", "device")])
def test_width_that_is_no_multiple_of_four(mode, noise):
    """--emb_size 50: the tables carry two zero columns; the noise row is normalised over the 50 logical columns and the
    pad columns stay exactly zero."""
    from coldrec_amd import ops
    from coldrec_amd.train import CLEngine
    from coldrec_amd.util.utils import epoch_triples, set_seed
    _, data = builder()
    set_seed(3, False)
    init = torch.nn.init.xavier_uniform_
    U0, V0 = init(torch.empty(data.user_num, 50)), init(torch.empty(data.item_num, 50))
    u, i, j = (np.asarray(t)[:300] for t in epoch_triples(data, 512))
    rowptr, col, val = data.norm_adj_csr()
    eng = CLEngine(U0, V0, rowptr, col, val, 2, 1e-3, 1e-4, DEV, mode=mode, l_cl=2, noise=noise, seed=9, **HYPER)
    eng.keep_grad = True
    ud, idd, jd = (torch.from_numpy(t).to(DEV) for t in (u, i, j))
    torch.manual_seed(42)
    eng.step(ud, idd, jd, ops.build_plans_device(ud, idd, jd, 300)[0])
    assert eng.E.shape[1] == 52 and float(eng.E[:, 50:].abs().max()) == 0.0 and float(eng.G[:, 50:].abs().max()) == 0.0
    assert float(eng.P[0][:, 50:].abs().max()) == 0.0 and torch.isfinite(eng.loss).all()
    if noise == "device":                      # (no reference for this stream: finite, and the pad columns untouched)
        return
    torch.manual_seed(42)
    E = torch.cat([U0, V0], 0).double().requires_grad_()
    terms, total = cl_restate.step_f64(E, cl_restate.dense_adj(data), data.user_num, mode, 2, 2, HYPER["eps"], HYPER["tau"],
                                       HYPER["cl_rate"], 1e-4, *(torch.from_numpy(t).long() for t in (u, i, j)),
                                       cl_restate.host_noise(E.shape[0], 50))
    total.backward()
    want_l = np.array([float(t.detach()) for t in terms])
    assert (np.abs(eng.loss.cpu().numpy() - want_l) / np.abs(want_l)).max() <= 1e-5
    g = eng.G[:, :50].cpu().numpy()
    assert np.abs(g - E.grad.numpy()).max() <= 1e-4 * np.abs(E.grad.numpy()).max()


@pytest.mark.parametrize("mode, L", [("simgcl", 1), ("simgcl", 3), ("xsimgcl", 2)])
def test_sgd_optimizer_applies_the_same_gradient(toy, mode, L, monkeypatch):
    """--optimizer sgd: E <- fma(-lr, dE0, E), in the last SpMM's epilogue or by the dense kernel -- never Adam."""
    from coldrec_amd import ops
    from coldrec_amd.train import CLEngine
    data = toy["data"]
    rowptr, col, val = data.norm_adj_csr()
    ud, idd, jd = (torch.from_numpy(toy[k]).to(DEV) for k in ("u", "i", "j"))
    plan = ops.build_plans_device(ud, idd, jd, 512)[0]
    e0 = torch.cat([toy["U0"], toy["V0"]], 0).to(DEV)
    outs = []
    for fused in ("1", "0"):
        monkeypatch.setenv("CRH_LGCN_FUSED", fused)
        eng = CLEngine(toy["U0"], toy["V0"], rowptr, col, val, L, 0.05, 1e-4, DEV, optimizer="sgd", mode=mode, l_cl=L,
                       noise="device", seed=4, **HYPER)
        eng.keep_grad = True
        assert eng.M is None
        eng.step(ud, idd, jd, plan)
        assert float((eng.E - (e0 - 0.05 * eng.G)).abs().max()) <= 2.0 ** -23 * float(e0.abs().max())     # fma vs two roundings
        assert float(eng.G.abs().max()) > 0
        outs.append((eng.E.clone(), eng.G.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
