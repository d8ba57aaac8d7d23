"""GPU: the fused CLCRec loss (csrc/clcrec.hip) against the float64 restatement (tests/clcrec_restate.py, itself pinned to
the reference's run by tests/test_clcrec.py), its determinism contract, the autograd operator, the argument errors, and a
whole run against G20."""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import clcrec_restate
from tests.conftest import load_golden
from tests.test_contrastive_gpu import _lists_vs_reference, _metrics_vs_reference
from tests.test_host_logic import builder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

#        B    G    d   nu   ni    T   lam  num_sample
CASES = [(37, 5, 20, 11, 7, 2.0, 0.5, 0.5),          # every item repeats many times
         (64, 128, 64, 50, 400, 2.0, 0.5, 0.5),      # the defaults' group size
         (33, 1, 64, 9, 40, 0.1, 0.1, 1.0),
         (40, 16, 256, 300, 500, 0.5, 1.0, 0.0),     # nothing mixed
         (50, 8, 64, 5, 30, 0.2, 0.5, 0.5),          # one user, item 3 the positive of every record: the long segments
         (129, 256, 64, 300, 500, 1.0, 0.2, 0.1),
         (1, 3, 4, 2, 6, 2.0, 0.5, 0.5)]
REG = 1e-2      # (large enough for the regulariser's share of the gradients to be visible at the bar)


def _inputs(case, seed=0):
    B, G, d, nu, ni, T, lam, ns = case
    g = torch.Generator().manual_seed(1000 + seed + B * 7 + G)
    U, V = torch.randn(nu, d, generator=g) * 0.3, torch.randn(ni, d, generator=g) * 0.3
    users = torch.randint(nu, (B,), generator=g)
    items = torch.randint(ni, (B, 1 + G), generator=g)
    if (B, G) == (50, 8):
        users[:] = 2
        items[:, 0] = 3
    M = B * (1 + G)
    rand_index = torch.randint(M, (int(M * ns),), generator=g)
    n_slots = torch.unique(items).numel()
    E = torch.randn(n_slots, d, generator=g) * 0.5
    return U, V, E, users, items, rand_index


def _fused(case, inp, scale=1.0, want=(True, True, True)):
    from coldrec_amd import ops
    B, G, d, nu, ni, T, lam, ns = case
    U, V, E, users, items, rand_index = inp
    plan = ops.clcrec_plan(users.to(DEV), items.to(DEV), nu, ni)
    counts = torch.bincount(rand_index, minlength=B * (1 + G)).to(torch.int32).to(DEV)
    loss, gu, gv, ge = ops.clcrec(U.to(DEV), V.to(DEV), E.to(DEV), plan, counts, T, lam, REG, scale=scale,
                                  want_user=want[0], want_item=want[1], want_feat=want[2])
    torch.cuda.synchronize()
    return loss.cpu(), gu, gv, ge


@pytest.fixture(scope="module")
def oracle():
    """The float64 restatement of every case, computed once."""
    out = {}
    for case in CASES:
        inp = _inputs(case)
        out[case] = (inp, clcrec_restate.step(*inp, case[5], case[6], REG))
    return out


def _compare(tag, got, want, touched=None):
    loss, gu, gv, ge = got
    wl, wu, wv, we = want
    rel = np.abs(loss.numpy().astype(np.float64) - wl) / np.abs(wl)
    errs = []
    for name, g, w in (("dU", gu, wu), ("dV", gv, wv), ("dE", ge, we)):
        g = g.cpu().numpy().astype(np.float64)
        scale = np.abs(w).max()
        errs.append(np.abs(g - w).max() / scale if scale > 0 else np.abs(g).max())
        assert np.array_equal(g[(w == 0).all(1)], w[(w == 0).all(1)]), f"{tag}: {name} is not zero at an untouched row"
    print(f"{tag}: loss rel {rel.max():.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert rel.max() <= 1e-5
    assert max(errs) <= 1e-4


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-G%d-d%d" % c[:3])
def test_kernel_matches_float64_restatement(oracle, case):
    inp, want = oracle[case]
    nu, ni = case[3], case[4]
    got = _fused(case, inp)
    _compare("B%d G%d d%d" % case[:3], got, want)
    users, items = inp[3], inp[4]
    um = torch.ones(nu, dtype=torch.bool)
    um[users] = False
    im = torch.ones(ni, dtype=torch.bool)
    im[items.reshape(-1)] = False
    assert (got[1].cpu()[um] == 0).all() and (got[2].cpu()[im] == 0).all()       # rows no record touches: exactly zero


def test_mixing_is_count_weighted():
    """Some rows are drawn three times: dE carries three times the second softmax's term there (a flag would miss the bar)."""
    case = (24, 6, 32, 10, 25, 0.5, 0.3, 0.5)
    U, V, E, users, items, rand_index = _inputs(case, seed=5)
    rand_index = torch.cat([rand_index, torch.tensor([0, 0, 0, 9, 9, 9, 40, 40, 40])])
    inp = (U, V, E, users, items, rand_index)
    assert torch.bincount(rand_index).max() >= 3
    want = clcrec_restate.step(*inp, case[5], case[6], REG)
    _compare("counts", _fused(case, inp), want)
    flagged = clcrec_restate.step(U, V, E, users, items, torch.unique(rand_index), case[5], case[6], REG)
    assert np.abs(flagged[3] - want[3]).max() > 1e-2 * np.abs(want[3]).max()      # (the test can tell the two apart)


@pytest.mark.parametrize("case", [CASES[4], CASES[5]], ids=lambda c: "B%d-G%d" % c[:2])
def test_determinism_scale_and_null_gradients(oracle, case):
    inp, _ = oracle[case]
    a, b = _fused(case, inp), _fused(case, inp)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    half = _fused(case, inp, scale=0.5)
    assert torch.equal(half[0], a[0])
    for x, y in zip(a[1:], half[1:]):
        assert torch.equal(x * 0.5, y)
    for k in range(3):
        want = [True, True, True]
        want[k] = False
        part = _fused(case, inp, want=tuple(want))
        assert part[1 + k] is None and torch.equal(part[0], a[0])
        for j in range(3):
            if j != k:
                assert torch.equal(part[1 + j], a[1 + j])


def _toy_cfg(data, **kw):
    a = dict(dataset="toy", model="CLCRec", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, num_neg=16, temp_value=2.0, lr_lambda=0.5, num_sample=0.5)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=DEV)


def test_learner_loss_matches_torch_formula_under_autograd():
    """Learner.loss against the torch formula in float32 on the device, through torch.autograd.grad with grad_out = 0.7;
    the encoder's parameters receive dE (their summed gradient is compared too)."""
    from coldrec_amd.model.CLCRec import CLCRec_Learner
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    cfg = _toy_cfg(data, reg=1e-2)
    set_seed(3, True)
    m = CLCRec_Learner(cfg.args, data, 64, DEV).to(DEV)
    g = torch.Generator().manual_seed(11)
    users = torch.randint(data.user_num, (48,), generator=g).to(DEV)
    items = torch.randint(data.item_num, (48, 17), generator=g).to(DEV)
    params = [m.embedding_dict["user_emb"], m.embedding_dict["item_emb"], m.encoder_layer1.weight, m.encoder_layer1.bias,
              m.encoder_layer2.weight, m.encoder_layer2.bias]
    torch.manual_seed(5)
    got = torch.autograd.grad(m.loss(users, items), params, grad_outputs=torch.tensor(0.7, device=DEV))
    got_terms = m.last_terms.cpu().numpy().astype(np.float64)
    torch.manual_seed(5)
    rand_index = torch.randint(items.numel(), (int(items.numel() * 0.5),)).to(DEV)
    terms = clcrec_restate.loss_terms(params[0], params[1], m.encoder(items.reshape(-1)), users, items, rand_index, 2.0, 0.5,
                                      1e-2)
    want = torch.autograd.grad(terms[3], params, grad_outputs=torch.tensor(0.7, device=DEV))
    want_terms = np.array([float(t) for t in terms])
    rel = np.abs(got_terms - want_terms) / np.abs(want_terms)
    errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]
    sums = (float(sum(a.double().sum() for a in got[2:])), float(sum(b.double().sum() for b in want[2:])))
    print(f"autograd: loss rel {rel.max():.2e}, gradient err / max {errs}, encoder gradient sums {sums}")
    assert rel.max() <= 1e-5 and max(errs) <= 1e-4
    assert abs(sums[1]) > 0 and all(float(a.abs().max()) > 0 for a in got[2:])
    assert m.MLP.weight.grad is None and m.att_weight_1.grad is None


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    case = CASES[6]
    U, V, E, users, items, rand_index = _inputs(case)
    plan = ops.clcrec_plan(users.to(DEV), items.to(DEV))
    counts = torch.zeros(4, dtype=torch.int32, device=DEV)
    L = _lib.lib()

    def call(d=4, n_neg=3, ws_bytes=None):
        ws = ops.clcrec_workspace(1, 3, 4, plan["n_slots"], DEV)
        t = lambda x: x.to(DEV).contiguous()
        Ud, Vd, Ed = t(U), t(V), t(E)
        loss = torch.full((4,), -7.0, device=DEV)
        p = plan
        rc = L.crh_clcrec_f32(Ud.data_ptr(), Vd.data_ptr(), Ed.data_ptr(), p["users"].data_ptr(), p["items"].data_ptr(),
                              p["slot"].data_ptr(), p["slot_item"].data_ptr(), counts.data_ptr(), p["slot_ptr"].data_ptr(),
                              p["slot_rows"].data_ptr(), p["chunk_ptr"].data_ptr(), p["chunk_slot"].data_ptr(),
                              p["n_chunks"], p["user_ids"].data_ptr(), p["user_ptr"].data_ptr(), p["user_recs"].data_ptr(),
                              p["n_users"], 1, n_neg, d, p["n_slots"], 2.0, 0.5, 0.0, 1.0, None, None, None, loss.data_ptr(),
                              ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, _lib.current_stream())
        torch.cuda.synchronize()
        assert rc != 0 and (loss == -7.0).all()                   # nothing ran
        return L.crh_last_error().decode()

    assert "multiple of 4" in call(d=6)
    assert "n_neg = 0" in call(n_neg=0)
    assert "n_neg = %d" % (ops.clcrec_max_neg() + 1) in call(n_neg=ops.clcrec_max_neg() + 1)
    assert "workspace" in call(ws_bytes=16)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.clcrec(torch.zeros(2, 6, device=DEV), torch.zeros(6, 6, device=DEV), torch.zeros(plan["n_slots"], 6, device=DEV),
                   plan, counts, 2.0, 0.5, 0.0)


def _run(**kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle)."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    set_seed(2024, True)
    tr = AVAILABLE_MODELS["CLCRec"](_toy_cfg(data, **kw))
    tr.u0 = tr.model.embedding_dict["user_emb"].detach().clone().numpy()
    tr.v0 = tr.model.embedding_dict["item_emb"].detach().clone().numpy()
    tr.run()
    return tr


@pytest.fixture(scope="module")
def toy_run():
    return _run()


def test_run_matches_reference_g20(toy_run):
    """Structured as the G19 test.  The final-table bar is G19's 2e-4 of the table scale: plain float32 torch on the CPU
    ends 3.1e-6 / 2.6e-6 from G20 (tests/test_clcrec.py), so no wider bar is called for."""
    fx, tr = load_golden("g20_clcrec.npz"), toy_run
    assert clcrec_restate.crc(tr.u0) == int(fx["U0_crc"]) and clcrec_restate.crc(tr.v0) == int(fx["V0_crc"])
    assert tr.model.first_index_crc == int(fx["randint_crc"]), "torch's CPU integer stream differs from the fixture's"
    want = fx["losses"]
    assert tr.batch_losses.shape == want.shape
    rel = np.abs(tr.batch_losses - want) / np.abs(want)
    print(f"CLCRec: worst relative loss difference to G20 {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    U, V = fx["U"], fx["V"]
    eu = np.abs(tr.user_emb.cpu().numpy() - U).max() / np.abs(U).max()
    ev = np.abs(tr.item_emb.cpu().numpy() - V).max() / np.abs(V).max()
    print(f"CLCRec: final tables differ by {eu:.2e} / {ev:.2e} of their scale")
    assert eu < 2e-4 and ev < 2e-4
    same, det, total = _lists_vs_reference(tr, fx, U, V, min_frac=0.5)
    print(f"CLCRec: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    ref = dict(overall=fx["test_overall"], cold=fx["test_cold"], warm=fx["test_warm"],
               best=[int(fx["best_epoch"]), json.loads(str(fx["best_metrics"]))])
    _metrics_vs_reference(tr, ref, same == total)


def test_second_run_is_bit_identical(toy_run):
    b = _run()
    assert np.array_equal(toy_run.batch_losses, b.batch_losses)
    assert torch.equal(toy_run.user_emb, b.user_emb) and torch.equal(toy_run.item_emb, b.item_emb)


def test_cli_trains_end_to_end(tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "CLCRec", "--make_synthetic", "toy"] + common) is None
    pay = main(["--model", "CLCRec", "--num_neg", "16", "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "CLCRec" / "history.txt").is_file()
    for side in ("user", "item"):
        t = torch.load(tmp_path / "emb" / f"toy_cold_item_CLCRec_{side}_emb.pt", map_location="cpu")
        assert torch.is_tensor(t) and t.shape[1] == 64 and torch.isfinite(t).all()
