"""GPU: the fused CCFCRec loss (csrc/ccfcrec.hip) against the float64 restatement (tests/ccfcrec_restate.py, itself pinned
to the reference's run by tests/test_ccfcrec.py), its determinism contract, the autograd operator, the argument errors,
and whole runs against G21.

Bars of the kernel against the float64 restatement: 8x the worst distance of the float32 torch formula (CPU) from the
float64 one at the same cases -- both are fp32 sums over up to R ~ 1000 terms in other orders, while a wrong coefficient
or a missed occurrence shows at 1e-2 or more.  Measured on the CPU (tests/test_ccfcrec.py prints them again):
    loss terms, relative:          worst 1.35e-7 (B50-P2-N8)       -> LOSS_BAR = 1.08e-6
    gradients, error / maximum:    worst 3.84e-7 (B50-P2-N8, dQ)   -> GRAD_BAR = 3.07e-6
(the other cases: loss 6e-8 .. 1.1e-7, gradients 1.4e-7 .. 2.1e-7; one and eight CPU threads give the same figures)
"""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import ccfcrec_restate
from tests.conftest import load_golden
from tests.test_contrastive_gpu import _lists_vs_reference, _metrics_vs_reference
from tests.test_host_logic import builder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_LOSS_WORST, F32_GRAD_WORST = 1.35e-7, 3.84e-7         # float32 torch against float64 torch, measured (see above)
LOSS_BAR, GRAD_BAR = 8 * F32_LOSS_WORST, 8 * F32_GRAD_WORST

#        B    P    N   S    d   nu   ni   tau  lambda1
CASES = [(1, 1, 1, 1, 4, 3, 4, 0.1, 0.6),              # smallest everything
         (37, 2, 5, 3, 20, 11, 3, 0.1, 0.1),           # three items: owners of many chunks; width no power of two
         (16, 5, 40, 40, 64, 50, 400, 0.1, 0.6),       # the defaults' row count
         (33, 3, 7, 1, 132, 9, 40, 0.1, 1.0),
         (40, 1, 16, 9, 256, 300, 500, 0.1, 0.1),
         (50, 2, 8, 8, 64, 2, 30, 0.05, 0.6),          # one u_b, one k_b: the long user segments; scores span +-20
         (129, 4, 255, 3, 64, 300, 500, 0.1, 1.0)]     # R = 1028 > 1024
IDS = lambda c: "B%d-P%d-N%d-S%d-d%d" % c[:5]


def _inputs(case, seed=0):
    B, P, N, S, d, nu, ni, tau, lam = case
    g = torch.Generator().manual_seed(2000 + seed + B * 7 + N)
    U, V = torch.randn(nu, d, generator=g) * 0.3, torch.randn(ni, d, generator=g) * 0.3
    Q = torch.randn(B, d, generator=g) * 0.5
    users, neg_users = torch.randint(nu, (B,), generator=g), torch.randint(nu, (B,), generator=g)
    items = torch.randint(ni, (B,), generator=g)
    pos, neg = torch.randint(ni, (B, P), generator=g), torch.randint(ni, (B, P, N), generator=g)
    sneg = torch.randint(ni, (B, S), generator=g)
    if ni == 3:                      # item 1 is i_b, a positive, a negative and a self-negative of record 0
        items[0], pos[0, 0], neg[0, 0, 0], sneg[0, 0] = 1, 1, 1, 1
    if nu == 2:                      # all records share u_b; items 0 / 1 lie along / against every second q_b
        users[:], neg_users[:] = 0, 1
        w = torch.randn(d, generator=g) * 0.3
        V[0], V[1] = w, -1.5 * w
        Q[::2] = 0.7 * w + 0.005 * torch.randn(Q[::2].shape, generator=g)
    return U, V, Q, users, items, neg_users, pos, neg, sneg


def _fused(case, inp, scale=1.0, want=(True, True, True)):
    from coldrec_amd import ops
    nu, ni, tau, lam = case[5:]
    U, V, Q = (t.to(DEV) for t in inp[:3])
    plan = ops.ccfcrec_plan(*(t.to(DEV) for t in inp[3:]), nu, ni)
    loss, gu, gv, gq = ops.ccfcrec(U, V, Q, plan, tau, lam, scale=scale, want_user=want[0], want_item=want[1],
                                   want_q=want[2])
    torch.cuda.synchronize()
    return loss.cpu(), gu, gv, gq


@pytest.fixture(scope="module")
def oracle():
    """The float64 restatement of every case, computed once."""
    out = {}
    for case in CASES:
        inp = _inputs(case)
        out[case] = (inp, ccfcrec_restate.step(*inp, case[7], case[8]))
    return out


def distances(got, want):
    """(worst relative error of the loss terms, [error / maximum of dU, dV, dQ]) of (terms, dU, dV, dQ) numpy tuples."""
    rel = np.abs(np.asarray(got[0], np.float64) - want[0]) / np.abs(want[0])
    errs = []
    for g, w in zip(got[1:], want[1:]):
        top = np.abs(w).max()
        errs.append(np.abs(np.asarray(g, np.float64) - w).max() / top if top > 0 else np.abs(g).max())
    return rel.max(), errs


def _compare(tag, got, want):
    loss, gu, gv, gq = got
    got = (loss.numpy(), gu.cpu().numpy(), gv.cpu().numpy(), gq.cpu().numpy())
    rel, errs = distances(got, want)
    print(f"{tag}: loss rel {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    for name, g, w in (("dU", got[1], want[1]), ("dV", got[2], want[2])):
        assert not g[(w == 0).all(1)].any(), f"{tag}: {name} is not zero at an untouched row"
    assert rel <= LOSS_BAR
    assert max(errs) <= GRAD_BAR


def test_shape_admits_the_large_case():
    from coldrec_amd import ops
    assert ops.ccfcrec_rows(*CASES[6][1:4]) == 1028 <= ops.ccfcrec_max_rows()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_matches_float64_restatement(oracle, case):
    inp, want = oracle[case]
    nu, ni = case[5], case[6]
    got = _fused(case, inp)
    _compare(IDS(case), got, want)
    um = torch.ones(nu, dtype=torch.bool)
    um[inp[3]] = False
    um[inp[5]] = False
    im = torch.ones(ni, dtype=torch.bool)
    for t in (inp[4], inp[6], inp[7], inp[8]):
        im[t.reshape(-1)] = False
    assert (got[1].cpu()[um] == 0).all() and (got[2].cpu()[im] == 0).all()       # rows no record touches: exactly zero


def test_contrast_loss_is_divided_by_p_once(oracle):
    """P = 5: the restatement without the 1/P differs from the correct one by far more than 100 bars."""
    case = CASES[2]
    inp, want = oracle[case]
    wrong = ccfcrec_restate.step(*inp, case[7], case[8], divide_by_p=False)
    rel, errs = distances(wrong, want)
    assert rel > 100 * LOSS_BAR and max(errs) > 100 * GRAD_BAR                    # (the test can tell the two apart)
    _compare("1/P", _fused(case, inp), want)


@pytest.mark.parametrize("case", [CASES[1], CASES[5]], ids=IDS)
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
    a = dict(dataset="toy", model="CCFCRec", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, positive_number=3, negative_number=8, self_neg_number=8, tau=0.1, lambda1=0.6,
             attr_present_dim=64, implicit_dim=64, cat_implicit_dim=64, pretrain=False, pretrain_update=False)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=DEV)


def test_learner_loss_matches_torch_formula_under_autograd():
    """Learner.loss against the torch formula in float32 on the device, through torch.autograd.grad with grad_out = 0.7;
    the encoder's parameters receive dQ (attr_matrix, attr_W1 and the generator layers are compared)."""
    from coldrec_amd.model.CCFCRec import CCFCRec_Learner
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    cfg = _toy_cfg(data)
    set_seed(3, True)
    m = CCFCRec_Learner(cfg.args, data, 64, DEV).to(DEV)
    g = torch.Generator().manual_seed(11)
    B, P, N, S = 48, 3, 8, 8
    ru = lambda *shape: torch.randint(data.user_num, shape, generator=g).to(DEV)
    ri = lambda *shape: torch.randint(data.item_num, shape, generator=g).to(DEV)
    ids = (ru(B), ri(B), ru(B), ri(B, P), ri(B, P, N), ri(B, S))
    params = [m.user_embedding, m.item_embedding, m.attr_matrix, m.attr_W1, m.gen_layer1.weight, m.gen_layer1.bias,
              m.gen_layer2.weight, m.gen_layer2.bias]
    out = torch.tensor(0.7, device=DEV)
    got = torch.autograd.grad(m.loss(*ids), params, grad_outputs=out)
    got_terms = m.last_terms.cpu().numpy().astype(np.float64)
    terms = ccfcrec_restate.loss_terms(params[0], params[1], m(ids[0], ids[1]), *ids, 0.1, 0.6)
    want = torch.autograd.grad(terms[4], params, grad_outputs=out)
    want_terms = np.array([float(t.detach()) for t in terms])
    rel = np.abs(got_terms - want_terms) / np.abs(want_terms)
    errs = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(got, want)]
    print(f"autograd: loss rel {rel.max():.2e}, gradient err / max {errs}")
    # two float32 evaluations, each within its bar of the float64 value (the encoder's gradients are sums of dQ rows)
    assert rel.max() <= 2 * LOSS_BAR and max(errs) <= 2 * GRAD_BAR
    assert all(float(a.abs().max()) > 0 for a in got[2:])


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    case = CASES[0]
    inp = _inputs(case)
    plan = ops.ccfcrec_plan(*(t.to(DEV) for t in inp[3:]))
    L = _lib.lib()
    cap = ops.ccfcrec_max_rows()

    def call(d=4, n_neg=1, ws_bytes=None, item_rows=4, user_rows=3):
        ws = ops.ccfcrec_workspace(1, 1, 1, 1, 4, plan["n_items"], plan["n_users"], DEV)
        Ud, Vd, Qd = (t.to(DEV).contiguous() for t in inp[:3])
        loss = torch.full((5,), -7.0, device=DEV)
        p = plan
        rc = L.crh_ccfcrec_f32(Ud.data_ptr(), user_rows, Vd.data_ptr(), item_rows, Qd.data_ptr(), p["users"].data_ptr(),
                               p["neg_users"].data_ptr(), p["items"].data_ptr(), p["user_range"][0], p["user_range"][1],
                               p["item_range"][0], p["item_range"][1], p["item_ids"].data_ptr(), p["item_ptr"].data_ptr(),
                               p["item_occ"].data_ptr(), p["item_chunk_ptr"].data_ptr(), p["item_chunk_own"].data_ptr(),
                               p["n_items"], p["n_item_chunks"], p["user_ids"].data_ptr(), p["user_ptr"].data_ptr(),
                               p["user_occ"].data_ptr(), p["user_chunk_ptr"].data_ptr(), p["user_chunk_own"].data_ptr(),
                               p["n_users"], p["n_user_chunks"], 1, 1, n_neg, 1, d, 0.1, 0.6, 1.0, None, None, None,
                               loss.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                               _lib.current_stream())
        torch.cuda.synchronize()
        assert rc != 0 and (loss == -7.0).all()                   # nothing ran
        return L.crh_last_error().decode()

    assert "multiple of 4" in call(d=6)
    assert "n_neg = 0" in call(n_neg=0)
    assert "above the cap %d" % cap in call(n_neg=cap)
    assert "workspace" in call(ws_bytes=16)
    assert "outside the item table" in call(item_rows=plan["item_range"][1])
    assert "outside the user table" in call(user_rows=plan["user_range"][1])
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.ccfcrec(torch.zeros(3, 6, device=DEV), torch.zeros(4, 6, device=DEV), torch.zeros(1, 6, device=DEV), plan, 0.1,
                    0.6)
    with pytest.raises(RuntimeError, match="outside the item table"):
        ops.ccfcrec_plan(*(t.to(DEV) for t in inp[3:]), 3, int(plan["item_range"][1]))
    with pytest.raises(RuntimeError, match="outside the tables"):
        ops.ccfcrec(inp[0][:plan["user_range"][1]].to(DEV).contiguous(), inp[1].to(DEV), inp[2].to(DEV), plan, 0.1, 0.6)


def _run(**kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle)."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    set_seed(2024, True)
    tr = AVAILABLE_MODELS["CCFCRec"](_toy_cfg(data, **kw))
    tr.u0 = tr.model.user_embedding.detach().clone().numpy()
    tr.v0 = tr.model.item_embedding.detach().clone().numpy()
    tr.run()
    return tr


@pytest.fixture(scope="module")
def toy_run():
    return _run()


def test_run_matches_reference_g21(toy_run):
    """Structured as the G20 test.  Plain float32 torch on the CPU ends 3.2e-6 / 1.7e-7 of the tables' scale from G21 with
    losses 1.8e-7 apart (tests/test_ccfcrec.py); 8x those stay below CLCRec's bars, so the bars are CLCRec's: 2e-4 of the
    table scale, 1e-5 of every loss term."""
    fx, tr = load_golden("g21_ccfcrec.npz"), toy_run
    assert ccfcrec_restate.crc(tr.u0) == int(fx["U0_crc"]) and ccfcrec_restate.crc(tr.v0) == int(fx["V0_crc"])
    want = fx["losses"]
    assert tr.batch_losses.shape == want.shape
    rel = np.abs(tr.batch_losses - want) / np.abs(want)
    print(f"CCFCRec: worst relative loss difference to G21 {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    U, V = fx["U"], fx["V"]
    eu = np.abs(tr.user_emb.cpu().numpy() - U).max() / np.abs(U).max()
    ev = np.abs(tr.item_emb.cpu().numpy() - V).max() / np.abs(V).max()
    print(f"CCFCRec: final tables differ by {eu:.2e} / {ev:.2e} of their scale")
    assert eu < 2e-4 and ev < 2e-4
    same, det, total = _lists_vs_reference(tr, fx, U, V, min_frac=0.5)
    print(f"CCFCRec: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    ref = dict(overall=fx["test_overall"], cold=fx["test_cold"], warm=fx["test_warm"],
               best=[int(fx["best_epoch"]), json.loads(str(fx["best_metrics"]))])
    _metrics_vs_reference(tr, ref, same == total)


def test_second_run_is_bit_identical(toy_run):
    b = _run()
    assert np.array_equal(toy_run.batch_losses, b.batch_losses)
    assert torch.equal(toy_run.user_emb, b.user_emb) and torch.equal(toy_run.item_emb, b.item_emb)


def test_pretrained_tables_stay_frozen(tmp_path, monkeypatch):
    """--pretrain true after an MF run with --save_emb: the warm rows of both tables stay bit-equal to the loaded files,
    the cold item rows are replaced by generated ones."""
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "MF", "--make_synthetic", "toy"] + common) is None
    main(["--model", "MF", "--epochs", "1"] + common)
    loaded = {s: torch.load(tmp_path / "emb" / f"toy_cold_item_MF_{s}_emb.pt", map_location="cpu").detach()
              for s in ("user", "item")}
    main(["--model", "CCFCRec", "--pretrain", "true", "--epochs", "1", "--positive_number", "3", "--negative_number", "8",
          "--self_neg_number", "8"] + common)
    out = {s: torch.load(tmp_path / "emb" / f"toy_cold_item_CCFCRec_{s}_emb.pt", map_location="cpu")
           for s in ("user", "item")}
    _, data = builder()
    cold = torch.as_tensor(np.asarray(data.mapped_cold_item_idx), dtype=torch.long)
    warm = torch.ones(loaded["item"].shape[0], dtype=torch.bool)
    warm[cold] = False
    assert torch.equal(out["user"], loaded["user"]) and torch.equal(out["item"][warm], loaded["item"][warm])
    assert torch.isfinite(out["item"]).all() and not (out["item"][cold] == loaded["item"][cold]).all(1).any()


def test_cli_trains_end_to_end(tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", "item", "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "CCFCRec", "--make_synthetic", "toy"] + common) is None
    pay = main(["--model", "CCFCRec", "--positive_number", "3", "--negative_number", "8", "--self_neg_number", "8",
                "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "CCFCRec" / "history.txt").is_file()
    for side in ("user", "item"):
        t = torch.load(tmp_path / "emb" / f"toy_cold_item_CCFCRec_{side}_emb.pt", map_location="cpu")
        assert torch.is_tensor(t) and t.shape[1] == 64 and torch.isfinite(t).all()
