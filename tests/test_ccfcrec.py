"""CPU-only: CCFCRec's registry entry, flags and refusals, the kernel's cap and workspace queries, and the float64
restatement of a whole run pinned to G21 (the reference's own CCFCRec.run() on the toy item-cold split), which makes the
restatement the oracle of the GPU tests.  The distances of plain float32 torch from the float64 formula and from G21 --
the figures the GPU tests' bars are 8x of -- are measured, printed and checked here."""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import ccfcrec_restate
from tests.conftest import load_golden
from tests.test_ccfcrec_gpu import CASES, GRAD_BAR, IDS, LOSS_BAR, _inputs, distances
from tests.test_host_logic import builder


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="CCFCRec", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, positive_number=3, negative_number=8, self_neg_number=8, tau=0.1, lambda1=0.6,
             attr_present_dim=64, implicit_dim=64, cat_implicit_dim=64, pretrain=False, pretrain_update=False)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def test_registry_resolves_ccfcrec_without_changing_the_listings():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert "CCFCRec" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["CCFCRec"]
    assert issubclass(cls, BaseColdStartTrainer) and AVAILABLE_MODELS.get("CCFCRec") is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert "CCFCRec" not in keys and "CCFCRec" not in names
    assert "CCFCRec" in resolvable() and set(names) <= set(resolvable())


def test_cli_carries_the_reference_defaults():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "CCFCRec"])
    assert (a.positive_number, a.negative_number, a.self_neg_number) == (5, 40, 40)
    assert (a.tau, a.lambda1) == (0.1, 0.6)
    assert (a.attr_present_dim, a.implicit_dim, a.cat_implicit_dim) == (64, 64, 64)
    assert a.pretrain is False and a.pretrain_update is False
    b = parse_args(["--model", "CCFCRec", "--pretrain", "true", "--pretrain_update", "--negative_number", "8"])
    assert b.pretrain is True and b.pretrain_update is True and b.negative_number == 8
    with pytest.raises(ValueError, match="CCFCRec"):           # the error lists everything a --model flag can name
        parse_args(["--model", "NoSuchModel"])


def test_refusals(tmp_path, monkeypatch):
    from coldrec_amd import ops
    from coldrec_amd.model import AVAILABLE_MODELS
    _, data = builder()
    new = AVAILABLE_MODELS["CCFCRec"]
    with pytest.raises(Exception, match="Cold user is not supported in CCFCRec"):
        new(_cfg(data, cold_object="user"))
    with pytest.raises(ValueError, match="multiple of 4"):
        new(_cfg(data, implicit_dim=50))
    with pytest.raises(ValueError, match="multiple of 4"):
        new(_cfg(data, implicit_dim=260))
    cap = ops.ccfcrec_max_rows()
    with pytest.raises(ValueError, match="cap of %d" % cap):
        new(_cfg(data, positive_number=8, negative_number=cap // 8, self_neg_number=8))
    monkeypatch.chdir(tmp_path)
    with pytest.raises(FileNotFoundError, match=r"CCFCRec --pretrain requires ./emb/toy_cold_item_MF_user_emb.pt. Train "
                                                r"the backbone first"):
        new(_cfg(data, pretrain=True))
    tr = new(_cfg(data))
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "dp_from_env", lambda: object())  # a data-parallel launch is refused before anything runs
    tr.device = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="data-parallel"):
        tr.train()


def test_queries_without_gpu():
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    assert L.crh_ccfcrec_max_rows() >= 1024 and L.crh_ccfcrec_max_rows() >= ops.ccfcrec_rows(5, 40, 40) == 246
    assert L.crh_ccfcrec_chunk_rows() >= 64
    assert L.crh_ccfcrec_workspace_bytes(512, 3, 8, 8, 64, 300, 400) > 0
    assert L.crh_ccfcrec_workspace_bytes(512, 3, 8, 8, 6, 300, 400) == 0            # width
    assert L.crh_ccfcrec_workspace_bytes(512, 0, 8, 8, 64, 300, 400) == 0           # P
    assert L.crh_ccfcrec_workspace_bytes(512, 3, 8, 0, 64, 300, 400) == 0           # S
    assert L.crh_ccfcrec_workspace_bytes(512, 1, L.crh_ccfcrec_max_rows(), 1, 64, 300, 400) == 0      # R above the cap
    assert L.crh_ccfcrec_workspace_bytes(512, 3, 8, 8, 64, 300, 1025) == 0          # more distinct users than 2B


def test_learner_draws_the_reference_tables_and_encodes_like_the_restatement():
    """The package's learner and the restatement's: the same tables from the same seed, and the same encoder output."""
    from coldrec_amd.model.CCFCRec import CCFCRec_Learner
    from coldrec_amd.util.utils import set_seed
    _, data = builder()
    fx = load_golden("g21_ccfcrec.npz")
    set_seed(2024, False)
    m = CCFCRec_Learner(_cfg(data).args, data, 64, torch.device("cpu"))
    assert ccfcrec_restate.crc(m.user_embedding.detach().numpy()) == int(fx["U0_crc"])
    assert ccfcrec_restate.crc(m.item_embedding.detach().numpy()) == int(fx["V0_crc"])
    set_seed(2024, False)
    r = ccfcrec_restate.Learner(data, 64, 64, 64)
    idx = torch.arange(0, data.item_num, 3)
    with torch.no_grad():
        assert torch.equal(m(idx, idx), r.encoder(m.item_content[idx]))


@pytest.fixture(scope="module")
def restated():
    """The float64 and the float32 restatement of the G21 run, each on a fresh builder (the sampler shuffles in place)."""
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        _, data = builder()
        out[name] = ccfcrec_restate.run(data, dt)
        out[name]["cold_idx"] = np.asarray(data.mapped_cold_item_idx)
    return out


def _best_tables(fx, r):
    """The tables the trainer would report: the snapshot of the fixture's best epoch, cold rows generated."""
    U, V, cold = r["snaps"][int(fx["best_epoch"]) - 1]
    V = V.copy()
    V[r["cold_idx"]] = cold
    return U, V


def test_float64_restatement_of_a_run_matches_reference_g21(restated):
    fx, r = load_golden("g21_ccfcrec.npz"), restated["f64"]
    assert r["U0_crc"] == int(fx["U0_crc"]) and r["V0_crc"] == int(fx["V0_crc"])
    assert r["losses"].shape == fx["losses"].shape == (16, 5)
    rel = np.abs(r["losses"] - fx["losses"]) / np.abs(fx["losses"])
    print(f"float64 restatement: worst relative loss difference to G21 {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5
    U, V = _best_tables(fx, r)
    eu, ev = np.abs(U - fx["U"]).max() / np.abs(fx["U"]).max(), np.abs(V - fx["V"]).max() / np.abs(fx["V"]).max()
    print(f"float64 restatement: best-epoch tables differ from G21 by {eu:.2e} / {ev:.2e} of their scale")
    assert eu < 2e-4 and ev < 2e-4


def test_float32_restatement_ends_near_g21(restated):
    """How far plain float32 torch ends from the reference's own float32 run (other summation orders only).  Measured:
    losses 1.8e-7, tables 3.2e-6 / 1.7e-7 of their scale.  8x those lie below CLCRec's bars (1e-5 of a loss term, 2e-4 of
    the table scale), so the GPU run is held to CLCRec's bars; that the figures stay below an eighth of them is asserted."""
    fx, r = load_golden("g21_ccfcrec.npz"), restated["f32"]
    rel = np.abs(r["losses"] - fx["losses"]) / np.abs(fx["losses"])
    U, V = _best_tables(fx, r)
    eu, ev = np.abs(U - fx["U"]).max() / np.abs(fx["U"]).max(), np.abs(V - fx["V"]).max() / np.abs(fx["V"]).max()
    print(f"float32 restatement: losses differ from G21 by {rel.max():.2e}, best-epoch tables by {eu:.2e} / {ev:.2e} of "
          f"their scale")
    assert 8 * rel.max() <= 1e-5 and 8 * eu < 2e-4 and 8 * ev < 2e-4


def _lists_on_the_host(U_got, V_got, fx):
    """tests/test_e2e_gpu.py's _lists_vs_reference with the lists ranked here in float64: a user's ranking is determined
    when every adjacent gap of the reference's fp64 top-(k+1) exceeds twice (fp32 dot-product error bound + the score
    change the table difference can cause); those users' lists must be identical.  Returns (same, determined, users)."""
    U_ref, V_ref = fx["U"], fx["V"]
    d = U_ref.shape[1]
    eU, eV = float(np.abs(U_got - U_ref).max()), float(np.abs(V_got - V_ref).max())
    gam = d * 2.0 ** -24 / (1 - d * 2.0 ** -24)
    same = det = total = 0
    for t in ("all", "cold", "warm"):
        want_i, want_s, users = fx[f"{t}_idx"], fx[f"{t}_score"], fx[f"{t}_users_int"]
        k = want_i.shape[1]
        rp, rc = fx[f"{t}_rated_rowptr"], fx[f"{t}_rated_col"]

        def scores(U, V):
            S = U[users].astype(np.float64) @ V.T.astype(np.float64)
            for r in range(len(users)):
                S[r, rc[rp[r]:rp[r + 1]]] = -1e9
            if fx[f"{t}_cand"].size:
                S[:, fx[f"{t}_cand"]] = -1e9
            return S

        S = scores(U_ref, V_ref)
        top = -np.sort(-S, axis=1)[:, :k + 1]
        gaps = np.where(top[:, 1:] > -1e8, top[:, :-1] - top[:, 1:], np.inf)
        a_u = np.abs(U_ref[users]).astype(np.float64)
        err = gam * (a_u @ np.abs(V_ref).T.astype(np.float64)).max(axis=1)
        pert = eU * np.abs(V_ref).sum(1).max() + eV * a_u.sum(1) + d * eU * eV
        determined = gaps.min(axis=1) > 2.0 * (err + pert)
        got_i = np.argsort(-scores(U_got, V_got), axis=1, kind="stable")[:, :k]
        real = want_s > -1e8
        equal = np.array([np.array_equal(got_i[r][real[r]], want_i[r][real[r]]) for r in range(len(users))])
        assert equal[determined].all(), (t, np.nonzero(determined & ~equal)[0][:10])
        same, det, total = same + int(equal.sum()), det + int(determined.sum()), total + len(users)
    return same, det, total


def test_float32_restatement_keeps_the_reference_lists(restated):
    """The list condition of the GPU run (at least half of the lists with a determined ranking) holds for plain float32
    torch, so it can be relied on there."""
    fx, r = load_golden("g21_ccfcrec.npz"), restated["f32"]
    U, V = _best_tables(fx, r)
    same, det, total = _lists_on_the_host(U, V, fx)
    print(f"float32 restatement: {same} of {total} lists identical to G21's ({det} with a determined ranking)")
    assert det >= 0.5 * total


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_float32_formula_stays_within_the_kernel_bars(case):
    """The measurement behind LOSS_BAR / GRAD_BAR of tests/test_ccfcrec_gpu.py, repeated: float32 torch against float64
    torch at the GPU test's cases must itself lie within the bars (they are 8x its worst distance)."""
    inp = _inputs(case)
    want = ccfcrec_restate.step(*inp, case[7], case[8])
    rel, errs = distances(ccfcrec_restate.step(*inp, case[7], case[8], dtype=torch.float32), want)
    print(f"{IDS(case)}: float32 torch: loss rel {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
    assert rel <= LOSS_BAR and max(errs) <= GRAD_BAR


def test_float32_formula_at_the_edge_cases_sets_their_bars():
    """The measurement behind CCF_LOSS_BAR / CCF_GRAD_BAR of tests/test_loss_edges_gpu.py: float32 torch against float64
    torch at every new edge case, printed; the bars are 8x the worst of them or this file's own bars, whichever is larger,
    and the recorded worst figures must be the measured ones within a factor of 2 (another CPU's rounding moves them)."""
    from tests import test_loss_edges_gpu as edges
    worst = [0.0, 0.0]
    for tag, case, inp in edges.ccf_edge_cases():
        want = ccfcrec_restate.step(*inp, case[7], case[8])
        rel, errs = distances(ccfcrec_restate.step(*inp, case[7], case[8], dtype=torch.float32), want)
        print(f"{tag}: float32 torch: loss rel {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}")
        worst = [max(worst[0], rel), max(worst[1], max(errs))]
        assert rel <= edges.CCF_LOSS_BAR and max(errs) <= edges.CCF_GRAD_BAR
    print(f"worst over the edge cases: loss rel {worst[0]:.2e}, gradient err / max {worst[1]:.2e}")
    assert edges.CCF_F32_LOSS_WORST / 2 <= worst[0] <= 2 * edges.CCF_F32_LOSS_WORST
    assert edges.CCF_F32_GRAD_WORST / 2 <= worst[1] <= 2 * edges.CCF_F32_GRAD_WORST
    assert edges.CCF_LOSS_BAR == max(8 * edges.CCF_F32_LOSS_WORST, LOSS_BAR)
    assert edges.CCF_GRAD_BAR == max(8 * edges.CCF_F32_GRAD_WORST, GRAD_BAR)
