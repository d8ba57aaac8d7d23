"""CPU-only: MTPR's registry entry, flags and refusals, the learner's initial tensors, the kernel's workspace query, the
plan's arrays, and the restatement of whole runs pinned to G25 (the reference's own MTPR.run() on the toy item-cold and
user-cold splits), which makes the restatement the oracle of the GPU tests.  The distances of plain float32 torch from
the float64 formula and from G25 -- the figures the GPU tests' bars are 8x of -- are measured, printed and checked here
(within a factor of 2 of the recorded ones, which stand beside the constants of tests/test_mtpr_gpu.py).

Measured:
    float32 formula against float64 at the GPU cases, both modes: loss terms 1.40e-7 of the total at worst, gradients
        1.42e-6 of their maximum at worst (B = 1, d = 4); at the edge cases 1.55e-7 and 4.19e-6 (scores beyond +-30);
    float32 torch.optim.Adagrad against the float64 formula: 5.14e-8 of the maximum of p and of the accumulator;
    float64 run against G25: terms 1.16e-7 (item) / 1.26e-7 (user) of the total; best tables 7.99e-7 / 8.78e-7 (item: users /
        items) and 1.39e-6 / 6.21e-6 (user); trained tensors at worst 5.00e-6 / 4.03e-5 of their scale;
    float32 run (one thread) against G25: terms 2.13e-7 / 1.48e-7; best tables 3.13e-6 / 1.45e-6 and 1.07e-6 / 2.42e-6;
        trained tensors at worst 1.60e-5 / 1.28e-5; all 750 / 456 lists identical to the reference's (712 / 434 determined).
On the MI355X the kernel measures what tests/test_mtpr_gpu.py's docstring records.
"""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import mtpr_restate as R
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference
from tests.test_mtpr_gpu import (CASES, EDGE_F32_GRAD_WORST, EDGE_F32_LOSS_WORST, F32_ADAGRAD_WORST, F32_GRAD_WORST,
                                 F32_LOSS_WORST, F32_RUN_BEST, F32_RUN_LOSS, F32_RUN_TRAINED, IDS, MODES, RUN_LOSS_BAR,
                                 RUN_TABLE_BAR, WD1, adagrad_distance, restated_run)

COLD = ["item", "user"]


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="MTPR", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, p_emb=[0.05, 0.0], p_ctx=[0.05, 0.01], p_proj=[0.05, 0.01])
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def within_2x(measured, recorded):
    return recorded / 2 <= measured <= recorded * 2


def test_registry_resolves_mtpr_without_changing_the_listings():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert "MTPR" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["MTPR"]
    assert issubclass(cls, BaseColdStartTrainer) and AVAILABLE_MODELS.get("MTPR") is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert "MTPR" not in keys and "MTPR" not in names and "MTPR" in resolvable()
    assert cls.fused_eval is True and cls._eval_parts is BaseColdStartTrainer._eval_parts       # the one-table ranking


def test_cli_carries_the_reference_defaults_and_both_pair_spellings():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "MTPR"])
    assert (a.p_emb, a.p_ctx, a.p_proj) == ([0.05, 0.0], [0.05, 0.01], [0.05, 0.01])
    b = parse_args(["--model", "MTPR", "--p_emb", "0.1,0", "--p_ctx", "[0.02, 0.5]", "--p_proj", "0.3, 1e-3",
                    "--cold_object", "user"])
    assert (b.p_emb, b.p_ctx, b.p_proj, b.cold_object) == ([0.1, 0.0], [0.02, 0.5], [0.3, 1e-3], "user")
    for bad in ("0.1", "0.1,0.2,0.3", "a,b"):
        with pytest.raises(SystemExit):
            parse_args(["--model", "MTPR", "--p_emb", bad])


@pytest.mark.parametrize("cold", COLD)
def test_refusals(cold, monkeypatch):
    from coldrec_amd.model import AVAILABLE_MODELS
    data = R.toy_data(cold)
    new = AVAILABLE_MODELS["MTPR"]
    with pytest.raises(ValueError, match="multiple of 4"):
        new(_cfg(data, cold_object=cold, emb_size=50))
    with pytest.raises(ValueError, match=r"multiple of 4 in \[4, 128\]"):
        new(_cfg(data, cold_object=cold, emb_size=132))
    with pytest.raises(ValueError, match="--optimizer sgd is not built"):
        new(_cfg(data, cold_object=cold, optimizer="sgd"))
    with pytest.raises(ValueError, match="--lazy_adam on is not built"):
        new(_cfg(data, cold_object=cold, lazy_adam="on"))
    with pytest.raises(ValueError, match="--shard_graph is not built"):
        new(_cfg(data, cold_object=cold, shard_graph=True))
    tr = new(_cfg(data, cold_object=cold, optimizer="adam", lazy_adam="auto"))              # both cold objects construct
    m = tr.model
    assert not m.P.weight.requires_grad and not m.Q.weight.requires_grad                    # stepped by ops.adagrad_rows
    assert [n for n, _ in m.named_parameters()] == ["W", "weu", "wei", "P.weight", "Q.weight"]
    assert m.content.shape == ((data.user_num if cold == "user" else data.item_num), 16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "dp_from_env", lambda: object())  # a data-parallel launch is refused before anything runs
    tr.device = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="data-parallel"):
        tr.train()


@pytest.mark.parametrize("cold", COLD)
def test_learner_draws_the_reference_initial_tensors(cold):
    """Equal seeds give the bits of G25's five initial tensors -- in the learner and in the restatement's initialiser."""
    from coldrec_amd.model.MTPR import MTPR_Learner
    from coldrec_amd.util.utils import set_seed
    data = R.toy_data(cold)
    fx = load_golden(f"g25_mtpr_{cold}.npz")
    set_seed(2024, False)
    m = MTPR_Learner(_cfg(data, cold_object=cold).args, data, 64, torch.device("cpu"))
    set_seed(2024, False)
    again = R.init(data.user_num, data.item_num, 16, 64, cold == "user")
    mine = (m.P.weight, m.Q.weight, m.W, m.weu, m.wei)
    for name, a, b in zip(("P", "Q", "W", "weu", "wei"), mine, again):
        assert np.array_equal(a.detach().numpy(), fx["init_" + name]), name
        assert np.array_equal(b.detach().numpy(), fx["init_" + name]), name
    assert m.P.weight.shape == (data.user_num, 64 if cold == "user" else 128)
    assert m.Q.weight.shape == (data.item_num, 128 if cold == "user" else 64)


def test_queries_without_gpu():
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    assert L.crh_mtpr_chunk_rows() == ops.mtpr_chunk_rows() >= 64
    for cu in (0, 1):
        assert L.crh_mtpr_workspace_bytes(4096, 64, cu, 3000, 2000) > 0 and L.crh_mtpr_workspace_bytes(1, 4, cu, 1, 1) > 0
        assert L.crh_mtpr_workspace_bytes(512, 6, cu, 100, 100) == 0 and L.crh_mtpr_workspace_bytes(512, 132, cu, 100, 100) == 0
        assert L.crh_mtpr_workspace_bytes(0, 64, cu, 1, 1) == 0                                                # B
        assert L.crh_mtpr_workspace_bytes(8, 64, cu, 17, 8) == 0 and L.crh_mtpr_workspace_bytes(8, 64, cu, 16, 9) == 0
        sizes = [ops.mtpr_workspace_bytes(B, 64, cu, min(2 * B, 500), min(B, 300)) for B in (1, 2, 63, 64, 65, 512, 513, 4096,
                                                                                             16384, 16385, 65536)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]                          # monotone in B
        # the trainer's one workspace (every id distinct) holds any step of its batch size or a shorter one
        assert ops.mtpr_workspace_bytes(512, 64, cu, 1024, 512) >= ops.mtpr_workspace_bytes(347, 64, cu, 500, 300)


def test_plan_arrays_against_a_numpy_grouping():
    from coldrec_amd import ops
    g = torch.Generator().manual_seed(11)
    chunk = 4
    users, pos, neg = (torch.randint(n, (57,), generator=g) for n in (5, 9, 9))
    plan = ops.mtpr_plan(users, pos, neg, chunk=chunk)
    assert plan["batch"] == 57 and plan["user_range"] == (int(users.min()), int(users.max()))
    assert plan["item_range"] == (int(min(pos.min(), neg.min())), int(max(pos.max(), neg.max())))
    assert all(plan[k].dtype == torch.int32 for k in ("users", "pos", "neg", "user_ids", "item_ids", "item_occ"))
    for side, ids in (("user", users.numpy()), ("item", np.concatenate([pos.numpy(), neg.numpy()]))):
        uniq = np.unique(ids)
        assert np.array_equal(plan[f"{side}_ids"].numpy(), uniq) and plan[f"n_{side}s"] == len(uniq)
        ptr, occ = plan[f"{side}_ptr"].numpy(), plan[f"{side}_occ"].numpy()
        cptr, cown = plan[f"{side}_chunk_ptr"].numpy(), plan[f"{side}_chunk_own"].numpy()
        want_own = []
        for s, v in enumerate(uniq):
            where = np.nonzero(ids == v)[0]
            assert np.array_equal(occ[ptr[s]:ptr[s + 1]], where)                      # ascending inside an owner
            n_chunks = (len(where) + chunk - 1) // chunk
            assert cptr[s + 1] - cptr[s] == n_chunks
            want_own += [s] * n_chunks
        assert np.array_equal(cown, want_own) and plan[f"n_{side}_chunks"] == len(want_own)
    rng = ((0, 4), (0, 8))
    assert ops.mtpr_plan(users, pos, neg, id_range=rng, chunk=chunk)["item_range"] == (0, 8)       # the host-known ranges
    with pytest.raises(RuntimeError, match="outside the user table"):
        ops.mtpr_plan(users, pos, neg, n_users=int(users.max()), chunk=chunk)
    with pytest.raises(RuntimeError, match=r"must be \(B,\)"):
        ops.mtpr_plan(users, pos[:-1], neg, chunk=chunk)


# ---- the measurements behind the GPU tests' bars -----------------------------------------------------------------------

def test_float32_formula_distance_at_the_gpu_cases():
    worst = [0.0, 0.0]
    for cu in MODES:
        for case in CASES:
            inp = R.inputs(case, cu)
            rel, errs = R.distances(R.step(*inp, WD1, cu, dtype=torch.float32), R.step(*inp, WD1, cu))
            print(f"float32 formula {IDS(case)} {'user' if cu else 'item'}: loss {rel:.2e}, gradients " +
                  " ".join(f"{e:.2e}" for e in errs))
            worst = [max(worst[0], rel), max(worst[1], max(errs))]
    print(f"float32 formula at the cases: worst loss {worst[0]:.3e}, worst gradient {worst[1]:.3e}")
    assert within_2x(worst[0], F32_LOSS_WORST) and within_2x(worst[1], F32_GRAD_WORST)


def test_float32_formula_distance_at_the_edges():
    worst = [0.0, 0.0]
    for cu in MODES:
        for tag, inp, wd1 in R.edge_cases(cu):
            rel, errs = R.distances(R.step(*inp, wd1, cu, dtype=torch.float32), R.step(*inp, wd1, cu))
            print(f"float32 formula {tag} {'user' if cu else 'item'}: loss {rel:.2e}, gradients " +
                  " ".join(f"{e:.2e}" for e in errs))
            worst = [max(worst[0], rel), max(worst[1], max(errs))]
    print(f"float32 formula at the edges: worst loss {worst[0]:.3e}, worst gradient {worst[1]:.3e}")
    assert within_2x(worst[0], EDGE_F32_LOSS_WORST) and within_2x(worst[1], EDGE_F32_GRAD_WORST)


def test_float32_torch_adagrad_distance():
    worst = 0.0
    for case in R.ADAGRAD_CASES:
        p, g, s, ids = R.adagrad_inputs(*case)
        want_p, want_s = R.adagrad(p.double(), g.double(), s.double(), ids, R.ADAGRAD_LR)
        ref = torch.nn.Parameter(p.clone())
        opt = torch.optim.Adagrad([ref], lr=R.ADAGRAD_LR)
        opt.state[ref]["sum"].copy_(s)
        dense = torch.zeros_like(g)
        dense[ids.long()] = g[ids.long()]
        ref.grad = dense
        opt.step()
        err = adagrad_distance(ref.detach(), opt.state[ref]["sum"], want_p, want_s)
        print(f"float32 torch.optim.Adagrad d{case[0]} {'first' if case[1] else 'later'}: {err:.2e}")
        worst = max(worst, err)
    print(f"float32 torch.optim.Adagrad: worst {worst:.3e}")
    assert within_2x(worst, F32_ADAGRAD_WORST)


@pytest.mark.parametrize("cold", COLD)
def test_float64_restatement_reproduces_g25(cold):
    """The restatement in float64 against the reference's float32 run: terms, trained tensors, best tables, within the
    project's run bars (what float32 rounding moves over 16 steps)."""
    fx = load_golden(f"g25_mtpr_{cold}.npz")
    r = restated_run(cold, torch.float64)
    for a, name in zip(r["init"], ("P", "Q", "W", "weu", "wei")):
        assert np.array_equal(a, fx["init_" + name])
    rel, e_best, e_trained = R.run_distances(fx, r["terms"], r["snaps"][int(fx["best_epoch"]) - 1], r["trained"])
    print(f"float64 restatement {cold}: terms {rel:.2e}; best tables {e_best[0]:.2e} / {e_best[1]:.2e}; trained " +
          " ".join(f"{e:.2e}" for e in e_trained))
    assert rel <= RUN_LOSS_BAR and max(e_best) <= RUN_TABLE_BAR and max(e_trained) <= RUN_TABLE_BAR
    assert r["terms"].shape == (int(fx["n_steps"]), 6) and int(fx["epochs_ran"]) == 2


@pytest.mark.parametrize("cold", COLD)
def test_float32_restatement_distance_to_g25(cold):
    fx = load_golden(f"g25_mtpr_{cold}.npz")
    r = restated_run(cold, torch.float32)
    best = r["snaps"][int(fx["best_epoch"]) - 1]
    rel, e_best, e_trained = R.run_distances(fx, r["terms"], best, r["trained"])
    print(f"float32 restatement {cold}: terms {rel:.3e}; best tables {e_best[0]:.3e} / {e_best[1]:.3e}; trained " +
          " ".join(f"{e:.3e}" for e in e_trained))
    assert within_2x(rel, F32_RUN_LOSS[cold]) and within_2x(max(e_trained), F32_RUN_TRAINED[cold])
    assert all(within_2x(e, w) for e, w in zip(e_best, F32_RUN_BEST[cold]))
    # 8x the float32 distances stay below the project's run bars: the bars stand
    assert 8 * rel <= RUN_LOSS_BAR and 8 * max(e_best + e_trained) <= RUN_TABLE_BAR
    for k, name in enumerate(("P", "Q")):          # rows no batch touched keep their initial bits under Adagrad
        rows = ~r["touched"][k]
        assert np.array_equal(r["trained"][k][rows].astype(np.float32), fx["init_" + name][rows])
    same, det, total = lists_vs_reference(fx, best, None, min_frac=0.5)
    print(f"float32 restatement {cold}: {same} of {total} lists identical to the reference's ({det} determined)")
