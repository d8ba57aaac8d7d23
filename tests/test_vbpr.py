"""CPU-only: VBPR's and AMR's registry entries, flags, refusals and file names, the learner's initial tensors, the kernel's
workspace query, and the restatement of whole runs pinned to G26 (the reference's own VBPR.run() on the toy item-cold and
user-cold splits and AMR.run() on the item-cold one), which makes the restatement -- AMR's in the running-sum form of
the noise -- the oracle of the GPU tests.  The distances of plain float32 torch from the float64 formula and from G26
-- the figures the GPU tests' bars are 8x of -- are measured, printed and checked here (within a factor of 2 of the
recorded ones, which stand beside the constants of tests/test_vbpr_gpu.py).

Measured:
    float32 formula against float64 at the GPU cases, all variants: loss terms 1.29e-7 of the total at worst, gradients
        3.29e-7 of their maximum at worst, 4.59e-6 in the "chunks" case; at the edge cases 9.52e-8 and 7.97e-7;
    float32 torch.optim.Adagrad against the float64 formula: 5.14e-8 of the maximum of p and of the accumulator;
    float64 run against G26 (VBPR item / VBPR user / AMR item): terms 1.42e-7 / 9.94e-8 / 9.06e-8 of the total; best and
        trained tensors at worst 1.56e-6 / 3.83e-6 / 3.48e-6 of their scale; AMR's noise norms 2.67e-7;
    float32 run (one thread) against G26: terms 1.41e-7 / 2.20e-7 / 1.57e-7; tensors at worst 1.48e-6 / 2.31e-6 / 3.82e-6;
        noise norms 1.20e-7; all 750 / 456 / 750 lists identical to the reference's (716 / 437 / 720 determined).
On the MI355X the kernel and the runs measure what tests/test_vbpr_gpu.py's docstring records.
"""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import vbpr_restate as R
from tests.conftest import load_golden
from tests.mtpr_restate import ADAGRAD_CASES, ADAGRAD_LR, adagrad_inputs
from tests.test_gar_gpu import lists_vs_reference
from tests.test_mtpr_gpu import F32_ADAGRAD_WORST, adagrad_distance
from tests.test_vbpr_gpu import (CASES, EDGE_F32_GRAD_WORST, EDGE_F32_LOSS_WORST, F32_CHUNKS_GRAD_WORST, F32_GRAD_WORST,
                                 F32_LOSS_WORST, F32_RUN_LOSS, F32_RUN_NOISE, F32_RUN_TENSORS, IDS, LMD, RUN_IDS, RUN_LOSS_BAR, RUN_TABLE_BAR,
                                 RUNS, VARIANT_IDS, VARIANTS, WD1, content_of, restated_run, write_loaded)


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="VBPR", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, p_emb=list(R.P_EMB), p_ctx=list(R.P_CTX), eps=R.EPS, lmd=R.LMD)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def within_2x(measured, recorded):
    return recorded / 2 <= measured <= recorded * 2


@pytest.mark.parametrize("name", ["VBPR", "AMR"])
def test_registry_resolves_without_changing_the_listings(name):
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    from coldrec_amd.model.FusedLossTrainer import FusedLossTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert name in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS[name]
    assert issubclass(cls, FusedLossTrainer) and AVAILABLE_MODELS.get(name) is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert name not in keys and name not in names and name in resolvable()
    assert cls.fused_eval is True and cls._eval_parts is BaseColdStartTrainer._eval_parts       # the one-table ranking
    assert cls.predict is FusedLossTrainer.predict and cls.batch_predict is FusedLossTrainer.batch_predict
    assert cls.LOSS_TERMS == (("bpr", "regs", "batch_loss") if name == "VBPR" else ("bpr", "adv", "regs", "batch_loss"))
    assert cls.TABLES == ("user_emb_main", "item_emb_main", "user_emb_aux", "item_emb_aux", "w_value", "user_emb", "item_emb")
    assert tuple(cls.SAVE_FILES.values()) == R.FILES


def test_other_trainers_keep_their_file_names():
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.model.FusedLossTrainer import FusedLossTrainer
    assert FusedLossTrainer.SAVE_FILES is None
    for name in ("CLCRec", "CCFCRec", "ALDI", "GAR", "MTPR"):
        assert AVAILABLE_MODELS[name].SAVE_FILES is None


def test_cli_carries_the_reference_defaults():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "VBPR"])
    assert (a.p_emb, a.p_ctx) == ([0.05, 0.0], [0.05, 0.01]) and not hasattr(a, "eps")
    b = parse_args(["--model", "AMR"])
    assert (b.p_emb, b.p_ctx, b.eps, b.lmd) == ([0.05, 0.0], [0.05, 0.01], 0.1, 1)
    c = parse_args(["--model", "AMR", "--p_emb", "0.1,0.02", "--p_ctx", "[0.02, 0.5]", "--eps", "0.3", "--lmd", "2"])
    assert (c.p_emb, c.p_ctx, c.eps, c.lmd) == ([0.1, 0.02], [0.02, 0.5], 0.3, 2)
    with pytest.raises(SystemExit):
        parse_args(["--model", "VBPR", "--p_emb", "0.1"])


@pytest.fixture
def loaded_dir(tmp_path, monkeypatch):
    """A working directory whose ./emb holds what VBPR (both cold objects) and AMR load, from G26."""
    for which, cold in RUNS:
        write_loaded(load_golden(f"g26_{which}_{cold}.npz"), tmp_path, which, cold, R.toy_data(cold))
    monkeypatch.chdir(tmp_path)
    return tmp_path


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_refusals(run, loaded_dir, monkeypatch):
    from coldrec_amd.model import AVAILABLE_MODELS
    which, cold = run
    data = R.toy_data(cold)
    name = which.upper()
    new = lambda **kw: AVAILABLE_MODELS[name](_cfg(data, model=name, cold_object=cold, **kw))
    with pytest.raises(ValueError, match="multiple of 4"):
        new(emb_size=50)
    with pytest.raises(ValueError, match=r"multiple of 4 in \[4, 128\]"):
        new(emb_size=132)
    with pytest.raises(ValueError, match="--optimizer sgd is not built"):
        new(optimizer="sgd")
    with pytest.raises(ValueError, match="--lazy_adam on is not built"):
        new(lazy_adam="on")
    with pytest.raises(ValueError, match="--shard_graph is not built"):
        new(shard_graph=True)
    with pytest.raises(ValueError, match="do not fit this dataset" if which == "vbpr" else "need"):
        new(emb_size=32)                                                                    # the saved files are 64 wide
    tr = new(optimizer="adam", lazy_adam="auto")
    m = tr.model
    assert not any(t.weight.requires_grad for t in (m.P, m.Q, m.PQ2)) and m.W.requires_grad   # stepped by ops.adagrad_rows
    assert m.content.shape == ((data.user_num if cold == "user" else data.item_num), 16)
    assert m.PQ2.weight.shape == ((data.item_num if cold == "user" else data.user_num), 64)
    if which == "amr":
        assert m.noise.shape == m.content.shape and not m.noise.any() and (m.eps, m.lmd) == (0.1, 1.0)
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "dp_from_env", lambda: object())  # a data-parallel launch is refused before anything runs
    tr.device = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="data-parallel"):
        tr.train()


def test_amr_refuses_cold_users_and_names_the_missing_vbpr_file(loaded_dir):
    from coldrec_amd.model import AVAILABLE_MODELS
    with pytest.raises(ValueError, match=r"--cold_object user is not built.*model/AMR\.py:148"):
        AVAILABLE_MODELS["AMR"](_cfg(R.toy_data("user"), model="AMR", cold_object="user"))
    data = R.toy_data("item")
    (loaded_dir / "emb" / "toy_cold_item_VBPR_W.pt").unlink()
    with pytest.raises(FileNotFoundError, match=r"toy_cold_item_VBPR_W\.pt.*--model VBPR --dataset toy --cold_object item"):
        AVAILABLE_MODELS["AMR"](_cfg(data, model="AMR"))
    (loaded_dir / "emb" / "toy_cold_item_MF_user_emb.pt").unlink()
    with pytest.raises(FileNotFoundError, match=r"MF_user_emb\.pt.*--model MF"):
        AVAILABLE_MODELS["VBPR"](_cfg(data))


@pytest.mark.parametrize("cold", ["item", "user"])
def test_learner_draws_the_reference_initial_tensors(cold, loaded_dir):
    """Equal seeds give the bits of G26's initial PQ2 and W -- in the learner and in the restatement's initialiser."""
    from coldrec_amd.model.VBPR import VBPR_Learner
    from coldrec_amd.util.utils import set_seed
    data = R.toy_data(cold)
    fx = load_golden(f"g26_vbpr_{cold}.npz")
    set_seed(2024, False)
    m = VBPR_Learner(_cfg(data, cold_object=cold).args, data, 64, torch.device("cpu"))
    set_seed(2024, False)
    again = R.init(data.user_num, data.item_num, 16, 64, cold == "user")
    assert np.array_equal(m.P.weight.numpy(), fx["loaded_U"]) and np.array_equal(m.Q.weight.numpy(), fx["loaded_V"])
    for name, a, b in zip(("PQ2", "W"), (m.PQ2.weight, m.W), again):
        assert np.array_equal(a.detach().numpy(), fx["init_" + name]), name
        assert np.array_equal(b.detach().numpy(), fx["init_" + name]), name


def test_amr_learner_starts_from_vbprs_files(loaded_dir):
    from coldrec_amd.model.AMR import AMR_Learner
    data = R.toy_data("item")
    fx = load_golden("g26_amr_item.npz")
    m = AMR_Learner(_cfg(data, model="AMR").args, data, 64, torch.device("cpu"))
    for t, k in zip((m.P.weight, m.Q.weight, m.PQ2.weight, m.W), ("user_emb_main", "item_emb_main", "user_emb_aux", "w_value")):
        assert np.array_equal(t.detach().numpy(), fx["loaded_" + k])


def test_published_tensors_and_file_names(loaded_dir):
    """forward() gives copies of the five tensors and the ranked pair whose product is score1 + score2."""
    from coldrec_amd.model.FusedLossTrainer import VBPR_FILES
    from coldrec_amd.model.VBPR import VBPR_Learner
    assert tuple(VBPR_FILES.values()) == R.FILES
    for cold in ("item", "user"):
        data = R.toy_data(cold)
        m = VBPR_Learner(_cfg(data, cold_object=cold).args, data, 64, torch.device("cpu"))
        with torch.no_grad():
            um, im, ua, ia, w, user, item = m()
        assert um.data_ptr() != m.P.weight.data_ptr() and w.data_ptr() != m.W.data_ptr()       # a later step moves no snapshot
        assert user.shape == (data.user_num, 128) and item.shape == (data.item_num, 128)
        want = um.double() @ im.double().T + ua.double() @ ia.double().T
        assert torch.allclose(user.double() @ item.double().T, want, rtol=0, atol=1e-12)
        aux = torch.as_tensor(content_of(data, cold)) @ w
        assert torch.equal(ua if cold == "user" else ia, aux)


def test_queries_without_gpu():
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    assert L.crh_vbpr_chunk_rows() == ops.vbpr_chunk_rows() >= 64
    for cu in (0, 1):
        assert L.crh_vbpr_workspace_bytes(4096, 64, cu, 3000, 2000) > 0 and L.crh_vbpr_workspace_bytes(1, 4, cu, 1, 1) > 0
        assert L.crh_vbpr_workspace_bytes(7, 256, cu, 10, 5) > 0
        assert L.crh_vbpr_workspace_bytes(512, 6, cu, 100, 100) == 0 and L.crh_vbpr_workspace_bytes(512, 260, cu, 100, 100) == 0
        assert L.crh_vbpr_workspace_bytes(0, 64, cu, 1, 1) == 0 and L.crh_vbpr_workspace_bytes(1 << 30, 64, cu, 1, 1) == 0
        assert L.crh_vbpr_workspace_bytes(8, 64, cu, 17, 8) == 0 and L.crh_vbpr_workspace_bytes(8, 64, cu, 16, 9) == 0
        sizes = [ops.vbpr_workspace_bytes(B, 64, cu, min(2 * B, 500), min(B, 300)) for B in (1, 2, 63, 64, 65, 512, 513, 4096)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]                          # monotone in B
        # the trainer's one workspace (every id distinct) holds any step of its batch size or a shorter one
        assert ops.vbpr_workspace_bytes(512, 64, cu, 1024, 512) >= ops.vbpr_workspace_bytes(347, 64, cu, 500, 300)
    assert L.crh_vbpr_f32(None, 0, None, 0, *([None] * 6), 0, 0, 0, 0, *([None] * 5), 0, 0, *([None] * 5), 0, 0, 0, 0, 0, 0.0,
                          0.0, 0.0, *([None] * 8), 0, None) == -1 and b"NULL" in L.crh_last_error()
    plan = ops.vbpr_plan(torch.tensor([0, 1, 0]), torch.tensor([2, 2, 3]), torch.tensor([4, 3, 2]), chunk=2)
    assert plan["item_ids"].tolist() == [2, 3, 4] and plan["n_item_chunks"] == 4 and plan["user_ids"].tolist() == [0, 1]
    with pytest.raises(RuntimeError, match="vbpr_plan: user id outside"):
        ops.vbpr_plan(torch.tensor([0, 5]), torch.tensor([1, 1]), torch.tensor([2, 2]), n_users=5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.vbpr(torch.zeros(2, 4), torch.zeros(5, 4), torch.zeros(2, 4), torch.zeros(6, 4), plan, 0.01)


# ---- the measurements behind the GPU tests' bars -----------------------------------------------------------------------

def _worst(rows, label):
    worst = [0.0, 0.0]
    for tag, variant, inp, wd1, lmd in rows:
        cu = variant[0]
        rel, errs = R.distances(R.step(*inp, wd1, cu, lmd, dtype=torch.float32), R.step(*inp, wd1, cu, lmd))
        print(f"float32 formula {tag} {VARIANT_IDS(variant)}: loss {rel:.2e}, gradients " + " ".join(f"{e:.2e}" for e in errs))
        worst = [max(worst[0], rel), max(worst[1], max(errs))]
    print(f"float32 formula at the {label}: worst loss {worst[0]:.3e}, worst gradient {worst[1]:.3e}")
    return worst


def test_float32_formula_distance_at_the_gpu_cases():
    plain = _worst([(IDS(c), v, R.inputs(c, *v), WD1, LMD) for v in VARIANTS for c in CASES if c[0] != "chunks"], "cases")
    chunks = _worst([(IDS(c), v, R.inputs(c, *v), WD1, LMD) for v in VARIANTS for c in CASES if c[0] == "chunks"], "chunks case")
    assert within_2x(max(plain[0], chunks[0]), F32_LOSS_WORST) and within_2x(plain[1], F32_GRAD_WORST)
    assert within_2x(chunks[1], F32_CHUNKS_GRAD_WORST)


def test_float32_formula_distance_at_the_edges():
    worst = _worst([(e[0], v, e[1], e[2], e[3]) for v in VARIANTS for e in R.edge_cases(*v)], "edges")
    assert within_2x(worst[0], EDGE_F32_LOSS_WORST) and within_2x(worst[1], EDGE_F32_GRAD_WORST)


def test_float32_torch_adagrad_distance():
    """The formula ``ops.adagrad_rows`` restates (tests/mtpr_restate.py) against torch.optim.Adagrad in float32."""
    worst = 0.0
    for case in ADAGRAD_CASES:
        p, g, s, ids = adagrad_inputs(*case)
        want_p, want_s = R.adagrad(p.double(), g.double(), s.double(), ids, ADAGRAD_LR)
        ref = torch.nn.Parameter(p.clone())
        opt = torch.optim.Adagrad([ref], lr=ADAGRAD_LR)
        opt.state[ref]["sum"].copy_(s)
        dense = torch.zeros_like(g)
        dense[ids.long()] = g[ids.long()]
        ref.grad = dense
        opt.step()
        worst = max(worst, adagrad_distance(ref.detach(), opt.state[ref]["sum"], want_p, want_s))
    print(f"float32 torch.optim.Adagrad: worst {worst:.3e}")
    assert within_2x(worst, F32_ADAGRAD_WORST)


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_float64_restatement_reproduces_g26(run):
    """The restatement in float64 against the reference's float32 run: terms, trained and best tensors and, for AMR in its
    running-sum form, the noise's norm after every backward -- within the project's run bars."""
    which, cold = run
    fx = load_golden(f"g26_{which}_{cold}.npz")
    r = restated_run(which, cold, torch.float64)
    amr = which == "amr"
    if not amr:
        assert np.array_equal(r["init"][2], fx["init_PQ2"]) and np.array_equal(r["init"][3], fx["init_W"])
    rel, e_best, e_trained, e_noise = R.run_distances(fx, r["terms"], r["snaps"][int(fx["best_epoch"]) - 1], r["trained"],
                                                      r["noise_norms"] if amr else None)
    print(f"float64 restatement {which} {cold}: terms {rel:.2e}; best " + " ".join(f"{e:.2e}" for e in e_best) + "; trained " +
          " ".join(f"{e:.2e}" for e in e_trained) + (f"; noise norms {e_noise:.2e}" if amr else ""))
    assert rel <= RUN_LOSS_BAR and max(e_best) <= RUN_TABLE_BAR and max(e_trained) <= RUN_TABLE_BAR
    assert r["terms"].shape == (int(fx["n_steps"]), 4 if amr else 3) and int(fx["epochs_ran"]) == 2
    if amr:
        assert e_noise <= RUN_LOSS_BAR and len(r["noise_norms"]) == 2 * int(fx["n_steps"])
        assert float(fx["terms"][:, 1].min()) > 0


@pytest.mark.parametrize("run", RUNS, ids=RUN_IDS)
def test_float32_restatement_distance_to_g26(run):
    which, cold = run
    key = RUN_IDS(run)
    fx = load_golden(f"g26_{which}_{cold}.npz")
    r = restated_run(which, cold, torch.float32)
    amr = which == "amr"
    best = r["snaps"][int(fx["best_epoch"]) - 1]
    rel, e_best, e_trained, e_noise = R.run_distances(fx, r["terms"], best, r["trained"], r["noise_norms"] if amr else None)
    worst = max(e_best + e_trained)
    print(f"float32 restatement {key}: terms {rel:.3e}; worst best / trained tensor {worst:.3e}" +
          (f"; noise norms {e_noise:.3e}" if amr else ""))
    assert within_2x(rel, F32_RUN_LOSS[key]) and within_2x(worst, F32_RUN_TENSORS[key])
    # 8x the float32 distances stay below the project's run bars: the bars stand
    assert 8 * rel <= RUN_LOSS_BAR and 8 * worst <= RUN_TABLE_BAR
    if amr:
        assert within_2x(e_noise, F32_RUN_NOISE) and 8 * e_noise <= RUN_LOSS_BAR
    cold_user = cold == "user"
    for k, rows in ((0, ~r["touched"][0]), (1, ~r["touched"][1]), (2, ~r["touched"][1 if cold_user else 0])):
        assert np.array_equal(r["trained"][k][rows].astype(np.float32), r["init"][k][rows])      # untouched under Adagrad
    content = content_of(R.toy_data(cold), cold)
    ranked = R.published(*(torch.from_numpy(t) for t in best), torch.from_numpy(content.astype(np.float64)), cold_user)
    same, det, total = lists_vs_reference(R.ranked_of(fx, content, cold_user), [t.numpy() for t in ranked], None, min_frac=0.5)
    print(f"float32 restatement {key}: {same} of {total} lists identical to the reference's ({det} determined)")
