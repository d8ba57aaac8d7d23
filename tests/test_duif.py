"""CPU-only: DUIF's registry entry, refusals, initial tensors, the plan's grouping, the kernel's queries, and the
restatement of whole runs pinned to G28 (the reference's own DUIF.run() on the toy item-cold and user-cold splits), which
makes the restatement the oracle of the GPU tests.  The distances of plain float32 torch from the float64 formula and from
G28 -- the figures the GPU tests' bars are 8x of -- are measured, printed and checked here (within a factor of 2 of the
recorded ones, which stand beside the constants of tests/test_duif_gpu.py).

Measured:
    float32 formula against float64 at the GPU cases, both modes: loss terms 1.40e-7 of the total at worst, gradients and
        H 6.19e-7 of their maximum at worst, 1.60e-6 in the "chunks" case; at the edges at worst 1.62e-7 (loss terms) and
        1.49e-5 (gradients, pos == neg in every record; 1.06e-6 at scores beyond +-30, below 3e-7 at the other four);
    float64 run against G28 (item / user): terms 1.47e-7 / 1.45e-7 of the total; best and trained tensors at worst 5.25e-5
        / 7.24e-6 of their scale (the free table; W 2.72e-7 / 2.26e-7);
    float32 run (one thread) against G28: terms 8.45e-8 / 8.49e-8; tensors at worst 1.18e-7 / 6.13e-7; all 750 / 456
        lists identical to the reference's, 739 / 447 determined (at least 96 % in every setting).
On the MI355X the kernel and the runs measure what tests/test_duif_gpu.py's docstring records.
"""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import duif_restate as R
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference
from tests.test_duif_gpu import (CASES, EDGE_F32_WORST, F32_CHUNKS_GRAD_WORST, F32_GRAD_WORST,
                                 F32_LOSS_WORST, F32_RUN_LOSS, F32_RUN_TENSORS, IDS, MODE_IDS, MODES, REG, RUN_LOSS_BAR,
                                 RUN_TABLE_BAR)


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="DUIF", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def within_2x(measured, recorded):
    return recorded / 2 <= measured <= recorded * 2


def test_registry_resolves_without_changing_the_listings():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    from coldrec_amd.model.FusedLossTrainer import FusedLossTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert "DUIF" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["DUIF"]
    assert issubclass(cls, FusedLossTrainer) and AVAILABLE_MODELS.get("DUIF") is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert "DUIF" not in keys and "DUIF" not in names and "DUIF" in resolvable()
    assert cls.fused_eval is True and cls._eval_parts is BaseColdStartTrainer._eval_parts       # the one-table ranking
    assert cls.predict is FusedLossTrainer.predict and cls.batch_predict is FusedLossTrainer.batch_predict
    assert cls.LOSS_TERMS == ("bpr", "reg", "batch_loss") and cls.TABLES == ("user_emb", "item_emb")
    assert cls.SAVE_FILES is None and cls._optimizers is FusedLossTrainer._optimizers       # one Adam over model.parameters()


def test_cli_adds_no_flags():
    from coldrec_amd.main import parse_args
    from coldrec_amd.model import AVAILABLE_MODELS
    a, b = parse_args(["--model", "DUIF"]), parse_args(["--model", "MF"])
    assert set(vars(a)) == set(vars(b)) and (a.lr, a.reg) == (0.001, 0.0001) and a.model in AVAILABLE_MODELS


@pytest.mark.parametrize("cold", ["item", "user"])
def test_refusals(cold, monkeypatch):
    from coldrec_amd.model import AVAILABLE_MODELS
    data = R.toy_data(cold)
    new = lambda **kw: AVAILABLE_MODELS["DUIF"](_cfg(data, cold_object=cold, **kw))
    with pytest.raises(ValueError, match=r"DUIF: --emb_size 50 must be a multiple of 4 in \[4, 256\]"):
        new(emb_size=50)
    with pytest.raises(ValueError, match=r"DUIF: --emb_size 260 must be a multiple of 4"):
        new(emb_size=260)
    with pytest.raises(ValueError, match="--optimizer sgd is not built"):
        new(optimizer="sgd")
    with pytest.raises(ValueError, match="--lazy_adam on is not built"):
        new(lazy_adam="on")
    with pytest.raises(ValueError, match="--shard_graph is not built"):
        new(shard_graph=True)
    tr = new(optimizer="adam", lazy_adam="auto")
    m = tr.model
    assert set(m.state_dict()) == {"embedding_dict.user_emb", "embedding_dict.item_emb", f"{cold}_projector.weight"}
    assert m.content.shape == ((data.user_num if cold == "user" else data.item_num), 16)
    assert m.table.shape == ((data.item_num if cold == "user" else data.user_num), 64) and m.projector.weight.shape == (64, 16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "dp_from_env", lambda: object())  # a data-parallel launch is refused before anything runs
    tr.device = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="data-parallel"):
        tr.train()


@pytest.mark.parametrize("cold", ["item", "user"])
def test_encoder_draws_the_reference_initial_tensors_and_publishes_copies(cold):
    """Equal seeds give the bits of G28's three initial parameters -- in the encoder and in the restatement's initialiser."""
    from coldrec_amd.model.DUIF import DUIF_Encoder
    from coldrec_amd.util.utils import set_seed
    data = R.toy_data(cold)
    fx = load_golden(f"g28_duif_{cold}.npz")
    cold_user = cold == "user"
    set_seed(2024, False)
    m = DUIF_Encoder(_cfg(data, cold_object=cold).args, data, 64, torch.device("cpu"))
    set_seed(2024, False)
    again = R.init(data.user_num, data.item_num, 16, 64)
    mine = (m.embedding_dict["user_emb"], m.embedding_dict["item_emb"], m.projector.weight)
    for a, b, want in zip(mine, again, R.init_of(fx, cold_user)):
        assert np.array_equal(a.detach().numpy(), want) and np.array_equal(b.numpy(), want)
    assert [n for n, _ in m.named_parameters()] == __import__("json").loads(str(fx["param_names"]))
    with torch.no_grad():
        user, item = m()
    free, proj = (item, user) if cold_user else (user, item)
    assert free.data_ptr() != m.table.data_ptr() and torch.equal(free, m.table)          # a later step moves no snapshot
    assert torch.equal(proj, m.content @ m.projector.weight.T)
    assert user.shape == (data.user_num, 64) and item.shape == (data.item_num, 64)


def test_plan_groups_the_free_side_only():
    from coldrec_amd import ops
    users, pos, neg = torch.tensor([3, 1, 3, 3, 1]), torch.tensor([2, 2, 5, 2, 9]), torch.tensor([5, 2, 2, 7, 2])
    p = ops.duif_plan(users, pos, neg, False, chunk=2)
    assert p["batch"] == 5 and p["cold_user"] is False and p["user_range"] == (1, 3) and p["item_range"] == (2, 9)
    assert p["own_ids"].tolist() == [1, 3] and p["own_ptr"].tolist() == [0, 2, 5]
    assert p["own_occ"].tolist() == [1, 4, 0, 2, 3]                                     # stable: ascending inside an id
    assert p["own_chunk_ptr"].tolist() == [0, 1, 3] and p["own_chunk_own"].tolist() == [0, 1, 1]
    assert (p["n_own"], p["n_own_chunks"]) == (2, 3) and all(p[k].dtype == torch.int32 for k in ("users", "pos", "neg", "own_occ"))
    assert p["pos"].tolist() == pos.tolist() and p["neg"].tolist() == neg.tolist() and not any(k.startswith("item_") and k != "item_range" for k in p)
    q = ops.duif_plan(users, pos, neg, True, chunk=2)                                    # the 2 B items: pos, then neg
    assert q["own_ids"].tolist() == [2, 5, 7, 9] and q["own_ptr"].tolist() == [0, 6, 8, 9, 10]
    assert q["own_occ"].tolist() == [0, 1, 3, 6, 7, 9, 2, 5, 8, 4]
    assert q["own_chunk_ptr"].tolist() == [0, 3, 4, 5, 6] and q["own_chunk_own"].tolist() == [0, 0, 0, 1, 2, 3]
    big = ops.duif_plan(torch.zeros(600, dtype=torch.long), pos[:1].repeat(600), neg[:1].repeat(600), False)
    assert big["n_own_chunks"] == -(-600 // ops.duif_chunk_rows())                      # the library's chunk by default
    with pytest.raises(RuntimeError, match="duif_plan: user id outside"):
        ops.duif_plan(users, pos, neg, False, n_users=3)
    with pytest.raises(RuntimeError, match="duif_plan: item id outside"):
        ops.duif_plan(users, pos, neg, True, n_items=9)
    with pytest.raises(RuntimeError, match="duif_plan: item id outside"):
        ops.duif_plan(users, pos, neg, False, n_items=100, id_range=((1, 3), (2, 100)))
    with pytest.raises(RuntimeError, match=r"must be \(B,\)"):
        ops.duif_plan(users, pos[:4], neg, False)


def test_queries_without_gpu():
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    assert L.crh_duif_chunk_rows() == ops.duif_chunk_rows() >= 64 and ops.duif_part_chunk() >= 2
    for cu in (0, 1):
        assert ops.duif_workspace_bytes(4096, 64, 300, cu, 2000) > 0 and ops.duif_workspace_bytes(1, 4, 1, cu, 1) > 0
        assert ops.duif_workspace_bytes(7, 256, 4096, cu, 5) > 0
        assert ops.duif_workspace_bytes(512, 6, 16, cu, 100) == 0 and ops.duif_workspace_bytes(512, 260, 16, cu, 100) == 0
        assert ops.duif_workspace_bytes(512, 64, 0, cu, 100) == 0 and ops.duif_workspace_bytes(512, 64, 4097, cu, 100) == 0
        assert ops.duif_workspace_bytes(0, 64, 16, cu, 1) == 0 and ops.duif_workspace_bytes(1 << 31, 64, 16, cu, 1) == 0
        assert ops.duif_workspace_bytes(8, 64, 16, cu, (16 if cu else 8) + 1) == 0
        sizes = [ops.duif_workspace_bytes(B, 64, 16, cu, B) for B in (1, 2, 63, 64, 65, 512, 513, 4096)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]                          # monotone in B
    # the partials: a function of the shape, never fewer for more rows, and the three boundaries the GPU cases sit on
    assert ops.duif_parts(0, 64, 16) == 0 and ops.duif_parts(64, 6, 16) == 0 and ops.duif_parts(64, 64, 0) == 0
    counts = [ops.duif_parts(r, 64, 16) for r in range(1, 3000)]
    assert counts[0] == 1 and all(a <= b <= a + 1 for a, b in zip(counts, counts[1:])) and counts[-1] > ops.duif_part_chunk()
    assert ops.duif_parts((1 << 32) - 1, 256, 4096) >= 1
    for cu in MODES:
        got = [ops.duif_parts((1 if cu else 2) * R.parts_batch(w, 8, 5, cu), 8, 5) for w in ("1", "2", "chunk+1")]
        assert got == [1, 2, ops.duif_part_chunk() + 1]
    assert L.crh_duif_f32(None, 0, None, 0, 0, *([None] * 4), 0, 0, 0, 0, *([None] * 5), 0, 0, 0, 0, 0, 0.0, 0.0,
                          *([None] * 5), 0, None) == -1 and b"NULL" in L.crh_last_error()
    plan = ops.duif_plan(torch.tensor([0, 1, 0]), torch.tensor([2, 2, 3]), torch.tensor([4, 3, 2]), False, chunk=2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.duif(torch.zeros(2, 4), torch.zeros(5, 3), torch.zeros(4, 3), plan, 0.01)


# ---- the measurements behind the GPU tests' bars -----------------------------------------------------------------------

def _worst(rows, label):
    worst = [0.0, 0.0]
    for tag, cu, inp, reg in rows:
        rel, errs = R.distances(R.step(*inp, reg, cu, dtype=torch.float32), R.step(*inp, reg, cu))
        print(f"float32 formula {tag} {MODE_IDS(cu)}: loss {rel:.2e}, d T, d W, H " + " ".join(f"{e:.2e}" for e in errs))
        worst = [max(worst[0], rel), max(worst[1], max(errs))]
    print(f"float32 formula at the {label}: worst loss {worst[0]:.3e}, worst gradient {worst[1]:.3e}")
    return worst


def test_float32_formula_distance_at_the_gpu_cases():
    plain = _worst([(IDS(c), m, R.inputs(c, m), REG) for m in MODES for c in CASES if c[0] != "chunks"], "cases")
    chunks = _worst([(IDS(c), m, R.inputs(c, m), REG) for m in MODES for c in CASES if c[0] == "chunks"], "chunks case")
    assert within_2x(max(plain[0], chunks[0]), F32_LOSS_WORST) and within_2x(plain[1], F32_GRAD_WORST)
    assert within_2x(chunks[1], F32_CHUNKS_GRAD_WORST)


def test_float32_formula_distance_at_the_edges():
    """Each edge has its own pair of figures: the worse of the two modes."""
    from coldrec_amd import ops
    for k, tag in enumerate(e[0] for e in R.edge_cases(False)):
        worst = _worst([(tag, m, *R.edge_cases(m)[k][1:]) for m in MODES], "edge " + tag)
        for m in MODES:                                 # every edge is a batch the plan accepts for its tables
            T, C, _, users, pos, neg = R.edge_cases(m)[k][1]
            nu, ni = (C.shape[0], T.shape[0]) if m else (T.shape[0], C.shape[0])
            plan = ops.duif_plan(users, pos, neg, m, n_users=nu, n_items=ni)
            if tag == "first-and-last":
                assert plan["user_range"] == (0, nu - 1) and plan["item_range"] == (0, ni - 1)
        assert within_2x(worst[0], EDGE_F32_WORST[tag][0]) and within_2x(worst[1], EDGE_F32_WORST[tag][1]), tag


@pytest.mark.parametrize("cold", ["item", "user"])
def test_float64_restatement_reproduces_g28(cold):
    """The restatement in float64 against the reference's float32 run: terms, trained and best tensors -- within the
    project's run bars."""
    fx = load_golden(f"g28_duif_{cold}.npz")
    cold_user = cold == "user"
    r = R.restated_run(cold, torch.float64)
    for a, b in zip(r["init"], R.init_of(fx, cold_user)):
        assert np.array_equal(a, b)
    best = r["snaps"][int(fx["best_epoch"]) - 1]
    rel, e_best, e_trained = R.run_distances(fx, cold_user, r["terms"], best, r["trained"])
    print(f"float64 restatement {cold}: terms {rel:.2e}; best " + " ".join(f"{e:.2e}" for e in e_best) + "; trained " +
          " ".join(f"{e:.2e}" for e in e_trained))
    assert rel <= RUN_LOSS_BAR and max(e_best) <= RUN_TABLE_BAR and max(e_trained) <= RUN_TABLE_BAR
    assert r["terms"].shape == (int(fx["n_steps"]), 3) == (16, 3) and int(fx["epochs_ran"]) == 2
    assert int(fx["best_epoch"]) == 1 and not bool(fx["best_is_last"])
    assert np.allclose(fx["terms"][:, 2], fx["terms"][:, 0] + fx["terms"][:, 1], rtol=1e-6) and fx["terms"][:, 1].min() > 0


@pytest.mark.parametrize("cold", ["item", "user"])
def test_float32_restatement_distance_to_g28(cold):
    fx = load_golden(f"g28_duif_{cold}.npz")
    cold_user = cold == "user"
    r = R.restated_run(cold, torch.float32)
    best = r["snaps"][int(fx["best_epoch"]) - 1]
    rel, e_best, e_trained = R.run_distances(fx, cold_user, r["terms"], best, r["trained"])
    worst = max(e_best + e_trained)
    print(f"float32 restatement {cold}: terms {rel:.3e}; worst best / trained tensor {worst:.3e}")
    assert within_2x(rel, F32_RUN_LOSS[cold]) and within_2x(worst, F32_RUN_TENSORS[cold])
    # 8x the float32 distances stay below the project's run bars: the bars stand
    assert 8 * rel <= RUN_LOSS_BAR and 8 * worst <= RUN_TABLE_BAR
    # the condition of the lists' check: at least half of the users keep a determined ranking in every setting
    content = np.asarray(R.toy_data(cold).mapped_user_content if cold_user else R.toy_data(cold).mapped_item_content, np.float64)
    proj = content @ best[1].T
    ranked = (proj, best[0]) if cold_user else (best[0], proj)
    same, det, total = lists_vs_reference(R.ranked_of(fx, cold_user), ranked, None, min_frac=0.5)
    print(f"float32 restatement {cold}: {same} of {total} lists identical to the reference's ({det} determined)")
