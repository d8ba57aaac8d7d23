"""CPU-only: GAR's registry entry, flags and refusals, the kernel's workspace query, the plan's arrays, and the restatement
of whole runs pinned to G24 (the reference's own MF.run() + GAR.run() on the toy item-cold and user-cold splits), which
makes the restatement the oracle of the GPU tests.  The distances of plain float32 torch from the float64 formula and
from G24 -- the figures the GPU tests' bars are 8x of -- are measured, printed and checked here.

Measured:
    float32 formula against float64 at the GPU cases, both modes: loss terms 1.91e-7 of the total at worst, gradients
        7.78e-7 of their maximum at worst (the chunk case); at the edge cases 1.33e-7 and 2.51e-6 (scores beyond +-30);
    float64 run against G24: loss terms 1.65e-7 (item) / 1.24e-7 (user) of the total; tables 1.15e-5 / 3.21e-6 (item: users /
        items) and 5.43e-7 / 1.39e-6 (user) of their scale;
    float32 run against G24: loss terms 8.81e-8 / 8.91e-8; tables 1.51e-5 / 1.46e-6 and 2.35e-7 / 2.34e-7;
    the float32 restatement's lists: see test_float32_restatement_keeps_the_reference_lists_and_metrics;
    float32 formula against float64 at the count cases of tests/test_owner_pass_gpu.py (tests/owner_cases.py: reg = B =
        2746, thirteen widths, both modes): loss terms 1.05e-5 of the total at worst, gradients 2.15e-5 of their maximum
        (both at d = 256: float32 torch's norm of a 2746 x 256 block); 1.5e-7 .. 2.2e-7 and 9e-7 at d = 4;
    the mutated float64 restatements at those cases, least distance over the widths and modes, as gradient error over
        the maximum: counts swapped 0.80, every occurrence counted as a positive 0.24, one occurrence of a three-chunk
        owner miscounted 1.57e-3, R's part dropped on the user side 0.97 -- against 4 bars = 6.9e-4.
On the MI355X the kernel measures what tests/test_gar_gpu.py's docstring records.
"""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import gar_restate
from tests import owner_cases as oc
from tests import test_owner_pass_gpu as op
from tests.conftest import load_golden
from tests.test_gar_gpu import (CASES, COEF, EDGE_F32_GRAD_WORST, EDGE_F32_LOSS_WORST, EDGE_GRAD_BAR, EDGE_LOSS_BAR,
                                F32_GRAD_WORST, F32_LOSS_WORST, F32_RUN_LOSS, F32_RUN_TABLES, GRAD_BAR, IDS, LOSS_BAR,
                                MODES, RUN_LOSS_BAR, RUN_TABLE_BAR, _inputs, distances, edge_cases, lists_vs_reference,
                                metrics_vs_reference, run_distances, write_loaded)

COLD = ["item", "user"]


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="GAR", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, alpha=0.05, beta=0.1)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def test_registry_resolves_gar_without_changing_the_listings():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert "GAR" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["GAR"]
    assert issubclass(cls, BaseColdStartTrainer) and AVAILABLE_MODELS.get("GAR") is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert "GAR" not in keys and "GAR" not in names and "GAR" in resolvable()
    assert cls.fused_eval is True and cls._eval_parts is BaseColdStartTrainer._eval_parts       # the one-table ranking


def test_cli_carries_the_reference_defaults():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "GAR"])
    assert (a.alpha, a.beta, a.backbone) == (0.05, 0.1, "MF")
    b = parse_args(["--model", "GAR", "--alpha", "0.3", "--beta", "0.6", "--cold_object", "user"])
    assert (b.alpha, b.beta, b.cold_object) == (0.3, 0.6, "user")


@pytest.mark.parametrize("cold", COLD)
def test_refusals(cold, tmp_path, monkeypatch):
    from coldrec_amd.model import AVAILABLE_MODELS
    data = gar_restate.toy_data(cold)
    new = AVAILABLE_MODELS["GAR"]
    monkeypatch.chdir(tmp_path)
    with pytest.raises(ValueError, match="multiple of 4"):
        new(_cfg(data, cold_object=cold, emb_size=50))
    with pytest.raises(ValueError, match="multiple of 4"):
        new(_cfg(data, cold_object=cold, emb_size=260))
    with pytest.raises(FileNotFoundError, match=rf"GAR requires ./emb/toy_cold_{cold}_MF_user_emb.pt. Train the backbone "
                                                rf"first \(e.g. main.py --model MF --dataset toy --cold_object {cold} "
                                                rf"--save_emb true\)"):
        new(_cfg(data, cold_object=cold))
    fx = load_golden(f"g24_gar_{cold}.npz")
    write_loaded(fx, tmp_path, cold)
    with pytest.raises(ValueError, match="do not fit this dataset"):
        new(_cfg(data, cold_object=cold, emb_size=32))
    tr = new(_cfg(data, cold_object=cold))                                                  # both cold objects construct
    m = tr.model
    assert m.user_emb.requires_grad and m.item_emb.requires_grad                           # the tables are trained
    assert isinstance(m.user_emb, torch.nn.Parameter) and np.array_equal(m.user_emb.detach().numpy(), fx["loaded_U"])
    assert [n for n, _ in m.named_parameters()] == ["user_emb", "item_emb", "generator.0.weight", "generator.0.bias",
                                                     "generator.2.weight", "generator.2.bias"]
    assert m.content.shape == ((data.user_num if cold == "user" else data.item_num), 16)
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "dp_from_env", lambda: object())  # a data-parallel launch is refused before anything runs
    tr.device = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="data-parallel"):
        tr.train()


@pytest.mark.parametrize("cold", COLD)
def test_learner_draws_the_restatement_generator(cold, tmp_path, monkeypatch):
    """The package's learner and the restatement's: the same generator from the same seed, drawn before the tables load."""
    from coldrec_amd.model.GAR import GAR_Learner
    from coldrec_amd.util.utils import set_seed
    data = gar_restate.toy_data(cold)
    write_loaded(load_golden(f"g24_gar_{cold}.npz"), tmp_path, cold)
    monkeypatch.chdir(tmp_path)
    set_seed(2024, False)
    m = GAR_Learner(_cfg(data, cold_object=cold).args, data, 64, torch.device("cpu"))
    set_seed(2024, False)
    g = gar_restate.generator(16, 64)
    for (na, pa), (nb, pb) in zip(m.generator.named_parameters(), g.named_parameters()):
        assert na == nb and torch.equal(pa, pb)


def test_queries_without_gpu():
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    assert L.crh_gar_chunk_rows() == ops.gar_chunk_rows() >= 64
    assert L.crh_gar_workspace_bytes(4096, 64, 3000, 2000) > 0 and L.crh_gar_workspace_bytes(1, 4, 1, 1) > 0
    assert L.crh_gar_workspace_bytes(512, 6, 100, 100) == 0 and L.crh_gar_workspace_bytes(512, 260, 100, 100) == 0   # width
    assert L.crh_gar_workspace_bytes(0, 64, 1, 1) == 0                                                               # B
    assert L.crh_gar_workspace_bytes(8, 64, 17, 8) == 0 and L.crh_gar_workspace_bytes(8, 64, 16, 9) == 0        # owners > occurrences
    sizes = [ops.gar_workspace_bytes(B, 64, min(2 * B, 500), min(B, 300)) for B in (1, 2, 63, 64, 65, 512, 513, 4096, 65536)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]                                  # monotone in B


@pytest.mark.parametrize("which", ["gar", "mtpr"])
@pytest.mark.parametrize("case", [(37, 20, 11, 30), ("chunks", 132, 3, 5), (2048, 64, 300, 500)], ids=IDS)
def test_plan_arrays_against_a_numpy_grouping(case, which):
    """One body builds both plans: each against the NumPy grouping at its own library chunk size, and the two against
    each other, same keys and equal tensors, at that chunk size and at a small one."""
    from coldrec_amd import ops
    _, _, users, pos, neg, _ = _inputs(case)
    make_plan = getattr(ops, which + "_plan")
    chunk = getattr(ops, which + "_chunk_rows")()
    plan = make_plan(users, pos, neg, n_users=case[2], n_items=case[3])
    for c in (chunk, 7):
        a, b = ops.gar_plan(users, pos, neg, chunk=c), ops.mtpr_plan(users, pos, neg, chunk=c)
        assert list(a) == list(b) and all(torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k] for k in a)
    B = users.shape[0]
    assert plan["batch"] == B and all(v.dtype == torch.int32 for v in plan.values() if torch.is_tensor(v))
    for side, ids in (("user", users.numpy()), ("item", np.concatenate([pos.numpy(), neg.numpy()]))):
        uniq = np.unique(ids)
        order = np.argsort(ids, kind="stable")
        cnt = np.array([(ids == x).sum() for x in uniq])
        ptr = np.concatenate([[0], np.cumsum(cnt)])
        nch = (cnt + chunk - 1) // chunk
        assert np.array_equal(plan[f"{side}_ids"].numpy(), uniq) and plan[f"n_{side}s"] == len(uniq)
        assert np.array_equal(plan[f"{side}_occ"].numpy(), order) and np.array_equal(plan[f"{side}_ptr"].numpy(), ptr)
        assert np.array_equal(plan[f"{side}_chunk_ptr"].numpy(), np.concatenate([[0], np.cumsum(nch)]))
        assert np.array_equal(plan[f"{side}_chunk_own"].numpy(), np.repeat(np.arange(len(uniq)), nch))
        assert plan[f"n_{side}_chunks"] == nch.sum() <= len(uniq) + len(ids) // chunk
        assert plan[f"{side}_range"] == (ids.min(), ids.max())
    assert np.array_equal(plan["users"].numpy(), users.numpy()) and np.array_equal(plan["pos"].numpy(), pos.numpy())
    assert np.array_equal(plan["neg"].numpy(), neg.numpy())
    stated = make_plan(users, pos, neg, id_range=((0, case[2] - 1), (0, case[3] - 1)))
    assert stated["user_range"] == (0, case[2] - 1) and torch.equal(stated["item_occ"], plan["item_occ"])
    with pytest.raises(RuntimeError, match=which + "_plan: user id outside the user table"):
        make_plan(users, pos, neg, n_users=int(users.max()))
    with pytest.raises(RuntimeError, match=which + r"_plan: users, pos, neg must be \(B,\)"):
        make_plan(users, pos[:-1], neg)


@pytest.fixture(scope="module")
def measured():
    """float32 torch against float64 torch at the GPU test's cases and edges, both modes: {(set, mode): [(tag, loss err /
    total, [gradient err / max]), ...]}, computed once and printed."""
    out = {}
    for name, items in (("cases", [(IDS(c), _inputs(c), COEF) for c in CASES]), ("edges", edge_cases())):
        for cold_user in MODES:
            rows = []
            for tag, inp, coef in items:
                want = gar_restate.step(*inp, *coef, cold_user)
                assert all(np.isfinite(x).all() for x in want)
                rel, errs = distances(gar_restate.step(*inp, *coef, cold_user, dtype=torch.float32), want)
                print(f"{name} {tag} {'user' if cold_user else 'item'}: float32 torch: loss err / total {rel:.2e}, gradient "
                      f"err / max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}; terms {want[0]}")
                rows.append((tag, rel, errs))
            out[(name, cold_user)] = rows
    return out


@pytest.mark.parametrize("cold_user", MODES, ids=lambda m: "user" if m else "item")
def test_float32_formula_stays_within_the_kernel_bars(measured, cold_user):
    """The measurement behind LOSS_BAR / GRAD_BAR and the edge bars of tests/test_gar_gpu.py, repeated: float32 torch
    against float64 torch at the GPU test's cases must itself lie within the bars (they are 8x its worst distance)."""
    for name, bars in (("cases", (LOSS_BAR, GRAD_BAR)), ("edges", (EDGE_LOSS_BAR, EDGE_GRAD_BAR))):
        for tag, rel, errs in measured[(name, cold_user)]:
            assert rel <= bars[0] and max(errs) <= bars[1], (name, tag, rel, errs)


def test_recorded_worst_figures_are_the_measured_ones(measured):
    """The recorded worst figures are the measured ones within a factor of 2 (another CPU's rounding moves them), so the
    bars stay what they claim to be."""
    for name, rec in (("cases", (F32_LOSS_WORST, F32_GRAD_WORST)), ("edges", (EDGE_F32_LOSS_WORST, EDGE_F32_GRAD_WORST))):
        rows = [r for m in MODES for r in measured[(name, m)]]
        worst = max(r[1] for r in rows), max(max(r[2]) for r in rows)
        print(f"worst over the {name}, both modes: loss err / total {worst[0]:.2e}, gradient err / max {worst[1]:.2e}")
        for k in range(2):
            assert rec[k] / 2 <= worst[k] <= 2 * rec[k], (name, k, worst[k], rec[k])
    assert (LOSS_BAR, GRAD_BAR) == (8 * F32_LOSS_WORST, 8 * F32_GRAD_WORST)
    assert EDGE_LOSS_BAR == max(8 * EDGE_F32_LOSS_WORST, LOSS_BAR) and EDGE_GRAD_BAR == max(8 * EDGE_F32_GRAD_WORST, GRAD_BAR)


def test_edge_inputs_are_the_edges_they_claim():
    edges = {tag: (inp, coef) for tag, inp, coef in edge_cases()}
    inp = edges["pos-is-neg"][0]
    assert int(inp[3][5]) == int(inp[4][5])
    inp = edges["pos-and-neg"][0]
    assert int(inp[3][0]) == int(inp[4][1]) == 7 and int(inp[4][0]) != 7 and int(inp[3][1]) != 7
    assert {edges[f"alpha{a}-beta{b}"][1][:2] for a in (0, 1) for b in (0, 1)} == {(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0)}
    assert edges["reg0"][1][2] == 0.0 and not edges["gen-zero"][0][5].any()
    inp = edges["first-and-last-rows"][0]
    assert {0, 49} <= set(inp[2].tolist()) and {0, 399} <= set(inp[3].tolist()) and {0, 399} <= set(inp[4].tolist())
    for cold_user in MODES:                           # G = 0: no NaN out of the zero-norm block
        got = gar_restate.step(*edges["gen-zero"][0], *edges["gen-zero"][1], cold_user)
        assert all(np.isfinite(x).all() for x in got)


# ---- the count cases of tests/test_owner_pass_gpu.py ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def count_measured():
    """At the count cases (tests/owner_cases.py: reg = B, unequal block norms, per-item counts of positives at the window
    and chunk edges), every width and both modes: {(d, mode): (loss err / total and [gradient err / max] of float32 torch,
    {mutation: worst gradient err / max of the mutated float64 restatement}, the same of the unmutated written-out
    form)}, computed once and printed.  On one thread: torch's multi-threaded CPU reductions change their order with the
    machine, and the block norms here run over up to 2746 x 256 elements."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _count_measured()
    finally:
        torch.set_num_threads(threads)


def _count_measured():
    out = {}
    for d in oc.WIDTHS:
        inp, coef = oc.gar_count_inputs(d)
        for cold_user in MODES:
            true, mutated, written = oc.gar_mutations(inp, coef, cold_user)
            assert all(np.isfinite(x).all() for x in true)
            rel, errs = distances(gar_restate.step(*inp, *coef, cold_user, dtype=torch.float32), true)
            far = {k: float(max(distances(m, true)[1])) for k, m in mutated.items()}
            print(f"counts d{d} {'user' if cold_user else 'item'}: float32 torch: loss err / total {rel:.2e}, gradient err / "
                  f"max {errs[0]:.2e} {errs[1]:.2e} {errs[2]:.2e}; mutated: " + ", ".join(f"{k} {v:.2e}" for k, v in far.items())
                  + f"; R / total {true[0][2] / true[0][3]:.3f}")
            out[(d, cold_user)] = (float(rel), [float(e) for e in errs], far, float(max(distances(written, true)[1])))
    return out


def test_count_cases_float32_figures_are_the_recorded_ones(count_measured):
    """The measurement behind COUNT_LOSS_BAR / COUNT_GRAD_BAR of tests/test_owner_pass_gpu.py, repeated: float32 torch lies
    within the bars (they are 8x its worst distance) and the recorded worst figures are the measured ones within a factor
    of 2."""
    worst = max(v[0] for v in count_measured.values()), max(max(v[1]) for v in count_measured.values())
    print(f"worst over the count cases, both modes: loss err / total {worst[0]:.2e}, gradient err / max {worst[1]:.2e}")
    for k, rec in enumerate((op.COUNT_F32_LOSS_WORST, op.COUNT_F32_GRAD_WORST)):
        assert rec / 2 <= worst[k] <= 2 * rec, (k, worst[k], rec)
    assert (op.COUNT_LOSS_BAR, op.COUNT_GRAD_BAR) == (8 * op.COUNT_F32_LOSS_WORST, 8 * op.COUNT_F32_GRAD_WORST)
    assert worst[0] <= op.COUNT_LOSS_BAR and worst[1] <= op.COUNT_GRAD_BAR


def test_count_cases_make_every_miscount_visible(count_measured):
    """The condition of the count cases: the regulariser's part written out (factor x count x row) is the restatement's,
    and with the counts swapped, every occurrence counted as a positive, one occurrence of a three-chunk owner miscounted,
    or R's part dropped on the user side, the float64 gradients lie at least 4 bars from the true ones, at every width and
    in both modes -- a kernel that got a count wrong could not pass tests/test_owner_pass_gpu.py."""
    least = {}
    for key, (_, _, far, written) in count_measured.items():
        assert written <= 1e-12, key
        assert set(far) == {"counts swapped", "all counted as positives", "one occurrence miscounted", "R dropped on the user side"}
        for name, v in far.items():
            assert v >= op.MUTATION_MARGIN * op.COUNT_GRAD_BAR, (key, name, v)
            least[name] = min(least.get(name, v), v)
    print("least over the widths and modes: " + ", ".join(f"{k} {v:.2e}" for k, v in least.items())
          + f"; bar {op.COUNT_GRAD_BAR:.2e}, {op.MUTATION_MARGIN} bars {op.MUTATION_MARGIN * op.COUNT_GRAD_BAR:.2e}")


# ---- whole runs against G24 --------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=COLD)
def restated(request):
    """The float64 and the float32 restatement of a G24 run, each on a fresh builder (the sampler shuffles in place)."""
    cold = request.param
    fx, out = load_golden(f"g24_gar_{cold}.npz"), {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        out[name] = gar_restate.run(gar_restate.toy_data(cold), fx["loaded_U"], fx["loaded_V"], dt, cold == "user")
    return cold, fx, out


def _best_tables(fx, r):
    return r["snaps"][int(fx["best_epoch"]) - 1]


def test_fixture_holds_what_the_issue_lists(restated):
    cold, fx, _ = restated
    assert str(fx["which"]) == "GAR" and str(fx["cold_object"]) == cold
    assert (int(fx["d"]), int(fx["batch_size"]), int(fx["epochs"]), int(fx["seed"]), int(fx["data_seed"])) == (64, 512, 2, 2024, 1)
    assert (float(fx["alpha"]), float(fx["beta"]), float(fx["lr"]), float(fx["reg"])) == (0.05, 0.1, 1e-3, 1e-4)
    assert fx["losses"].shape == (16, 3) and fx["loaded_U"].dtype == np.float32 == fx["user_emb"].dtype
    assert np.allclose(fx["losses"][:, 2], fx["losses"][:, 0] + fx["losses"][:, 1], atol=1e-3)          # + R, about 2e-5
    assert float(np.abs(fx["user_emb"] - fx["loaded_U"]).max()) > 1e-3                       # the tables are trained
    assert float(np.abs(fx["item_emb"] - fx["loaded_V"]).max()) > 1e-3


def test_float64_restatement_of_a_run_matches_reference_g24(restated):
    cold, fx, out = restated
    rel, errs = run_distances(fx, out["f64"]["losses"], _best_tables(fx, out["f64"]))
    print(f"float64 restatement, {cold}: worst loss-term difference to G24 over the total {rel:.2e}; best-epoch tables "
          f"differ by {errs[0]:.2e} / {errs[1]:.2e} of their scale")
    assert rel <= RUN_LOSS_BAR and max(errs) <= RUN_TABLE_BAR


def test_float32_restatement_ends_near_g24(restated):
    """How far plain float32 torch ends from the reference's own float32 run: 8x the figures stay below the project's run
    bars (1e-5 loss, 2e-4 tables), so those are the GPU run's bars.  Asserted: the figures are the recorded ones within a
    factor of 2 (another CPU's rounding moves them)."""
    cold, fx, out = restated
    rel, errs = run_distances(fx, out["f32"]["losses"], _best_tables(fx, out["f32"]))
    print(f"float32 restatement, {cold}: loss terms differ from G24 by {rel:.2e} of the total, best-epoch tables by "
          f"{errs[0]:.2e} / {errs[1]:.2e} of their scale")
    assert 8 * rel <= RUN_LOSS_BAR and 8 * max(errs) <= RUN_TABLE_BAR
    assert rel <= 2 * F32_RUN_LOSS[cold] and all(e <= 2 * m for e, m in zip(errs, F32_RUN_TABLES[cold]))


def _host_lists_and_metrics(fx, tables, data):
    """The three settings' top-20 lists of ``tables``, ranked here in float64, and their 5-dp metrics."""
    from coldrec_amd.util.evaluator import ranking_metrics, truth_csr
    U, V = (np.asarray(t, np.float64) for t in tables)
    lists, results = {}, {}
    for t, name, truth in (("all", "overall", data.overall_test_set), ("cold", "cold", data.cold_test_set),
                           ("warm", "warm", data.warm_test_set)):
        users, rp, rc = fx[f"{t}_users_int"], fx[f"{t}_rated_rowptr"], fx[f"{t}_rated_col"]
        S = U[users] @ V.T
        for r in range(len(users)):
            S[r, rc[rp[r]:rp[r + 1]]] = -1e9
        if fx[f"{t}_cand"].size:
            S[:, fx[f"{t}_cand"]] = -1e9
        lists[t] = np.argsort(-S, axis=1, kind="stable")[:, :20]
        _, gt_rowptr, gt_items = truth_csr(truth, item_of=data.item)
        results[name] = ranking_metrics(gt_rowptr, gt_items, lists[t], [10, 20])
    return lists, results


def test_float32_restatement_keeps_the_reference_lists_and_metrics(restated):
    """The list condition of the GPU run (at least half of the users with a determined ranking, min_frac = 0.5) holds for
    plain float32 torch on both fixtures, so it can be relied on there; the metrics follow the lists."""
    cold, fx, out = restated
    tables = _best_tables(fx, out["f32"])
    lists, results = _host_lists_and_metrics(fx, tables, gar_restate.toy_data(cold))
    same, det, total = lists_vs_reference(fx, tables, lists, min_frac=0.5)
    print(f"float32 restatement, {cold}: {same} of {total} lists identical to G24's ({det} with a determined ranking)")
    metrics_vs_reference(results, fx, same == total)
