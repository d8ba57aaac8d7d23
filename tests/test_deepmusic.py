"""CPU-only: DeepMusic's registry entry, flags and refusals, the kernel's workspace query and argument errors, the
derivation of the closed form, and the restatements of whole runs pinned to G27 (the reference's own MF.run() +
DeepMusic.run() on the toy item-cold and user-cold splits), which makes the closed form the oracle of the GPU tests.  The
distances of plain float32 torch from the float64 closed form and from G27 -- the figures the GPU tests' bars are 8x of --
are measured, printed and checked here, on one thread (torch's multi-threaded CPU reductions change their order with the
machine).

Measured: what tests/test_deepmusic_gpu.py's docstring records, and
    the closed form against the autograd form, both float64: 1.4e-14 at worst over the cases and edges (bar 1e-12);
    float64 closed-form run against G27: loss terms 2.09e-7 (item) / 1.11e-7 (user) of the total, the published table 2.69e-7 /
        2.90e-7 of its scale, the MLP's parameters 6.81e-7 / 2.95e-7.
"""
import argparse
import ctypes
import functools
import json
import types

import numpy as np
import pytest
import torch

from tests import deepmusic_restate as dr
from tests.conftest import load_golden
from tests.metaemb_restate import param_distances
from tests.test_deepmusic_gpu import (BARS, EDGE_BARS, EDGE_F32_WORST, F32_RUN_LOSS, F32_RUN_PARAMS, F32_RUN_TABLES, F32_WORST,
                                      RUN_LOSS_BAR, RUN_TABLE_BAR)
from tests.test_gar_gpu import lists_vs_reference, run_distances, write_loaded

COLD = ["item", "user"]
# A recorded run distance of 0 means float32 torch reproduced the reference bit for bit on the CPU that made the record;
# on another CPU or thread count its reductions round differently and the distance is a few float32 units (2.0e-7 of the
# total in loss terms, 2.4e-7 in parameters, measured on a 16-thread machine).  So a recorded figure is held to twice
# itself or to four float32 units, whichever is larger; 8 x four units (3.8e-6) still lies below the run bars.
ULP = 4 * 2.0 ** -23
NAMES = ["transformation.0.weight", "transformation.0.bias", "transformation.2.weight", "transformation.2.bias"]


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="DeepMusic", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def test_registry_resolves_deepmusic_without_changing_the_listings():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    from coldrec_amd.model.FusedLossTrainer import FusedLossTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert "DeepMusic" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["DeepMusic"]
    assert issubclass(cls, FusedLossTrainer) and AVAILABLE_MODELS.get("DeepMusic") is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert "DeepMusic" not in keys and "DeepMusic" not in names and "DeepMusic" in resolvable()
    assert cls.fused_eval is True and cls._eval_parts is BaseColdStartTrainer._eval_parts       # the one-table ranking
    assert cls.LOSS_TERMS == ("mse", "reg", "batch_loss") and cls.TABLES == ("user_emb", "item_emb")
    assert cls.SAVE_FILES is None                                                 # --save_emb: user_emb / item_emb


def test_cli_takes_no_flags_of_its_own():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "DeepMusic", "--cold_object", "user"])
    assert (a.backbone, a.cold_object, a.reg) == ("MF", "user", 0.0001) and not hasattr(a, "alpha")


@pytest.mark.parametrize("cold", COLD)
def test_refusals_and_construction(cold, tmp_path, monkeypatch):
    from coldrec_amd.model import AVAILABLE_MODELS
    data = dr.toy_data(cold)
    new = AVAILABLE_MODELS["DeepMusic"]
    monkeypatch.chdir(tmp_path)
    fx = load_golden(f"g27_deepmusic_{cold}.npz")
    with pytest.raises(FileNotFoundError, match=rf"DeepMusic requires ./emb/toy_cold_{cold}_MF_user_emb.pt. Train the "
                                                rf"backbone first \(e.g. main.py --model MF --dataset toy --cold_object {cold} "
                                                rf"--save_emb true\)"):
        new(_cfg(data, cold_object=cold))
    write_loaded(fx, tmp_path, cold)
    with pytest.raises(ValueError, match="DeepMusic: --emb_size 50 must be a multiple of 4"):
        new(_cfg(data, cold_object=cold, emb_size=50))
    with pytest.raises(ValueError, match="DeepMusic: --emb_size 260 must be a multiple of 4"):
        new(_cfg(data, cold_object=cold, emb_size=260))
    with pytest.raises(ValueError, match="do not fit this dataset"):
        new(_cfg(data, cold_object=cold, emb_size=32))
    tr = new(_cfg(data, cold_object=cold, lr=0.02, reg=0.3))
    m = tr.model
    assert m.reg == 0.3 and m.cold_user == (cold == "user")
    assert [n for n, _ in m.named_parameters()] == NAMES                                   # the tables are frozen
    assert not m.user_emb.requires_grad and np.array_equal(m.user_emb.numpy(), fx["loaded_U"])
    assert np.array_equal(m.item_emb.numpy(), fx["loaded_V"])
    assert m.content.shape == ((data.user_num if cold == "user" else data.item_num), 16)
    opt, = tr._optimizers(m)
    assert isinstance(opt, torch.optim.Adam) and opt.defaults["lr"] == 0.02
    assert sum(len(g["params"]) for g in opt.param_groups) == 4
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.loss(torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "dp_from_env", lambda: object())  # a data-parallel launch is refused before anything runs
    tr.device = torch.device("cuda:0")
    with pytest.raises(RuntimeError, match="DeepMusic: data-parallel"):
        tr.train()


@pytest.mark.parametrize("cold", COLD)
def test_encoder_draws_the_reference_mlp(cold, tmp_path, monkeypatch):
    """The encoder's initial parameters are G27's bit for bit: the MLP is drawn from the reference's stream."""
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    fx = load_golden(f"g27_deepmusic_{cold}.npz")
    write_loaded(fx, tmp_path, cold)
    monkeypatch.chdir(tmp_path)
    set_seed(2024, False)
    tr = AVAILABLE_MODELS["DeepMusic"](_cfg(dr.toy_data(cold), cold_object=cold))
    params = list(tr.model.transformation.parameters())
    assert len(params) == int(fx["n_params"]) == 4
    for k, p in enumerate(params):
        assert np.array_equal(p.detach().numpy(), fx[f"gen_init_{k}"])


@pytest.mark.parametrize("cold", COLD)
def test_current_tables_replace_exactly_the_cold_rows_and_are_copies(cold, tmp_path, monkeypatch):
    from coldrec_amd.model import AVAILABLE_MODELS
    fx = load_golden(f"g27_deepmusic_{cold}.npz")
    write_loaded(fx, tmp_path, cold)
    monkeypatch.chdir(tmp_path)
    data = dr.toy_data(cold)
    tr = AVAILABLE_MODELS["DeepMusic"](_cfg(data, cold_object=cold))
    m = tr.model
    with torch.no_grad():
        user, item = tr._current_tables()
    assert not m.training and user.data_ptr() != m.user_emb.data_ptr() and item.data_ptr() != m.item_emb.data_ptr()
    made, kept, loaded = (user, item, m.user_emb) if cold == "user" else (item, user, m.item_emb)
    idx = torch.as_tensor(np.asarray(data.mapped_cold_user_idx if cold == "user" else data.mapped_cold_item_idx))
    is_cold = torch.zeros(made.shape[0], dtype=torch.bool)
    is_cold[idx] = True
    assert torch.equal(kept, m.item_emb if cold == "user" else m.user_emb) and torch.equal(made[~is_cold], loaded[~is_cold])
    with torch.no_grad():
        want = m.transformation(m.content[idx])
    assert is_cold.any() and torch.equal(made[idx], want) and not made.requires_grad
    made.zero_()                                                          # a copy: the frozen tables keep their bits
    assert np.array_equal(m.user_emb.numpy(), fx["loaded_U"]) and np.array_equal(m.item_emb.numpy(), fx["loaded_V"])
    data.mapped_cold_user_idx, data.mapped_cold_item_idx = [], []         # an empty cold set: nothing is replaced
    tr._cold_idx = None
    with torch.no_grad():
        user, item = tr._current_tables()
    assert torch.equal(user, m.user_emb) and torch.equal(item, m.item_emb)


def test_queries_and_argument_errors_without_gpu():
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    assert L.crh_deepmusic_workspace_bytes(4096, 64) >= 4096 * 16 and L.crh_deepmusic_workspace_bytes(1, 4) > 0
    assert L.crh_deepmusic_workspace_bytes(512, 6) == 0 and L.crh_deepmusic_workspace_bytes(512, 260) == 0     # width
    assert L.crh_deepmusic_workspace_bytes(0, 64) == 0 and L.crh_deepmusic_workspace_bytes(1 << 31, 64) == 0   # B
    sizes = [ops.deepmusic_workspace_bytes(n, 64) for n in (1, 2, 63, 64, 65, 512, 513, 4096, 65536)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
    buf = (ctypes.c_float * 64)()                       # host memory: the argument checks end the call before any launch
    p = ctypes.addressof(buf)
    for args, text in (((None, 11, p, 0, 10, p, 2, 4, 1e-4, 1., p, p, p, 64, None), "NULL table"),
                       ((p, 11, None, 0, 10, p, 2, 4, 1e-4, 1., p, p, p, 64, None), "NULL id"),
                       ((p, 11, p, 0, 10, None, 2, 4, 1e-4, 1., p, p, p, 64, None), "NULL table"),
                       ((p, 11, p, 0, 10, p, 2, 4, 1e-4, 1., None, None, p, 64, None), "nothing to compute"),
                       ((p, 11, p, 0, 10, p, 2, 6, 1e-4, 1., p, p, p, 64, None), "d = 6 must be a multiple of 4"),
                       ((p, 11, p, 0, 11, p, 2, 4, 1e-4, 1., p, p, p, 64, None), "outside the frozen table of 11 rows"),
                       ((p, 11, p, 0, 10, p, 0, 4, 1e-4, 1., p, p, p, 64, None), "batch = 0"),
                       ((p, 11, p, 0, 10, p + 4, 2, 4, 1e-4, 1., p, p, p, 64, None), "16-byte aligned")):
        assert L.crh_deepmusic_f32(*args) == -1 and text in L.crh_last_error().decode(), text
    assert L.crh_deepmusic_f32(p, 11, p, 0, 10, p, 2, 4, 1e-4, 1., p, p, None, 64, None) == -3            # CRH_ERR_WS
    assert "workspace" in L.crh_last_error().decode()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.deepmusic(torch.zeros(11, 4), torch.zeros(2, dtype=torch.long), torch.zeros(2, 4), 1e-4)


# ---- the derivation, and the measurements behind the GPU tests' bars ---------------------------------------------------

ALL = [("cases",) + r for r in dr.case_runs()] + [("edges",) + e for e in dr.edge_cases()]


@pytest.mark.parametrize("run", ALL, ids=lambda r: r[1])
def test_closed_form_equals_the_autograd_form_in_float64(run):
    """The derivation, independently of any kernel: the formulas equal what autograd makes of the reference's loss."""
    _, tag, inp, reg = run
    closed, auto = dr.closed_form(*inp, reg), dr.step(*inp, reg)
    for a, b in zip(closed, auto):
        assert np.isfinite(a).all() and np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), tag


def test_edges_are_what_they_claim():
    runs = {r[1]: r[2:] for r in ALL}
    assert runs["reg0"][1] == 0.0 and not runs["gen-zero"][0][2].any() and runs["gen-zero"][1] > 0
    T, ids, G = runs["gen-is-table"][0]
    assert torch.equal(G, T[ids]) and dr.closed_form(T, ids, G, 0.65)[0][0] == 0
    assert {0, 49} <= set(runs["first-and-last-rows"][0][1].tolist()) and len(set(runs["ids-equal"][0][1].tolist())) == 1
    assert max(np.bincount(runs["B300-d256"][0][1].numpy())) >= 20               # heavy id repeats
    got = dr.closed_form(*runs["gen-zero"][0], runs["gen-zero"][1])              # G = 0: no NaN out of the zero norm
    assert np.isfinite(got[1]).all() and got[0][1] == 0


@pytest.fixture(scope="module")
def measured():
    """float32 torch, the reference's way, against the float64 closed form at the GPU test's cases and edges:
    {set: [(tag, loss err / total, gradient err / max), ...]}, computed once, on one thread, and printed."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {"cases": [], "edges": []}
        for name, tag, inp, reg in ALL:
            want = dr.closed_form(*inp, reg)
            dist = dr.distances(dr.step(*inp, reg, dtype=torch.float32), want)
            print(f"{name} {tag}: float32 torch: loss err / total {dist[0]:.2e}, gradient err / max {dist[1]:.2e}; terms {want[0]}")
            out[name].append((tag,) + dist)
        return out
    finally:
        torch.set_num_threads(threads)


def test_float32_formula_stays_within_the_kernel_bars_and_is_the_recorded_one(measured):
    """The measurement behind the bars of tests/test_deepmusic_gpu.py, repeated: float32 torch lies within them (they are
    8x its worst distance) and the recorded worst figures are the measured ones within a factor of 2."""
    for name, bars, rec in (("cases", BARS, F32_WORST), ("edges", EDGE_BARS, EDGE_F32_WORST)):
        worst = [max(r[1 + k] for r in measured[name]) for k in range(2)]
        print(f"worst over the {name}: loss {worst[0]:.2e}, gradient {worst[1]:.2e}")
        for k in range(2):
            assert worst[k] <= bars[k] and rec[k] / 2 <= worst[k] <= 2 * rec[k], (name, k, worst[k], rec[k])
    assert BARS == tuple(8 * w for w in F32_WORST)
    assert EDGE_BARS == tuple(max(8 * e, b) for e, b in zip(EDGE_F32_WORST, BARS))


# ---- whole runs against G27 --------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _restated(cold):
    """The float64 closed-form and the float32 reference-way restatement of a G27 run, each on a fresh builder; once, on
    one thread as the fixture's maker ran."""
    fx = load_golden(f"g27_deepmusic_{cold}.npz")
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        out = {name: dr.run(dr.toy_data(cold), fx["loaded_U"], fx["loaded_V"], dt, cold == "user", closed=closed)
               for name, dt, closed in (("f64", torch.float64, True), ("f32", torch.float32, False))}
    finally:
        torch.set_num_threads(threads)
    return fx, out


def _run_distances(fx, r):
    rel, errs = run_distances(fx, r["losses"], r["snaps"][int(fx["best_epoch"]) - 1])
    return rel, errs, max(param_distances(fx, r["params"]))


@pytest.mark.parametrize("cold", COLD)
def test_fixture_holds_what_the_issue_lists(cold):
    fx, out = _restated(cold)
    assert str(fx["which"]) == "DeepMusic" and str(fx["cold_object"]) == cold
    assert (int(fx["d"]), int(fx["batch_size"]), int(fx["epochs"]), int(fx["seed"]), int(fx["data_seed"])) == (64, 512, 2, 2024, 1)
    assert (float(fx["lr"]), float(fx["reg"])) == (1e-3, 1e-4) and fx["losses"].shape == (16, 3)
    assert np.allclose(fx["losses"][:, 2], fx["losses"][:, 0] + fx["losses"][:, 1], rtol=1e-6) and (fx["losses"][:, 1] > 0).all()
    assert [fx[f"gen_init_{k}"].shape for k in range(4)] == [(128, 16), (128,), (64, 128), (64,)]
    assert float(np.abs(fx["gen_final_0"] - fx["gen_init_0"]).max()) > 1e-3               # the MLP is trained
    for k, p in enumerate(out["f32"]["init"]):
        assert np.array_equal(p, fx[f"gen_init_{k}"])
    assert len(json.loads(str(fx["loss_lines"]))) == 2
    assert np.array_equal(fx["user_emb" if cold == "item" else "item_emb"], fx["loaded_U" if cold == "item" else "loaded_V"])


@pytest.mark.parametrize("cold", COLD)
def test_float64_closed_form_run_matches_reference_g27(cold):
    fx, out = _restated(cold)
    rel, errs, perr = _run_distances(fx, out["f64"])
    print(f"float64 closed-form run, {cold}: loss terms differ from G27 by {rel:.2e} of the total; best-epoch tables by "
          f"{errs[0]:.2e} / {errs[1]:.2e} of their scale, parameters by {perr:.2e}")
    assert rel <= RUN_LOSS_BAR and max(errs) <= RUN_TABLE_BAR and perr <= RUN_TABLE_BAR


@pytest.mark.parametrize("cold", COLD)
def test_float32_restatement_ends_near_g27(cold):
    """How far plain float32 torch ends from the reference's own float32 run: 8x the figures stay below the project's run
    bars (1e-5 loss, 2e-4 tables and parameters), so those are the GPU run's bars.  Asserted: the figures are the recorded
    ones within a factor of 2 (or four float32 units: see ULP)."""
    fx, out = _restated(cold)
    rel, errs, perr = _run_distances(fx, out["f32"])
    print(f"float32 restatement, {cold}: loss terms differ from G27 by {rel:.2e} of the total; best-epoch tables by "
          f"{errs[0]:.2e} / {errs[1]:.2e} of their scale, parameters by {perr:.2e}")
    assert 8 * rel <= RUN_LOSS_BAR and 8 * max(errs) <= RUN_TABLE_BAR and 8 * perr <= RUN_TABLE_BAR
    assert rel <= max(2 * F32_RUN_LOSS[cold], ULP) and perr <= max(2 * F32_RUN_PARAMS[cold], ULP)
    assert all(e <= max(2 * m, ULP) for e, m in zip(errs, F32_RUN_TABLES[cold]))


@pytest.mark.parametrize("cold", COLD)
def test_reference_lists_are_determined_for_half_the_users(cold):
    """The list condition of the GPU run (min_frac = 0.5) holds for plain float32 torch on both fixtures."""
    fx, out = _restated(cold)
    same, det, total = lists_vs_reference(fx, out["f32"]["snaps"][int(fx["best_epoch"]) - 1], None, min_frac=0.5)
    print(f"float32 restatement, {cold}: {same} of {total} lists identical to G27's ({det} with a determined ranking)")
