"""CPU-only: CLCRec's registry entry, flags and refusals, and the float64 restatement of a whole run pinned to G20 (the
reference's own CLCRec.run() on the toy item-cold split), which makes the restatement the oracle of the GPU tests."""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import clcrec_restate
from tests.conftest import load_golden
from tests.test_host_logic import builder

HYPER = dict(num_neg=16, temp_value=2.0, lr_lambda=0.5, num_sample=0.5)


def _cfg(data, device="cpu", **kw):
    a = dict(dataset="toy", model="CLCRec", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=False, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1, **HYPER)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def test_registry_resolves_clcrec_without_changing_the_listings():
    from coldrec_amd.model import AVAILABLE_MODELS, resolvable
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    keys, names = list(AVAILABLE_MODELS.keys()), list(AVAILABLE_MODELS.names())
    assert "CLCRec" in AVAILABLE_MODELS
    cls = AVAILABLE_MODELS["CLCRec"]
    assert issubclass(cls, BaseColdStartTrainer) and AVAILABLE_MODELS.get("CLCRec") is cls
    assert list(AVAILABLE_MODELS.keys()) == keys and list(AVAILABLE_MODELS.names()) == names
    assert "CLCRec" not in keys and "CLCRec" not in names
    assert "CLCRec" in resolvable() and set(names) <= set(resolvable())


def test_cli_carries_the_reference_defaults():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "CLCRec"])
    assert (a.num_neg, a.temp_value, a.lr_lambda, a.num_sample) == (128, 2.0, 0.5, 0.5)
    assert parse_args(["--model", "CLCRec", "--num_neg", "16"]).num_neg == 16
    with pytest.raises(ValueError, match="CLCRec"):            # the error lists everything a --model flag can name
        parse_args(["--model", "NoSuchModel"])


def test_refusals():
    from coldrec_amd.model import AVAILABLE_MODELS
    _, data = builder()
    with pytest.raises(Exception, match="Cold user is not supported in CLCRec"):
        AVAILABLE_MODELS["CLCRec"](_cfg(data, cold_object="user"))
    with pytest.raises(ValueError, match="multiple of 4"):
        AVAILABLE_MODELS["CLCRec"](_cfg(data, emb_size=50))
    with pytest.raises(ValueError, match="multiple of 4"):
        AVAILABLE_MODELS["CLCRec"](_cfg(data, emb_size=260))
    tr = AVAILABLE_MODELS["CLCRec"](_cfg(data))
    with pytest.raises(RuntimeError, match="MI355X only"):
        tr.train()


def test_argument_errors_without_gpu():
    from coldrec_amd import _lib
    L = _lib.lib()
    assert L.crh_clcrec_max_neg() >= 256 and L.crh_clcrec_chunk_rows() >= 64
    assert L.crh_clcrec_workspace_bytes(512, 16, 64, 300) > 0
    assert L.crh_clcrec_workspace_bytes(512, 16, 6, 300) == 0 and L.crh_clcrec_workspace_bytes(512, 0, 64, 300) == 0


@pytest.fixture(scope="module")
def restated():
    """The float64 and the float32 restatement of the G20 run, each on a fresh builder (the sampler shuffles in place)."""
    out = {}
    for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
        _, data = builder()
        out[name] = clcrec_restate.run(data, dt, reg=1e-4, **{"num_neg": 16, "temp": 2.0, "lam": 0.5, "num_sample": 0.5})
        out[name]["cold_idx"] = np.asarray(data.mapped_cold_item_idx)
    return out


def test_float64_restatement_of_a_run_matches_reference_g20(restated):
    fx, r = load_golden("g20_clcrec.npz"), restated["f64"]
    assert r["U0_crc"] == int(fx["U0_crc"]) and r["V0_crc"] == int(fx["V0_crc"])
    assert r["randint_crc"] == int(fx["randint_crc"]), "torch's CPU integer stream differs from the fixture's"
    assert r["losses"].shape == fx["losses"].shape == (16, 4)
    rel = np.abs(r["losses"] - fx["losses"]) / np.abs(fx["losses"])
    print(f"float64 restatement: worst relative loss difference to G20 {rel.max():.2e} (per term {rel.max(axis=0)})")
    assert rel.max() <= 1e-5


def test_float32_restatement_ends_near_g20(restated):
    """How far plain float32 torch ends from the reference's own float32 run (other summation orders only): the figure the
    GPU run's table bar is judged against.  Printed; the bar itself (2e-4 of the table scale, G19's) is asserted here too."""
    fx, r = load_golden("g20_clcrec.npz"), restated["f32"]
    V = r["V"].copy()
    V[r["cold_idx"]] = r["cold"]
    eu = np.abs(r["U"] - fx["U"]).max() / np.abs(fx["U"]).max()
    ev = np.abs(V - fx["V"]).max() / np.abs(fx["V"]).max()
    print(f"float32 restatement: final tables differ from G20 by {eu:.2e} / {ev:.2e} of their scale")
    assert eu < 2e-4 and ev < 2e-4


def test_float32_formula_at_the_large_logit_cases_stays_within_the_bars():
    """tests/test_loss_edges_gpu.py holds the kernel to this file's fixed bars (1e-5 of a loss term, 1e-4 of a gradient's
    maximum) where the second softmax's scores are hundreds apart: float32 torch against float64 torch there, printed.
    Measured: loss terms 5.0e-8 / 8.1e-8, gradients 3.0e-6 / 1.8e-5."""
    from tests import test_loss_edges_gpu as edges
    from tests.test_clcrec_gpu import REG
    for scales in edges.CLC_LOGIT_SCALES:
        case, inp = edges.clc_big_logit_inputs(*scales)
        want = clcrec_restate.step(*inp, case[5], case[6], REG)
        got = clcrec_restate.step(*inp, case[5], case[6], REG, dtype=torch.float32)
        rel = (np.abs(got[0] - want[0]) / np.abs(want[0])).max()
        errs = [np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got[1:], want[1:])]
        print(f"U, V, feat, T = {scales}: float32 torch: loss rel {rel:.2e}, gradient err / max {errs[0]:.2e} {errs[1]:.2e} "
              f"{errs[2]:.2e}; terms {want[0]}")
        assert np.isfinite(want[0]).all() and rel <= 1e-5 and max(errs) <= 1e-4
