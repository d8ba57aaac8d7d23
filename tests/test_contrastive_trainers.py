"""CPU-only: the built-in SimGCL / XSimGCL trainers resolve by name without changing what the registry lists, their flags
parse, their argument rules hold, and the G19 fixtures (the reference's own SimGCL.run() / XSimGCL.run() on the toy split,
tests/golden/make_golden_g19.py) are reproduced by the float64 restatement of tests/cl_restate.py from the same random
streams -- which pins the order of the noise draws the ``--cl_noise host`` mode has to follow."""
import argparse
import types

import numpy as np
import pytest
import torch

from tests import cl_restate
from tests.conftest import load_golden
from tests.test_host_logic import builder

CORE = ["DropoutNet", "LightGCN", "MF"]


def _cfg(data, model, device="cpu", **kw):
    a = dict(dataset="toy", model=model, epochs=2, layers=3, topN="10,20", bs=512, emb_size=64, lr=1e-3, reg=1e-4,
             early_stop=10, eval_every=1, cold_object="item", save_emb=False, seed=2024, cl_rate=0.5, tau=0.2, eps=0.1,
             l_cl=2, cl_noise="host")
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def test_contrastive_trainers_resolve_by_name_and_keys_stay_the_core_trainers():
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    before = sorted(AVAILABLE_MODELS.keys())
    for name in ("SimGCL", "XSimGCL"):
        assert name in AVAILABLE_MODELS
        cls = AVAILABLE_MODELS[name]
        assert isinstance(cls, type) and issubclass(cls, BaseColdStartTrainer) and cls.__name__ == name
        assert AVAILABLE_MODELS.get(name) is cls and cls.fused_eval
    assert sorted(AVAILABLE_MODELS.keys()) == before            # resolving a name does not change the listing
    assert [n for n in before if n in CORE] == CORE and "SimGCL" not in before and "XSimGCL" not in before
    assert [n for n in AVAILABLE_MODELS.names() if n in CORE + ["SimGCL", "XSimGCL"]] == \
        ["DropoutNet", "LightGCN", "MF", "SimGCL", "XSimGCL"]
    assert set(AVAILABLE_MODELS.names()) == set(before) | {"SimGCL", "XSimGCL"}
    assert "NoSuchModel" not in AVAILABLE_MODELS and AVAILABLE_MODELS.get("NoSuchModel") is None
    with pytest.raises(KeyError):
        AVAILABLE_MODELS["NoSuchModel"]


def test_cli_parser_knows_the_contrastive_flags():
    from coldrec_amd.main import parse_args
    a = parse_args(["--model", "XSimGCL", "--l_cl", "2", "--eps", "0.2"])
    assert (a.model, a.l_cl, a.eps, a.cl_rate, a.tau, a.cl_noise) == ("XSimGCL", 2, 0.2, 0.5, 0.2, "device")
    a = parse_args(["--model", "SimGCL", "--cl_noise", "host", "--tau", "0.1"])
    assert (a.cl_noise, a.tau, a.eps) == ("host", 0.1, 0.1) and not hasattr(a, "l_cl")
    assert parse_args(["--model", "XSimGCL"]).l_cl == 2       # the reference's default
    with pytest.raises(ValueError, match="SimGCL"):             # the error message lists every name that resolves
        parse_args(["--model", "NoSuchModel"])


def test_l_cl_rule_and_cpu_refusal():
    from coldrec_amd.model import AVAILABLE_MODELS
    _, data = builder()
    for bad in (0, 4):                                          # layers = 3
        with pytest.raises(ValueError, match="1 <= l_cl <= layers"):
            AVAILABLE_MODELS["XSimGCL"](_cfg(data, "XSimGCL", l_cl=bad))
    for name in ("SimGCL", "XSimGCL"):
        with pytest.raises(RuntimeError, match="MI355X only"):
            AVAILABLE_MODELS[name](_cfg(data, name)).train()


def test_numpy_philox_known_answer():
    """Philox4x32-10 known-answer vector of Random123 (counter and key all zero) through the helper's layout:
    counter word 0 = column group index, words 2, 3 = the draw, key = seed."""
    # counter (0,0,0,0), key (0,0) -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
    u = cl_restate.philox_uniform(1, 4, 0, 0)[0]
    want = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], np.uint64)
    np.testing.assert_array_equal(u, ((want >> np.uint64(8)).astype(np.float64) * 2.0 ** -24).astype(np.float32))
    r = cl_restate.philox_uniform(63, 12, 7, 3)
    assert r.shape == (63, 12) and r.dtype == np.float32 and (r >= 0).all() and (r < 1).all()
    assert not np.array_equal(r, cl_restate.philox_uniform(63, 12, 7, 4))
    assert abs(float(cl_restate.philox_uniform(1000, 64, 1, 0).mean()) - 0.5) < 0.01


@pytest.mark.parametrize("which, mode", [("g19_simgcl.npz", "simgcl"), ("g19_xsimgcl.npz", "xsimgcl")])
def test_float64_restatement_reproduces_g19(which, mode):
    """Every loss term of the reference's run within 1e-5 relative, from outside: same xavier tables (checksums), same
    triples, and torch.rand((N, d), float32) drawn once per perturbed layer in the reference's order (first draw's
    checksum).  Measured when the fixture was made: worst relative difference 3.1e-7 (both models)."""
    fx = load_golden(which)
    _, data = builder()
    got = cl_restate.run_f64(data, mode, int(fx["layers"]), int(fx["d"]), int(fx["epochs"]), int(fx["batch_size"]),
                             float(fx["cl_rate"]), float(fx["tau"]), float(fx["eps"]), l_cl=max(int(fx["l_cl"]), 1),
                             lr=float(fx["lr"]), reg=float(fx["reg"]), seed=int(fx["seed"]))
    assert got["U0_crc"] == int(fx["U0_crc"]) and got["V0_crc"] == int(fx["V0_crc"])
    assert got["noise_crc"] == int(fx["noise_crc"]), "torch's CPU uniform stream differs from the fixture's"
    assert tuple(fx["noise_shape"]) == (data.user_num + data.item_num, int(fx["d"]))
    want = fx["losses"]
    assert got["losses"].shape == want.shape == (int(fx["n_steps"]), 4)
    rel = np.abs(got["losses"] - want) / np.abs(want)
    print(f"{which}: worst relative loss difference {rel.max():.2e}")
    assert rel.max() <= 1e-5
