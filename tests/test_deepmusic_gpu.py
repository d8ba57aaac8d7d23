"""GPU: the fused DeepMusic loss (csrc/deepmusic.hip) against the float64 closed form (tests/deepmusic_restate.py, itself
pinned to the autograd form and to the reference's runs by tests/test_deepmusic.py): the shapes where it can go wrong, its
edges, its determinism contract, the argument errors, the trainer's autograd operator, and whole runs against G27.

Bars of the kernel against the float64 closed form: 8x the worst distance of the float32 torch formula (the reference's
way, F.mse_loss, torch.norm and autograd, on the CPU) from the float64 one at the same cases.  Loss terms are measured as
error over the TOTAL loss, the gradient as error over its maximum.  The cases run at reg = B / 100, which keeps R between
5 % and 85 % of the total.  Measured on the CPU on one thread (tests/test_deepmusic.py prints them again and holds them to
a factor of 2):
    cases:  loss terms 3.48e-7 (B300-d256), gradient 4.06e-7 (B300-d256: float32 torch's norm of a 300 x 256 block)
            -> LOSS_BAR = 2.78e-6, GRAD_BAR = 3.25e-6
    edges:  loss terms 8.11e-8 (G = 0), gradient 9.85e-8 (G = T[ids])     (below the cases': the edge bars are the cases')
On the MI355X the kernel measures 9.12e-8 (loss terms, B65-d252) and 1.30e-7 (gradient, B63-d64) at worst over the cases,
6.85e-8 and 1.06e-7 over the edges (both at the first and last rows).

Whole runs against G27: plain float32 torch on the CPU, the reference's way (tests/test_deepmusic.py), reproduces both
of G27's runs bit for bit on the CPU that made the fixture (distance 0 in loss terms, tables and parameters; on another
CPU 2.0e-7 of the total, 1.5e-7 and 2.4e-7), so the project's run bars, 1e-5 and 2e-4, are the bars.
On the MI355X the runs end 2.28e-7 (item) / 1.11e-7 (user) of the total from G27's loss terms, 2.95e-7 / 2.57e-7 of the
published table's scale from its tables and 3.84e-7 / 2.92e-7 from the MLP's parameters; every one of the 750 / 456 final
lists equals the reference's (739 / 451 users with a determined ranking).
"""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import deepmusic_restate as dr
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference, metrics_vs_reference, run_distances, write_loaded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_WORST = (3.48e-7, 4.06e-7)                  # float32 torch against the float64 closed form at the cases: loss, gradient
BARS = tuple(8 * w for w in F32_WORST)
EDGE_F32_WORST = (8.11e-8, 9.85e-8)             # ... at the edge cases
EDGE_BARS = tuple(max(8 * e, b) for e, b in zip(EDGE_F32_WORST, BARS))
RUN_LOSS_BAR, RUN_TABLE_BAR = 1e-5, 2e-4        # the project's run bars (see above)
F32_RUN_LOSS = dict(item=0.0, user=0.0)         # float32 torch against G27, measured: bit for bit
F32_RUN_TABLES = dict(item=(0.0, 0.0), user=(0.0, 0.0))
F32_RUN_PARAMS = dict(item=0.0, user=0.0)


def _fused(inp, reg, **kw):
    from coldrec_amd import ops
    T, ids, G = (t.to(DEV) for t in inp)
    loss, grad = ops.deepmusic(T, ids, G, reg, **kw)
    torch.cuda.synchronize()
    return loss.cpu(), grad


def _compare(tag, got, want, bars=BARS):
    got = (got[0].numpy(), got[1].cpu().numpy())
    assert all(np.isfinite(g).all() for g in got)
    rel, err = dr.distances(got, want)
    print(f"{tag}: loss err / total {rel:.2e}, gradient err / max {err:.2e}")
    assert rel <= bars[0]
    assert err <= bars[1]
    return got


@pytest.mark.parametrize("run", dr.case_runs(), ids=lambda r: r[0])
def test_kernel_matches_float64_closed_form(run):
    tag, inp, reg = run
    want = dr.closed_form(*inp, reg)
    _compare(tag, _fused(inp, reg), want)
    assert 0.04 * want[0][2] <= want[0][1] <= 0.9 * want[0][2]          # both terms are visible in the total


@pytest.mark.parametrize("edge", dr.edge_cases(), ids=lambda e: e[0])
def test_edges(edge):
    tag, inp, reg = edge
    want = dr.closed_form(*inp, reg)
    loss, grad = _compare(tag, _fused(inp, reg), want, EDGE_BARS)
    if tag == "reg0":
        assert loss[1] == 0 and loss[2] == loss[0]
    if tag == "gen-zero":                         # the zero-norm branch: no NaN, the gradient is the mse part alone
        assert loss[1] == 0 and loss[2] == loss[0] > 0 and not inp[2].any()
    if tag == "gen-is-table":
        assert loss[0] == 0 and loss[2] == loss[1] > 0 and torch.equal(inp[2], inp[0][inp[1]])
    if tag == "first-and-last-rows":
        assert {0, 49} <= set(inp[1].tolist())
    if tag == "ids-equal":
        assert len(set(inp[1].tolist())) == 1


@pytest.mark.parametrize("run", [dr.case_runs()[2], dr.case_runs()[6]], ids=lambda r: r[0])
def test_determinism_scale_and_outputs_not_asked_for(run):
    from coldrec_amd import _lib, ops
    tag, inp, reg = run
    a, b = _fused(inp, reg), _fused(inp, reg)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    half = _fused(inp, reg, scale=0.5)                # (a power of two scales every product exactly)
    assert torch.equal(half[0], a[0]) and torch.equal(half[1], a[1] * 0.5)
    no_grad = _fused(inp, reg, want_grad=False)
    assert no_grad[1] is None and torch.equal(no_grad[0], a[0])
    # through the C ABI: a NULL output is not written, the other keeps its bits
    T, ids, G = (t.to(DEV).contiguous() for t in inp)
    ids = ids.to(torch.int32)
    B, d = G.shape
    ws = ops.deepmusic_workspace(B, d, DEV)
    for skip in range(2):
        out = [torch.full((B, d), -7.0, device=DEV), torch.full((3,), -7.0, device=DEV)]
        ptrs = [None if k == skip else t.data_ptr() for k, t in enumerate(out)]
        rc = _lib.lib().crh_deepmusic_f32(T.data_ptr(), T.shape[0], ids.data_ptr(), 0, T.shape[0] - 1, G.data_ptr(), B, d, reg,
                                          1.0, *ptrs, ws.data_ptr(), ws.numel(), _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == 0
        for k, (t, ref) in enumerate(zip(out, (a[1], a[0].to(DEV)))):
            assert (t == -7.0).all() if k == skip else torch.equal(t, ref)


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    T, ids, G = (t.to(DEV).contiguous() for t in dr.inputs((2, 4, 11)))
    ids32 = ids.to(torch.int32)
    L = _lib.lib()
    p = lambda t: t.data_ptr()

    def call(d=4, batch=2, ws="ok", rows=11, rng=(0, 10), shift=0, table=True, idp=True, reg=1e-4):
        space = ops.deepmusic_workspace(2, 4, DEV)
        out = [torch.full((2, 4), -7.0, device=DEV), torch.full((3,), -7.0, device=DEV)]
        ws_ptr, ws_bytes = {"ok": (p(space), space.numel()), "null": (0, space.numel()), "short": (p(space), 16)}[ws]
        rc = L.crh_deepmusic_f32(p(T) if table else None, rows, p(ids32) if idp else None, rng[0], rng[1], p(G) + shift, batch,
                                 d, reg, 1.0, p(out[0]), p(out[1]), ws_ptr, ws_bytes, _lib.current_stream())
        torch.cuda.synchronize()
        assert all((t == -7.0).all() for t in out)                     # nothing ran
        return rc, L.crh_last_error().decode()

    ARG, WS = -1, -3                                                   # CRH_ERR_ARG, CRH_ERR_WS of include/coldrec_hip.h
    for kw, rc, text in ((dict(d=6), ARG, "multiple of 4"), (dict(d=260), ARG, "multiple of 4"),
                         (dict(batch=0), ARG, "batch = 0"), (dict(ws="null"), WS, "workspace"),
                         (dict(ws="short"), WS, "workspace"), (dict(shift=4), ARG, "16-byte aligned"),
                         (dict(rows=10), ARG, "outside the frozen table"), (dict(rng=(-1, 3)), ARG, "outside the frozen table"),
                         (dict(table=False), ARG, "NULL table"), (dict(idp=False), ARG, "NULL id"),
                         (dict(reg=float("inf")), ARG, "finite")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and text in msg, (kw, got_rc, msg)
    rc = L.crh_deepmusic_f32(p(T), 11, p(ids32), 0, 10, p(G), 2, 4, 1e-4, 1.0, None, None, None, 0, None)
    assert rc == ARG and "nothing to compute" in L.crh_last_error().decode()
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match=r"deepmusic: width 6 must be a multiple of 4 in \[4, 256\]"):
        ops.deepmusic(z(11, 6), ids, z(2, 6), 1e-4)
    with pytest.raises(RuntimeError, match="deepmusic: ids lie outside the table"):
        ops.deepmusic(T[:int(ids.max())].contiguous(), ids, G, 1e-4)
    with pytest.raises(RuntimeError, match="one row per id"):
        ops.deepmusic(T, ids, z(3, 4), 1e-4)
    with pytest.raises(RuntimeError, match="integer tensor"):
        ops.deepmusic(T, ids.float(), G, 1e-4)
    with pytest.raises(RuntimeError, match="contiguous 2-D float32"):
        ops.deepmusic(T.double(), ids, G, 1e-4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.deepmusic(T.cpu(), ids.cpu(), G.cpu(), 1e-4)


def test_autograd_operator_matches_restatement_through_the_generator():
    """The trainer's autograd operator, fed by a small MLP, against the float64 autograd form through torch.autograd.grad
    with grad_out = 0.7: the MLP's parameters receive their gradients."""
    from coldrec_amd.model.DeepMusic import _FusedLoss
    g0 = torch.Generator().manual_seed(28)
    rows, B, d, reg = 90, 96, 32, 0.5
    T = torch.randn(rows, d, generator=g0) * 0.3
    ids = torch.randint(rows, (B,), generator=g0)
    content = torch.randn(rows, 12, generator=g0)
    torch.manual_seed(5)
    gen = dr.generator(12, d)

    def grads(dt, dev, fused):
        g = dr.generator(12, d).to(dt).to(dev)
        g.load_state_dict({k: v.to(dt) for k, v in gen.state_dict().items()})
        made = g(content.to(dt).to(dev)[ids.to(dev)])
        if fused:
            total, terms = _FusedLoss.apply(made, T.to(dev), ids.to(dev), reg, None)
            assert float(total.detach()) == float(terms[2])
        else:
            terms = dr.loss_terms(T.to(dt)[ids], made, reg)
            total = terms[2]
        got = torch.autograd.grad(total, list(g.parameters()), grad_outputs=torch.tensor(0.7, dtype=dt, device=dev))
        return np.array([float(t.detach()) for t in terms]), [x.double().cpu().numpy() for x in got]

    terms, got = grads(torch.float32, DEV, True)
    want_terms, want = grads(torch.float64, "cpu", False)
    rel = np.abs(terms - want_terms).max() / want_terms[2]
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    print(f"autograd: loss err / total {rel:.2e}, gradient err / max {errs}")
    # the float32 MLP and the kernel, each within its bar of the float64 value
    assert rel <= 2 * BARS[0] and max(errs) <= 2 * BARS[1]
    assert all(np.abs(a).max() > 0 for a in got) and want_terms[1] > 0.04 * want_terms[2]


# ---- whole runs against G27 --------------------------------------------------------------------------------------------

def _cfg(data, device=DEV, **kw):
    a = dict(dataset="toy", model="DeepMusic", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001, reg=0.0001,
             runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF", early_stop=10,
             eval_every=1)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def _run(where, cold, **kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle), with ``where`` --
    whose ./emb holds the fixture's loaded tables -- as the working directory."""
    import os
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    data = dr.toy_data(cold)
    cwd = os.getcwd()
    os.chdir(where)
    try:
        set_seed(2024, True)
        tr = AVAILABLE_MODELS["DeepMusic"](_cfg(data, cold_object=cold, **kw))
        tr.run()
    finally:
        os.chdir(cwd)
    return tr


@pytest.mark.parametrize("cold", ["item", "user"])
def test_run_matches_reference_g27(cold, tmp_path):
    """Bars: RUN_LOSS_BAR / RUN_TABLE_BAR above."""
    from tests.metaemb_restate import param_distances
    fx = load_golden(f"g27_deepmusic_{cold}.npz")
    write_loaded(fx, tmp_path, cold)
    tr = _run(tmp_path, cold)
    tables = [t.cpu().numpy() for t in (tr.user_emb, tr.item_emb)]
    assert tr.batch_losses.shape == (16, 3) and type(tr).LOSS_TERMS == ("mse", "reg", "batch_loss")
    rel, errs = run_distances(fx, tr.batch_losses, tables)
    perr = param_distances(fx, [p.detach().cpu().numpy() for p in tr.model.transformation.parameters()])
    print(f"DeepMusic {cold}: worst loss-term difference to G27 over the total {rel:.2e}; final tables differ by "
          f"{errs[0]:.2e} / {errs[1]:.2e} of their scale, the MLP's parameters by " + " / ".join(f"{e:.2e}" for e in perr))
    assert rel <= RUN_LOSS_BAR and max(errs) <= RUN_TABLE_BAR and max(perr) <= RUN_TABLE_BAR
    assert tr.epochs_ran == int(fx["epochs_ran"]) and tr.bestPerformance[0] == int(fx["best_epoch"])
    # the frozen side and every row outside the cold set: the backbone's bits
    frozen, made = (1, 0) if cold == "user" else (0, 1)
    loaded = (fx["loaded_U"], fx["loaded_V"])
    is_cold = np.zeros(tables[made].shape[0], bool)
    is_cold[np.asarray(tr.data.mapped_cold_user_idx if cold == "user" else tr.data.mapped_cold_item_idx)] = True
    assert np.array_equal(tables[frozen], loaded[frozen]) and np.array_equal(tables[made][~is_cold], loaded[made][~is_cold])
    assert is_cold.any() and not np.array_equal(tables[made][is_cold], loaded[made][is_cold])
    got_lists = {}
    for t in ("all", "cold", "warm"):
        c, _s, i = tr._topk_arrays(tr._sets("test", t), t)
        assert np.array_equal(c["users_int"].cpu().numpy(), fx[f"{t}_users_int"])
        got_lists[t] = i
    same, det, total = lists_vs_reference(fx, tables, got_lists, min_frac=0.5)
    print(f"DeepMusic {cold}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    results = dict(overall=tr.overall_test_results, cold=tr.cold_test_results, warm=tr.warm_test_results)
    metrics_vs_reference(results, fx, same == total, tr.bestPerformance[1]["NDCG"])
    lines = json.loads(str(fx["loss_lines"]))
    assert len(lines) == 2 and [float(l.split("batch_loss:")[1]) for l in lines] == pytest.approx(
        list(tr.batch_losses[[0, 8], 2]), rel=RUN_LOSS_BAR)


@pytest.mark.parametrize("cold", ["item", "user"])
def test_cli_trains_end_to_end(cold, tmp_path, monkeypatch):
    from coldrec_amd.main import main
    monkeypatch.chdir(tmp_path)
    common = ["--dataset", "toy", "--cold_object", cold, "--emb_size", "64", "--bs", "512", "--save_emb", "true",
              "--seed", "2024", "--data_root", str(tmp_path / "data"), "--result_dir", str(tmp_path / "result")]
    assert main(["--model", "MF", "--make_synthetic", "toy"] + common) is None
    main(["--model", "MF", "--epochs", "1"] + common)
    loaded = {s: torch.load(tmp_path / "emb" / f"toy_cold_{cold}_MF_{s}_emb.pt", map_location="cpu").detach()
              for s in ("user", "item")}
    pay = main(["--model", "DeepMusic", "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "DeepMusic" / "history.txt").is_file()
    out = {s: torch.load(tmp_path / "emb" / f"toy_cold_{cold}_DeepMusic_{s}_emb.pt", map_location="cpu")
           for s in ("user", "item")}
    frozen, made = ("item", "user") if cold == "user" else ("user", "item")
    assert torch.equal(out[frozen], loaded[frozen])
    assert out[made].shape == loaded[made].shape and torch.isfinite(out[made]).all() and not torch.equal(out[made], loaded[made])
