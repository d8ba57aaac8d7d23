"""GPU: the fused MetaEmbedding loss (csrc/metaemb.hip) against the float64 closed form (tests/metaemb_restate.py, itself
pinned to the autograd form and to the reference's runs by tests/test_metaemb.py): the shapes where it can go wrong, its
edges, its determinism contract, the argument errors, the trainer's autograd operator, and whole runs against G27.

Bars of the kernel against the float64 closed form: 8x the worst distance of the float32 torch formula (the reference's
way, autograd and autograd.grad, on the CPU) from the float64 one at the same cases.  Loss terms are measured as error
over the TOTAL loss (ME), gradients as error over their maximum, the 2 N scores as error over the largest score.  The
cases run at cold_lr = N / 4, where the inner step moves a score by (s(y_a) - t) |o|^2 / 4 -- the order of the score
itself -- so a kernel that ignored the inner step misses loss_b by 0.02 .. 1.0 of the total.  Measured on the CPU on one
thread (tests/test_metaemb.py prints them again and holds them to a factor of 2):
    cases:  loss terms 2.17e-7 (N300-d256), gradients 2.00e-7 (N300-d256), scores 2.01e-7 (N65-d252)
            -> LOSS_BAR = 1.74e-6, GRAD_BAR = 1.60e-6, SCORE_BAR = 1.61e-6
    edges:  loss terms 1.14e-7 (alpha 0), gradients 9.51e-7 (scores beyond +-90, where a dot product's rounding decides how
            much of a saturated slope is left), scores 1.70e-7 (step of order 10)
            (the edge bars are 8x these or the cases' bars, whichever is larger)
On the MI355X the kernel measures 2.13e-7 (loss terms, N65-d252), 1.43e-7 (gradients, N63-d64) and 2.00e-7 (scores,
N300-d256) at worst over the cases; 3.98e-7 (step of order 10), 4.29e-7 (scores beyond +-90) and 1.43e-7 over the edges.

Whole runs against G27: plain float32 torch on the CPU, the reference's way (tests/test_metaemb.py), ends 8.60e-8 (item) /
8.59e-8 (user) of the total from G27's loss terms, 1.32e-7 / 1.30e-7 of the published table's scale from its cold rows
and 1.26e-7 / 2.60e-7 from the trained generator's parameters.  8x those stay below the project's run bars, 1e-5 and 2e-4,
which are therefore the bars.  The high-lr fixture (lr = 0.25, bs = 4: the inner step moves a score by 1.1e-3 on average,
|loss_b - loss_a| reaches 7.9e-4 of losses between 0.7 and 1.5) is reproduced bit for bit by float32 torch on the CPU that made the fixture;
loss_b - loss_a is compared as a quantity of its own at the loss bar, 1e-5 of the total: a kernel without the inner step
misses it more than twentyfold.
On the MI355X the runs end 8.61e-8 (item) / 8.61e-8 (user) of the total from G27's loss terms, 4.29e-7 / 1.30e-7 of the
published table's scale from its tables and 2.59e-6 / 2.60e-7 from the generator's parameters; every one of the 750 / 456
final lists equals the reference's (739 / 451 users with a determined ranking).  The high-lr run ends 4.01e-7 of the total
from G27's loss terms and 3.77e-7 from its loss_b - loss_a (which reaches 4.86e-4 of the total), 3.35e-7 from the item
table and 4.29e-7 from the parameters.
"""
import argparse
import json
import types

import numpy as np
import pytest
import torch

from tests import metaemb_restate as mr
from tests.conftest import load_golden
from tests.test_gar_gpu import lists_vs_reference, metrics_vs_reference, run_distances, write_loaded

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

F32_WORST = (2.17e-7, 2.00e-7, 2.01e-7)         # float32 torch against the float64 closed form at the cases: loss, gradient, scores
BARS = tuple(8 * w for w in F32_WORST)
EDGE_F32_WORST = (1.14e-7, 9.51e-7, 1.70e-7)    # ... at the edge cases
EDGE_BARS = tuple(max(8 * e, b) for e, b in zip(EDGE_F32_WORST, BARS))
RUN_LOSS_BAR, RUN_TABLE_BAR = 1e-5, 2e-4        # the project's run bars (see above)
F32_RUN_LOSS = dict(item=8.60e-8, user=8.59e-8, hi=0.0)          # float32 torch against G27, measured
F32_RUN_TABLES = dict(item=(0.0, 1.32e-7), user=(1.30e-7, 0.0), hi=(0.0, 0.0))
F32_RUN_PARAMS = dict(item=1.26e-7, user=2.60e-7, hi=0.0)
HI = dict(epochs=1, bs=4, lr=0.25)              # tests/golden/make_golden_g27.py's HI


def _fused(inp, n_pos, alpha, cold_lr, **kw):
    from coldrec_amd import ops
    T, ids, E = (t.to(DEV) for t in inp)
    kw.setdefault("want_scores", True)
    loss, grad, scores = ops.metaemb(T, ids, E, n_pos, alpha, cold_lr, **kw)
    torch.cuda.synchronize()
    return loss.cpu(), grad, scores


def _compare(tag, got, want, bars=BARS):
    got = (got[0].numpy(), got[1].cpu().numpy(), got[2].cpu().numpy())
    assert all(np.isfinite(g).all() for g in got)
    dist = mr.distances(got, want)
    print(f"{tag}: loss err / total {dist[0]:.2e}, gradient err / max {dist[1]:.2e}, score err / max {dist[2]:.2e}")
    assert dist[0] <= bars[0]
    assert dist[1] <= bars[1]
    assert dist[2] <= bars[2]
    return got


@pytest.mark.parametrize("run", mr.case_runs(), ids=lambda r: r[0])
def test_kernel_matches_float64_closed_form(run):
    tag, inp, n_pos, alpha, cold_lr = run
    want = mr.closed_form(*inp, n_pos, alpha, cold_lr)
    _compare(tag, _fused(inp, n_pos, alpha, cold_lr), want)
    assert abs(want[0][1] - want[0][0]) > 0.02 * want[0][2]          # the inner step is visible in loss_b


@pytest.mark.parametrize("edge", mr.edge_cases(), ids=lambda e: e[0])
def test_edges(edge):
    tag, inp, n_pos, alpha, cold_lr = edge
    want = mr.closed_form(*inp, n_pos, alpha, cold_lr)
    loss, grad, scores = _compare(tag, _fused(inp, n_pos, alpha, cold_lr), want, EDGE_BARS)
    if tag == "alpha0":
        assert loss[2] == loss[1] != loss[0]
    if tag == "alpha1":
        assert loss[2] == loss[0] != loss[1]
    if tag == "coldlr0":                          # no inner step: the second pass repeats the first bit for bit
        assert loss[1] == loss[0] == loss[2] and np.array_equal(scores[0], scores[1])
    if tag.startswith("step-order"):              # the inner step turns scores over
        assert (np.sign(scores[0]) != np.sign(scores[1])).sum() >= 10
    if tag.startswith("scores-beyond"):           # saturated: finite, and what is left of a slope keeps its sign
        top = 30 if tag.endswith("30") else 90
        assert scores.max() > top and scores.min() < -top
        # sigmoid(y) - t has the sign of 0.5 - t whatever y is (float64's own sigmoid(y) - 1 rounds to 0 from y = 37 on)
        sign = np.where(np.arange(len(inp[1])) < n_pos, -1.0, 1.0)[:, None] * np.sign(inp[0][inp[1]].numpy())
        nz = grad != 0
        assert nz.mean() > 0.25 and np.array_equal(np.sign(grad[nz]), sign[nz])
    if tag == "emb-zero":
        assert not scores[0].any() and scores[1].any() and loss[0] == pytest.approx(np.log(2), rel=1e-6)
    if tag == "first-and-last-rows":
        assert {0, 49} <= set(inp[1].tolist())
    if tag == "ids-equal":
        assert len(set(inp[1].tolist())) == 1


@pytest.mark.parametrize("run", [mr.case_runs()[3], mr.case_runs()[7]], ids=lambda r: r[0])
def test_determinism_scale_and_outputs_not_asked_for(run):
    from coldrec_amd import _lib, ops
    tag, inp, n_pos, alpha, cold_lr = run
    a, b = _fused(inp, n_pos, alpha, cold_lr), _fused(inp, n_pos, alpha, cold_lr)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    half = _fused(inp, n_pos, alpha, cold_lr, scale=0.5)
    assert torch.equal(half[0], a[0]) and torch.equal(half[1], a[1] * 0.5) and torch.equal(half[2], a[2])
    no_grad = _fused(inp, n_pos, alpha, cold_lr, want_grad=False)
    assert no_grad[1] is None and torch.equal(no_grad[0], a[0]) and torch.equal(no_grad[2], a[2])
    no_scores = _fused(inp, n_pos, alpha, cold_lr, want_scores=False)
    assert no_scores[2] is None and torch.equal(no_scores[0], a[0]) and torch.equal(no_scores[1], a[1])
    # through the C ABI: a NULL output is not written, the others keep their bits
    T, ids, E = (t.to(DEV).contiguous() for t in inp)
    ids = ids.to(torch.int32)
    N, d = E.shape
    ws = ops.metaemb_workspace(N, d, DEV)
    for skip in range(3):
        out = [torch.full((N, d), -7.0, device=DEV), torch.full((3,), -7.0, device=DEV), torch.full((2, N), -7.0, device=DEV)]
        ptrs = [None if k == skip else t.data_ptr() for k, t in enumerate(out)]
        rc = _lib.lib().crh_metaemb_f32(T.data_ptr(), T.shape[0], ids.data_ptr(), 0, T.shape[0] - 1, E.data_ptr(), N, n_pos, d,
                                        alpha, cold_lr, 1.0, *ptrs, ws.data_ptr(), ws.numel(), _lib.current_stream())
        torch.cuda.synchronize()
        assert rc == 0
        for k, (t, ref) in enumerate(zip(out, (a[1], a[0].to(DEV), a[2]))):
            assert (t == -7.0).all() if k == skip else torch.equal(t, ref)


def test_argument_errors_launch_nothing():
    from coldrec_amd import _lib, ops
    T, ids, E = (t.to(DEV).contiguous() for t in mr.inputs((2, 4, 11)))
    ids32 = ids.to(torch.int32)
    L = _lib.lib()
    p = lambda t: t.data_ptr()

    def call(d=4, n=2, n_pos=1, ws="ok", rows=11, rng=(0, 10), shift=0, table=True, idp=True, alpha=0.5):
        space = ops.metaemb_workspace(2, 4, DEV)
        out = [torch.full((2, 4), -7.0, device=DEV), torch.full((3,), -7.0, device=DEV), torch.full((2, 2), -7.0, device=DEV)]
        ws_ptr, ws_bytes = {"ok": (p(space), space.numel()), "null": (0, space.numel()), "short": (p(space), 16)}[ws]
        rc = L.crh_metaemb_f32(p(T) if table else None, rows, p(ids32) if idp else None, rng[0], rng[1], p(E) + shift, n, n_pos,
                               d, alpha, 1e-4, 1.0, p(out[0]), p(out[1]), p(out[2]), ws_ptr, ws_bytes, _lib.current_stream())
        torch.cuda.synchronize()
        assert all((t == -7.0).all() for t in out)                     # nothing ran
        return rc, L.crh_last_error().decode()

    ARG, WS = -1, -3                                                   # CRH_ERR_ARG, CRH_ERR_WS of include/coldrec_hip.h
    for kw, rc, text in ((dict(d=6), ARG, "multiple of 4"), (dict(d=260), ARG, "multiple of 4"), (dict(n=0), ARG, "n = 0"),
                         (dict(n_pos=3), ARG, "n_pos = 3"), (dict(n_pos=-1), ARG, "n_pos = -1"),
                         (dict(ws="null"), WS, "workspace"), (dict(ws="short"), WS, "workspace"),
                         (dict(shift=4), ARG, "16-byte aligned"), (dict(rows=10), ARG, "outside the frozen table"),
                         (dict(rng=(-1, 3)), ARG, "outside the frozen table"), (dict(table=False), ARG, "NULL table"),
                         (dict(idp=False), ARG, "NULL id"), (dict(alpha=float("nan")), ARG, "finite")):
        got_rc, msg = call(**kw)
        assert got_rc == rc and text in msg, (kw, got_rc, msg)
    rc = L.crh_metaemb_f32(p(T), 11, p(ids32), 0, 10, p(E), 2, 1, 4, 0.5, 1e-4, 1.0, None, None, None, None, 0, None)
    assert rc == ARG and "nothing to compute" in L.crh_last_error().decode()
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(RuntimeError, match=r"metaemb: width 6 must be a multiple of 4 in \[4, 256\]"):
        ops.metaemb(z(11, 6), ids, z(2, 6), 1, 0.5, 1e-4)
    with pytest.raises(RuntimeError, match="metaemb: ids lie outside the table"):
        ops.metaemb(T[:int(ids.max())].contiguous(), ids, E, 1, 0.5, 1e-4)
    with pytest.raises(RuntimeError, match="metaemb: ids lie outside the table"):
        ops.metaemb(T, ids, E, 1, 0.5, 1e-4, id_range=(-1, 3))
    with pytest.raises(RuntimeError, match=r"n_pos = 3 out of \[0, 2\]"):
        ops.metaemb(T, ids, E, 3, 0.5, 1e-4)
    with pytest.raises(RuntimeError, match="one row per id"):
        ops.metaemb(T, ids, z(3, 4), 1, 0.5, 1e-4)
    with pytest.raises(RuntimeError, match="integer tensor"):
        ops.metaemb(T, ids.float(), E, 1, 0.5, 1e-4)
    with pytest.raises(RuntimeError, match="contiguous 2-D float32"):
        ops.metaemb(T.double(), ids, E, 1, 0.5, 1e-4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.metaemb(T.cpu(), ids.cpu(), E.cpu(), 1, 0.5, 1e-4)


@pytest.mark.parametrize("cold_user", [False, True], ids=["item", "user"])
def test_autograd_operator_matches_restatement_through_the_generator(cold_user):
    """The trainer's autograd operator, fed by a small generator, against the float64 autograd form through
    torch.autograd.grad with grad_out = 0.7: the generator's parameters receive their gradients."""
    from coldrec_amd.model.MetaEmbedding import _FusedLoss
    g0 = torch.Generator().manual_seed(27)
    nu, ni, B, d, alpha = 40, 90, 96, 32, 0.3
    cold_lr = 2 * B / 4.
    U, V = torch.randn(nu, d, generator=g0) * 0.3, torch.randn(ni, d, generator=g0) * 0.3
    users, pos, neg = (torch.randint(n, (B,), generator=g0) for n in (nu, ni, ni))
    content = torch.randn(nu if cold_user else ni, 12, generator=g0)
    uu, ii = torch.cat([users, users]), torch.cat([pos, neg])
    table, ids, own = (V, ii, uu) if cold_user else (U, uu, ii)
    torch.manual_seed(5)
    gen = mr.generator(12, d)

    def grads(dt, dev, fused):
        g = mr.generator(12, d).to(dt).to(dev)
        g.load_state_dict({k: v.to(dt) for k, v in gen.state_dict().items()})
        E = g(content.to(dt).to(dev)[own.to(dev)]) / 5.
        if fused:
            total, terms = _FusedLoss.apply(E, table.to(dev), ids.to(dev), B, alpha, cold_lr, None)
            assert float(total.detach()) == float(terms[2])
        else:
            terms = mr.loss_terms(table.to(dt)[ids], E, B, alpha, cold_lr)[:3]
            total = terms[2]
        got = torch.autograd.grad(total, list(g.parameters()), grad_outputs=torch.tensor(0.7, dtype=dt, device=dev))
        return np.array([float(t.detach()) for t in terms]), [x.double().cpu().numpy() for x in got]

    terms, got = grads(torch.float32, DEV, True)
    want_terms, want = grads(torch.float64, "cpu", False)
    rel = np.abs(terms - want_terms).max() / want_terms[2]
    errs = [float(np.abs(a - b).max() / np.abs(b).max()) for a, b in zip(got, want)]
    print(f"autograd: loss err / total {rel:.2e}, gradient err / max {errs}")
    # the float32 generator and the kernel, each within its bar of the float64 value
    assert rel <= 2 * BARS[0] and max(errs) <= 2 * BARS[1]
    assert all(np.abs(a).max() > 0 for a in got) and abs(want_terms[1] - want_terms[0]) > 0.02 * want_terms[2]


# ---- whole runs against G27 --------------------------------------------------------------------------------------------

def _cfg(data, device=DEV, **kw):
    a = dict(dataset="toy", model="MetaEmbedding", epochs=2, layers=2, topN="10,20", bs=512, emb_size=64, lr=0.001,
             reg=0.0001, runs=1, seed=2024, use_gpu=True, save_emb=False, gpu_id=0, cold_object="item", backbone="MF",
             early_stop=10, eval_every=1, alpha=0.5)
    a.update(kw)
    return types.SimpleNamespace(args=argparse.Namespace(**a), data=data, device=torch.device(device))


def _run(where, cold, **kw):
    """A whole run on a FRESH builder (the sampler keeps the reference's cumulative in-place shuffle), with ``where`` --
    whose ./emb holds the fixture's loaded tables -- as the working directory."""
    import os
    from coldrec_amd.model import AVAILABLE_MODELS
    from coldrec_amd.util.utils import set_seed
    data = mr.toy_data(cold)
    cwd = os.getcwd()
    os.chdir(where)
    try:
        set_seed(2024, True)
        tr = AVAILABLE_MODELS["MetaEmbedding"](_cfg(data, cold_object=cold, **kw))
        tr.run()
    finally:
        os.chdir(cwd)
    return tr


def _params(tr):
    return [p.detach().cpu().numpy() for p in tr.model.emb_pred_Dense.parameters()]


@pytest.mark.parametrize("cold", ["item", "user"])
def test_run_matches_reference_g27(cold, tmp_path):
    """Bars: RUN_LOSS_BAR / RUN_TABLE_BAR above."""
    fx = load_golden(f"g27_metaemb_{cold}.npz")
    write_loaded(fx, tmp_path, cold)
    tr = _run(tmp_path, cold)
    tables = [t.cpu().numpy() for t in (tr.user_emb, tr.item_emb)]
    assert tr.batch_losses.shape == (16, 3) and type(tr).LOSS_TERMS == ("loss_a", "loss_b", "batch_loss")
    rel, errs = run_distances(fx, tr.batch_losses, tables)
    perr = mr.param_distances(fx, _params(tr))
    print(f"MetaEmbedding {cold}: worst loss-term difference to G27 over the total {rel:.2e}; final tables differ by "
          f"{errs[0]:.2e} / {errs[1]:.2e} of their scale, the generator's parameters by {perr[0]:.2e} / {perr[1]:.2e}")
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
    print(f"MetaEmbedding {cold}: {same} of {total} final lists identical to the reference's ({det} with a determined ranking)")
    results = dict(overall=tr.overall_test_results, cold=tr.cold_test_results, warm=tr.warm_test_results)
    metrics_vs_reference(results, fx, same == total, tr.bestPerformance[1]["NDCG"])
    lines = json.loads(str(fx["loss_lines"]))
    assert len(lines) == 2 and [float(l.split("batch_loss:")[1]) for l in lines] == pytest.approx(
        list(tr.batch_losses[[0, 8], 2]), rel=RUN_LOSS_BAR)


def test_high_lr_run_keeps_the_inner_step():
    """G27's high-lr run, where loss_b - loss_a is far above float32 resolution: compared as a quantity of its own."""
    import tempfile
    from pathlib import Path
    fx, base = load_golden("g27_metaemb_item_hi.npz"), load_golden("g27_metaemb_item.npz")
    assert (int(fx["epochs"]), int(fx["batch_size"]), float(fx["lr"])) == (HI["epochs"], HI["bs"], HI["lr"])
    with tempfile.TemporaryDirectory() as tmp:
        write_loaded(base, Path(tmp), "item")
        tr = _run(tmp, "item", **HI)
    want, got = fx["losses"], tr.batch_losses
    assert got.shape == want.shape == (905, 3)
    rel = (np.abs(got - want) / want[:, 2:3]).max()
    gap = (np.abs((got[:, 1] - got[:, 0]) - (want[:, 1] - want[:, 0])) / want[:, 2]).max()
    scale = (np.abs(want[:, 1] - want[:, 0]) / want[:, 2]).max()
    item = tr.item_emb.cpu().numpy()
    err = float(np.abs(item - fx["item_emb"]).max() / np.abs(fx["item_emb"]).max())
    perr = mr.param_distances(fx, _params(tr))
    print(f"MetaEmbedding high lr: loss terms differ from G27 by {rel:.2e} of the total, loss_b - loss_a by {gap:.2e} of the "
          f"total (it reaches {scale:.2e}); item table {err:.2e}, parameters {perr[0]:.2e} / {perr[1]:.2e}")
    assert rel <= RUN_LOSS_BAR and gap <= RUN_LOSS_BAR and scale >= 20 * RUN_LOSS_BAR
    assert err <= RUN_TABLE_BAR and max(perr) <= RUN_TABLE_BAR


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
    pay = main(["--model", "MetaEmbedding", "--epochs", "2"] + common)
    assert set(pay) == {"10", "20"} and (tmp_path / "result" / "MetaEmbedding" / "history.txt").is_file()
    out = {s: torch.load(tmp_path / "emb" / f"toy_cold_{cold}_MetaEmbedding_{s}_emb.pt", map_location="cpu")
           for s in ("user", "item")}
    frozen, made = ("item", "user") if cold == "user" else ("user", "item")
    assert torch.equal(out[frozen], loaded[frozen])
    assert out[made].shape == loaded[made].shape and torch.isfinite(out[made]).all() and not torch.equal(out[made], loaded[made])
