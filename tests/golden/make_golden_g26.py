"""Generate G26 under tests/golden/ by RUNNING THE REFERENCE: MF.run() (the backbone, saved with save_emb), then
VBPR.run() (model/VBPR.py, saved with save_emb) and, for cold items, AMR.run() (model/AMR.py) from VBPR's saved files.

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g26.py

g26_vbpr_item.npz / g26_amr_item.npz   the toy item-cold split (make_dataset("toy", "item", seed=1)), d = 64, bs = 512.
g26_vbpr_user.npz                      the toy user-cold split of the same data seed (the reference's AMR cannot train cold
    users: predict_adv indexes the users' noise with item ids, model/AMR.py:148).
    Backbone: MF, 3 epochs, set_seed(2024), on a builder of its own, inside a temporary working directory (./emb).
    VBPR and AMR each on a FRESH builder (the sampler shuffles the training pairs in place), set_seed(2024), 2 epochs,
    p_emb = [0.05, 0.01] (the default weight decay 0 would leave R_emb untested), p_ctx, eps, lmd at their defaults,
    everything on the CPU.
    Observed from outside: the model file's ``F`` is replaced by a pass-through that records the sum of every softplus
    (per step VBPR: one; AMR: the plain term before the noise, the plain term, the adversarial term), the learner's
    regs is wrapped, and Tensor.backward closes a step; after every backward of AMR the Frobenius norm of
    item_content.grad (the noise) is read.
    The trainer's save() is wrapped to copy P, Q, PQ2 and W when the best epoch is saved: the reference's own best_*
    of those four are the live parameters (forward() returns them as they are), so after a run whose best epoch is not
    its last they hold the last epoch's values beside the best epoch's content rows.  After run() the five tensors are
    set to the best epoch's copies and the reference's three test passes are run again: the stored metrics and lists
    are the reference's evaluation of the best epoch's model.
    Stored: data only -- the loaded tensors, the initial PQ2 and W, the per-step terms, the trained P, Q, PQ2, W, the
    best epoch's four where they differ from the trained ones (the five tensors and the ranked pair [main | aux] follow
    from them: aux = content @ W), the three settings' test metrics and top-20 lists, the ``training:`` lines, the
    settings.  A file stays below 1 MiB.  Regenerates byte for byte.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports it in place)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as real_F  # noqa: E402

from coldrec_amd.data.synth import make_dataset  # noqa: E402  (ours: input generator only)

BACKBONE = dict(model="MF", emb_size=64, epochs=3, bs=512, save_emb=True)
COMMON = dict(emb_size=64, epochs=2, bs=512, backbone="MF", save_emb=True, p_emb=[0.05, 0.01], p_ctx=[0.05, 0.01])
FIVE = ("user_emb_main", "item_emb_main", "user_emb_aux", "item_emb_aux", "w_value")
FILES = ("user_emb_main_P", "item_emb_main_Q", "user_emb_aux", "item_emb_aux", "W")


def _np(t):
    return t.detach().cpu().numpy().copy()


def _observed_run(which, cold, split, **settings):
    """One reference run in the current directory; returns the fixture's dict."""
    mod = importlib.import_module("model." + which)
    data = mg.ref_builder(split)
    cfg = mg.ref_config(data, model=which, cold_object=cold, **settings)
    mg.set_seed(2024, False)
    trainer = getattr(mod, which)(cfg)
    learner = trainer.model
    four = lambda: dict(P=_np(learner.P.weight), Q=_np(learner.Q.weight), PQ2=_np(learner.PQ2.weight), W=_np(learner.W))
    first, best = four(), {}
    real_save = trainer.save

    def save():
        real_save()
        best.clear()
        best.update(four())

    trainer.save = save

    sums, steps, norms, current = [], [], [], {}

    def softplus(x, *a, **kw):
        out = real_F.softplus(x, *a, **kw)
        sums.append(float(torch.sum(out).item()))
        return out

    real_regs = learner.regs

    def regs(*a, **kw):
        out = real_regs(*a, **kw)
        current["regs"] = float(out.item())
        return out

    learner.regs = regs
    mod.F = types.SimpleNamespace(softplus=softplus, normalize=real_F.normalize)
    real_backward = torch.Tensor.backward
    amr = which == "AMR"

    def backward_spy(self, *args, **kw):
        closing = "regs" in current
        if closing:
            if amr:
                assert len(sums) == 3 and sums[0] == sums[1]
                steps.append([sums[1], float(cfg.args.lmd) * sums[2], current["regs"], float(self.item())])
            else:
                assert len(sums) == 1
                steps.append([sums[0], current["regs"], float(self.item())])
            sums.clear()
            current.clear()
        out = real_backward(self, *args, **kw)
        if amr:
            norms.append(float(torch.linalg.norm(learner.item_content.grad).item()))
        return out

    torch.Tensor.backward = backward_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        torch.Tensor.backward = real_backward
        mod.F = real_F
    last = four()
    # the best epoch's model through the reference's own evaluation
    content = learner.user_content if cold == "user" else learner.item_content
    aux = torch.mm(content.detach(), torch.from_numpy(best["W"]))
    assert np.array_equal(_np(aux), _np(trainer.user_emb_aux if cold == "user" else trainer.item_emb_aux))
    t = {k: torch.from_numpy(v) for k, v in best.items()}
    trainer.user_emb_main, trainer.item_emb_main, trainer.w_value = t["P"], t["Q"], t["W"]
    trainer.user_emb_aux, trainer.item_emb_aux = (aux, t["PQ2"]) if cold == "user" else (t["PQ2"], aux)
    with contextlib.redirect_stdout(io.StringIO()):
        for kind in ("all", "cold", "warm"):
            trainer.full_evaluation(trainer.test(test_type=kind), test_type=kind)
    lists = mg._final_lists(trainer, data)
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    terms = np.array(steps, np.float64)
    for t in (terms,) + tuple(last.values()) + tuple(best.values()):
        assert np.isfinite(t).all()
    best_is_last = all(np.array_equal(best[k], last[k]) for k in last)
    assert best_is_last == (trainer.bestPerformance[0] == trainer.epochs_ran)
    a = cfg.args
    res = dict(
        which=which, cold_object=cold, d=a.emb_size, epochs=a.epochs, batch_size=a.bs, p_emb=np.array(a.p_emb, np.float64),
        p_ctx=np.array(a.p_ctx, np.float64), seed=2024, data_seed=1, user_num=data.user_num, item_num=data.item_num,
        n_train=len(data.training_data), n_steps=terms.shape[0], terms=terms, best_is_last=best_is_last,
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **lists)
    res.update({"trained_" + k: v for k, v in last.items()})
    if not best_is_last:
        res.update({"best_" + k: v for k, v in best.items()})
    if not amr:                     # (AMR starts from the loaded tensors; VBPR's P and Q are the loaded tables)
        res.update(init_PQ2=first["PQ2"], init_W=first["W"])
    if amr:
        res.update(eps=float(a.eps), lmd=float(a.lmd), noise_norms=np.array(norms, np.float64))
        assert len(norms) == 2 * terms.shape[0]
    print("g26 %s %s: %d steps; last terms %s; best %s" % (which, cold, terms.shape[0], terms[-1], trainer.bestPerformance))
    return res


def g26(cold):
    split = make_dataset("toy", cold, seed=1)
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("emb")
            mg.set_seed(2024, False)
            mg._run_quiet(mg.MF(mg.ref_config(mg.ref_builder(split), cold_object=cold, **BACKBONE)))
            stem = f"./emb/toy_cold_{cold}_"
            loaded = [_np(torch.load(f"{stem}MF_{s}_emb.pt", map_location="cpu")) for s in ("user", "item")]
            res = _observed_run("VBPR", cold, split, **COMMON)
            res.update(loaded_U=loaded[0], loaded_V=loaded[1])
            np.savez_compressed(os.path.join(HERE, f"g26_vbpr_{cold}.npz"), **res)
            if cold == "item":
                # (what AMR loads; item_emb_aux, which it reads and ignores, is not stored)
                saved = {k: _np(torch.load(f"{stem}VBPR_{f}.pt", map_location="cpu")) for k, f in zip(FIVE, FILES)}
                res = _observed_run("AMR", cold, split, eps=0.1, lmd=1, **COMMON)
                res.update({"loaded_" + k: v for k, v in saved.items() if k != "item_emb_aux"})
                np.savez_compressed(os.path.join(HERE, f"g26_amr_{cold}.npz"), **res)
        finally:
            os.chdir(cwd)


if __name__ == "__main__":
    g26("item")
    g26("user")
