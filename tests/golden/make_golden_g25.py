"""Generate G25 under tests/golden/ by RUNNING THE REFERENCE's MTPR.run() (model/MTPR.py:14-54 through
model/BaseRecommender.py), once per cold object.

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g25.py

g25_mtpr_item.npz   the toy item-cold split (make_dataset("toy", "item", seed=1)), d = 64, bs = 512, 2 epochs.
g25_mtpr_user.npz   the toy user-cold split of the same data seed, make_dataset("toy", "user", seed=1), same settings.
    set_seed(2024), then the trainer on a fresh builder, p_emb / p_ctx / p_proj at their defaults, everything on the
    CPU (so the learner draws its five tensors from the CPU generator).
    Observed from outside: the learner's four bpr_loss_* and regs are wrapped to record what they return, and
    Tensor.backward to close a step: per step [L_i, L_f, L_if, L_fi, regs, batch_loss].
    Stored: data only -- the five initial tensors, the per-step terms, the five trained tensors, the final (best-epoch)
    user_emb / item_emb, the three settings' test metrics and top-20 lists, the ``training:`` lines, the settings.
    Regenerates byte for byte.
"""
import contextlib
import importlib
import io
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports it in place)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coldrec_amd.data.synth import make_dataset  # noqa: E402  (ours: input generator only)

SETTINGS = dict(model="MTPR", emb_size=64, epochs=2, bs=512, p_emb=[0.05, 0.0], p_ctx=[0.05, 0.01], p_proj=[0.05, 0.01])
TERMS = ("bpr_loss_i", "bpr_loss_f", "bpr_loss_if", "bpr_loss_fi", "regs")
TENSORS = ("P", "Q", "W", "weu", "wei")


def _tensors(learner):
    t = (learner.P.weight, learner.Q.weight, learner.W, learner.weu, learner.wei)
    return {k: v.detach().cpu().numpy().copy() for k, v in zip(TENSORS, t)}


def g25(cold):
    split = make_dataset("toy", cold, seed=1)
    mod = importlib.import_module("model.MTPR")
    data = mg.ref_builder(split)
    cfg = mg.ref_config(data, cold_object=cold, **SETTINGS)
    mg.set_seed(2024, False)
    trainer = mod.MTPR(cfg)
    learner = trainer.model
    first = _tensors(learner)

    steps, current = [], {}
    for name in TERMS:
        def wrapped(*args, _real=getattr(learner, name), _name=name, **kw):
            out = _real(*args, **kw)
            current[_name] = float(out.item())
            return out
        setattr(learner, name, wrapped)
    real_backward = torch.Tensor.backward

    def backward_spy(self, *args, **kw):
        steps.append([current[k] for k in TERMS] + [float(self.item())])
        current.clear()
        return real_backward(self, *args, **kw)

    torch.Tensor.backward = backward_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        torch.Tensor.backward = real_backward
    lists = mg._final_lists(trainer, data)
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    terms = np.array(steps, np.float64)
    last = _tensors(learner)
    a = cfg.args
    user, item = trainer.user_emb.detach().numpy(), trainer.item_emb.detach().numpy()
    for t in (user, item, terms) + tuple(last.values()):
        assert np.isfinite(t).all()
    res = dict(
        which="MTPR", cold_object=cold, d=a.emb_size, epochs=a.epochs, batch_size=a.bs, p_emb=np.array(a.p_emb, np.float64),
        p_ctx=np.array(a.p_ctx, np.float64), p_proj=np.array(a.p_proj, np.float64), seed=2024, data_seed=1,
        user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data), n_steps=terms.shape[0],
        terms=terms, user_emb=user, item_emb=item,
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **lists)
    res.update({"init_" + k: v for k, v in first.items()})
    res.update({"trained_" + k: v for k, v in last.items()})
    np.savez_compressed(os.path.join(HERE, f"g25_mtpr_{cold}.npz"), **res)
    print("g25 MTPR %s: %d steps; last terms %s; best %s" % (cold, terms.shape[0], terms[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g25("item")
    g25("user")
