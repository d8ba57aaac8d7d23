"""Generate G28 under tests/golden/ by RUNNING THE REFERENCE's DUIF.run() (model/DUIF.py), once per cold object.

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g28.py

g28_duif_{item,user}.npz
    The toy splits of data seed 1, make_dataset("toy", cold, seed=1) (tests/gar_restate.py toy_data builds them), d = 64,
    bs = 512, epochs = 2, set_seed(2024), the reference's defaults lr = 0.001 and reg = 0.0001, everything on the CPU.  DUIF
    loads no backbone.
    Observed from outside: the reference forms the loss inline in train(), so Tensor.backward is wrapped and reads the
    calling frame of every step: the frame holds user_emb, pos_item_emb and neg_item_emb, from which the two terms are
    formed with the reference's own bpr_loss and l2_reg_loss, [bpr, reg, batch_loss].
    The trainer's save() is wrapped to copy the three parameters when the best epoch is saved: the reference's own best_*
    of the free table (the side without content) is the live parameter (forward() returns it as it is), so after a run
    whose best epoch is not its last it holds the last epoch's values beside the best epoch's projected table (asserted
    below).  After run() the two tables are set to the best epoch's copies and the reference's three test passes are run
    again: the stored metrics and lists are the reference's evaluation of the best epoch's model.
    Stored: data only -- the three parameters before the run in named_parameters() order (init_k) and those the run
    trained after it (trained_k: the cold side's table is drawn and never trained), the best epoch's (best_k) where the
    best epoch is not the last, the best epoch's projected table as the reference computed it (best_proj), the per-step
    terms, the three settings' test metrics and top-20 lists, the ``training:`` lines, the settings.  The reference's
    final pair is (trained free table, best_proj); the best epoch's pair is (best free table, best_proj).
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

SETTINGS = dict(model="DUIF", emb_size=64, epochs=2, bs=512)


def _np(t):
    return t.detach().cpu().numpy().copy()


def g28(cold):
    from util.utils import bpr_loss, l2_reg_loss
    mod = importlib.import_module("model.DUIF")
    data = mg.ref_builder(make_dataset("toy", cold, seed=1))
    cfg = mg.ref_config(data, cold_object=cold, **SETTINGS)
    mg.set_seed(2024, False)
    trainer = mod.DUIF(cfg)
    names = [n for n, _ in trainer.model.named_parameters()]
    params = lambda: [_np(p) for _, p in trainer.model.named_parameters()]
    init, best = params(), []
    real_save = trainer.save

    def save():
        real_save()
        best[:] = params()

    trainer.save = save
    terms = []
    real_backward = torch.Tensor.backward

    def backward_spy(self, *args, **kw):
        f = sys._getframe(1).f_locals
        assert f["batch_loss"] is self
        three = (f["user_emb"], f["pos_item_emb"], f["neg_item_emb"])
        with torch.no_grad():
            terms.append([float(bpr_loss(*three)), float(l2_reg_loss(f["self"].reg, *three)), float(self.item())])
        return real_backward(self, *args, **kw)

    torch.Tensor.backward = backward_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        torch.Tensor.backward = real_backward
    last = params()
    free, proj = (1, 0) if cold == "user" else (0, 1)               # the free and the projected side of (user, item)
    moved = [k for k in range(3) if not np.array_equal(init[k], last[k])]
    k_free = names.index("embedding_dict." + ("item_emb" if cold == "user" else "user_emb"))
    k_w = names.index(("user" if cold == "user" else "item") + "_projector.weight")
    assert moved == sorted([k_free, k_w]), moved                     # the cold side's table is never trained
    published = [_np(trainer.user_emb), _np(trainer.item_emb)]
    best_is_last = all(np.array_equal(b, t) for b, t in zip(best, last))
    assert best_is_last == (trainer.bestPerformance[0] == trainer.epochs_ran)
    # the aliasing: the published free table is the LIVE parameter, the projected one the best epoch's
    assert np.array_equal(published[free], last[k_free])
    best_proj = published[proj]
    content = trainer.model.user_content if cold == "user" else trainer.model.item_content
    assert np.array_equal(best_proj, _np(content @ torch.from_numpy(best[k_w]).T))
    # the best epoch's model through the reference's own evaluation
    pair = [None, None]
    pair[free], pair[proj] = torch.from_numpy(best[k_free]), torch.from_numpy(best_proj)
    trainer.user_emb, trainer.item_emb = pair
    with contextlib.redirect_stdout(io.StringIO()):
        for kind in ("all", "cold", "warm"):
            trainer.full_evaluation(trainer.test(test_type=kind), test_type=kind)
    lists = mg._final_lists(trainer, data)
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    terms = np.array(terms, np.float64)
    for t in [terms, best_proj] + last + best:
        assert np.isfinite(t).all()
    a = cfg.args
    res = dict(
        which="DUIF", cold_object=cold, d=a.emb_size, epochs=a.epochs, batch_size=a.bs, lr=a.lr, reg=a.reg, seed=2024,
        data_seed=1, user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data),
        n_steps=terms.shape[0], terms=terms, param_names=json.dumps(names), best_is_last=best_is_last, best_proj=best_proj,
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **lists)
    res.update({f"init_{k}": p for k, p in enumerate(init)})
    res.update({f"trained_{k}": last[k] for k in moved})
    if not best_is_last:
        res.update({f"best_{k}": best[k] for k in moved})
    np.savez_compressed(os.path.join(HERE, f"g28_duif_{cold}.npz"), **res)
    print("g28 DUIF %s: %d steps on %d pairs; last terms %s; best %s" % (cold, terms.shape[0], res["n_train"], terms[-1],
                                                                          trainer.bestPerformance))


if __name__ == "__main__":
    g28("item")
    g28("user")
