"""Generate G21 under tests/golden/ by RUNNING THE REFERENCE's CCFCRec.run() (model/CCFCRec.py:10-129 through
model/BaseRecommender.py:353-370).

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g21.py

g21_ccfcrec.npz   the toy item-cold split (make_dataset("toy", "item", seed=1), = toy_item.npz), emb_size = implicit_dim =
    attr_present_dim = cat_implicit_dim = 64, epochs=2, bs=512, positive_number=3, negative_number=8, self_neg_number=8,
    tau=0.1, lambda1=0.6, pretrain false, set_seed(2024): 3 619 records, 8 steps per epoch.
    Observed from outside: the reference forms the loss inline in train(), so Tensor.backward is wrapped and reads the
    calling frame's [contrast_sum, self_contrast_sum, y_ukv, y_ukv2, batch_loss] of every step.
    Stored: outputs only -- the loss terms, the checksums of the initial tables, the final (best-epoch) user and item
    tables, the three settings' test metrics and top-20 lists, the ``training:`` lines.  Regenerates byte for byte.
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

SETTINGS = dict(emb_size=64, implicit_dim=64, attr_present_dim=64, cat_implicit_dim=64, epochs=2, bs=512,
                positive_number=3, negative_number=8, self_neg_number=8, tau=0.1, lambda1=0.6, pretrain=False,
                pretrain_update=False)
TERMS = ("contrast_sum", "self_contrast_sum", "y_ukv", "y_ukv2", "batch_loss")


def g21():
    split = make_dataset("toy", "item", seed=1)
    data = mg.ref_builder(split)
    cfg = mg.ref_config(data, model="CCFCRec", **SETTINGS)
    mg.set_seed(2024, False)
    mod = importlib.import_module("model.CCFCRec")
    trainer = mod.CCFCRec(cfg)
    learner = trainer.model
    U0, V0 = learner.user_embedding.detach().clone().numpy(), learner.item_embedding.detach().clone().numpy()
    losses = []
    real_backward = torch.Tensor.backward
    a = cfg.args

    def backward_spy(self, *args, **kw):
        frame = sys._getframe(1).f_locals
        assert frame["batch_loss"] is self
        losses.append([float(frame[k].item()) for k in TERMS])
        return real_backward(self, *args, **kw)

    torch.Tensor.backward = backward_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        torch.Tensor.backward = real_backward
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    losses = np.array(losses, np.float64)
    n_steps = losses.shape[0]
    U, V = trainer.user_emb.detach().numpy(), trainer.item_emb.detach().numpy()
    assert np.isfinite(U).all() and np.isfinite(V).all() and np.isfinite(losses).all()
    res = dict(
        which="CCFCRec", d=a.implicit_dim, epochs=a.epochs, batch_size=a.bs, positive_number=a.positive_number,
        negative_number=a.negative_number, self_neg_number=a.self_neg_number, tau=a.tau, lambda1=a.lambda1, lr=a.lr,
        seed=2024, data_seed=1, user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data),
        n_steps=n_steps, losses=losses, U0_crc=np.int64(mg._crc(U0)), V0_crc=np.int64(mg._crc(V0)), U=U, V=V,
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **mg._final_lists(trainer, data))
    np.savez_compressed(os.path.join(HERE, "g21_ccfcrec.npz"), **res)
    print("g21 CCFCRec: %d steps; last losses %s; best %s" % (n_steps, losses[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g21()
