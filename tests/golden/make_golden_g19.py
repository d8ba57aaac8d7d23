"""Generate G19 under tests/golden/ by RUNNING THE REFERENCE's SimGCL.run() and XSimGCL.run() (model/SimGCL.py:10-113,
model/XSimGCL.py:10-124 through model/BaseRecommender.py:353-370).

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g19.py

g19_simgcl.npz / g19_xsimgcl.npz   the toy item-cold split (make_dataset("toy", "item", seed=1), = toy_item.npz),
    layers=3, emb_size=64, epochs=2, bs=512, cl_rate=0.5, tau=0.2, eps=0.1 (l_cl=2 for XSimGCL), set_seed(2024).
    Observed from outside, as G12 is: bpr_loss / l2_reg_loss / InfoNCE as the trainer's module sees them are wrapped to
    record every batch's four loss terms [bpr, l2, cl_user, cl_item] (the InfoNCE terms unscaled, as returned), and
    torch.rand_like to checksum the FIRST noise draw (a torch whose CPU stream differs is detected by that checksum).
    Stored: outputs only -- the loss terms, the checksums of the initial tables and of the first noise draw, the final
    (best-epoch, clean) user and item tables, the three settings' test metrics and top-20 lists.  Regenerates byte for byte.
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

SETTINGS = dict(layers=3, emb_size=64, epochs=2, bs=512, cl_rate=0.5, tau=0.2, eps=0.1)


def g19(cls_name, **extra):
    split = make_dataset("toy", "item", seed=1)
    data = mg.ref_builder(split)
    cfg = mg.ref_config(data, model=cls_name, **SETTINGS, **extra)
    mg.set_seed(2024, False)
    mod = importlib.import_module("model." + cls_name)
    trainer = getattr(mod, cls_name)(cfg)
    params = dict(trainer.model.embedding_dict.items())
    U0, V0 = params["user_emb"].detach().clone().numpy(), params["item_emb"].detach().clone().numpy()
    rec = dict(bpr=[], l2=[], cl=[], noise_crc=None, noise_shape=None, draws=0)
    real_bpr, real_l2, real_nce, real_rand_like = mod.bpr_loss, mod.l2_reg_loss, mod.InfoNCE, torch.rand_like

    def spy(real, key):
        def f(*a, **kw):
            out_ = real(*a, **kw)
            rec[key].append(float(out_.item()))
            return out_
        return f

    def rand_like_spy(*a, **kw):
        out_ = real_rand_like(*a, **kw)
        if rec["noise_crc"] is None:
            rec["noise_crc"], rec["noise_shape"] = mg._crc(out_.numpy()), tuple(out_.shape)
            assert out_.dtype == torch.float32
        rec["draws"] += 1
        return out_

    mod.bpr_loss, mod.l2_reg_loss, mod.InfoNCE = spy(real_bpr, "bpr"), spy(real_l2, "l2"), spy(real_nce, "cl")
    torch.rand_like = rand_like_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        mod.bpr_loss, mod.l2_reg_loss, mod.InfoNCE = real_bpr, real_l2, real_nce
        torch.rand_like = real_rand_like
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    n_steps = len(rec["bpr"])
    assert len(rec["l2"]) == n_steps and len(rec["cl"]) == 2 * n_steps
    cl = np.array(rec["cl"], np.float64).reshape(n_steps, 2)
    losses = np.stack([np.array(rec["bpr"], np.float64), np.array(rec["l2"], np.float64), cl[:, 0], cl[:, 1]], 1)
    a = cfg.args
    res = dict(
        which=cls_name, layers=a.layers, d=a.emb_size, epochs=a.epochs, batch_size=a.bs, cl_rate=a.cl_rate, tau=a.tau,
        eps=a.eps, l_cl=int(getattr(a, "l_cl", 0)), lr=a.lr, reg=a.reg, seed=2024, data_seed=1,
        user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data), n_steps=n_steps,
        losses=losses, noise_crc=np.int64(rec["noise_crc"]), noise_shape=np.array(rec["noise_shape"], np.int64),
        noise_draws=np.int64(rec["draws"]), U0_crc=np.int64(mg._crc(U0)), V0_crc=np.int64(mg._crc(V0)),
        U=trainer.user_emb.detach().numpy(), V=trainer.item_emb.detach().numpy(),
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **mg._final_lists(trainer, data))
    np.savez_compressed(os.path.join(HERE, "g19_%s.npz" % cls_name.lower()), **res)
    print("g19 %s: %d steps, %d noise draws; last losses %s; best %s"
          % (cls_name, n_steps, rec["draws"], losses[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g19("SimGCL")
    g19("XSimGCL", l_cl=2)
