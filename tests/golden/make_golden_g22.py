"""Generate G22 under tests/golden/ by RUNNING THE REFERENCE's MF.run() (the teacher, saved with save_emb) and then its
ALDI.run() (model/ALDI.py:25-160 through model/BaseRecommender.py:353-370).

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g22.py

g22_aldi.npz   the toy item-cold split (make_dataset("toy", "item", seed=1), = toy_item.npz), d = 64, bs = 512.
    Teacher: MF, 3 epochs, set_seed(2024), on a builder of its own, inside a temporary working directory (./emb).
    Student: ALDI on a FRESH builder (the sampler shuffles the training pairs in place), set_seed(2024), epochs=2,
    tws=1, freq_coef_M=4, alpha / beta / gamma / aldi_hidden at their defaults (0.9, 0.05, 0.1, 200).
    Observed from outside: the reference forms the loss inline in train(), so Tensor.backward is wrapped and reads the
    calling frame's [basic_loss, rating_dist_loss, ranking_dist_loss, iden_dist_loss, batch_loss] of every step.
    Stored: data only -- the saved teacher tables (the ALDI run's input), the item frequencies and pos_item_weights for
    tws 0 and 1, the loss terms, the final (best-epoch) warm_user_emb / cold_user_emb / item_emb, the three settings'
    test metrics and top-20 lists, the ``training:`` lines.  Regenerates byte for byte.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports it in place)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coldrec_amd.data.synth import make_dataset  # noqa: E402  (ours: input generator only)

TEACHER = dict(model="MF", emb_size=64, epochs=3, bs=512, save_emb=True)
SETTINGS = dict(model="ALDI", emb_size=64, epochs=2, bs=512, backbone="MF", alpha=0.9, beta=0.05, gamma=0.1, tws=1,
                freq_coef_M=4.0, aldi_hidden=200)
TERMS = ("basic_loss", "rating_dist_loss", "ranking_dist_loss", "iden_dist_loss", "batch_loss")


def g22():
    split = make_dataset("toy", "item", seed=1)
    mod = importlib.import_module("model.ALDI")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("emb")
            mg.set_seed(2024, False)
            mg._run_quiet(mg.MF(mg.ref_config(mg.ref_builder(split), **TEACHER)))
            teacher = [torch.load(f"./emb/toy_cold_item_MF_{s}_emb.pt", map_location="cpu").detach().numpy().copy()
                       for s in ("user", "item")]

            data = mg.ref_builder(split)
            cfg = mg.ref_config(data, **SETTINGS)
            mg.set_seed(2024, False)
            trainer = mod.ALDI(cfg)
            w1 = trainer.model.pos_item_weights.detach().numpy().copy()
            w0 = mod.ALDI_Learner(mg.ref_args(**dict(SETTINGS, tws=0)), data, 64,
                                  torch.device("cpu")).pos_item_weights.detach().numpy().copy()
            freq = mod._aldi_item_frequency(data)
            # (the second learner drew from the global generator: the run starts from the seed again)
            mg.set_seed(2024, False)
            trainer = mod.ALDI(cfg)
            losses = []
            real_backward = torch.Tensor.backward

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
            lists = mg._final_lists(trainer, data)
        finally:
            os.chdir(cwd)
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    losses = np.array(losses, np.float64)
    a = cfg.args
    warm_u, cold_u = trainer.warm_user_emb.detach().numpy(), trainer.cold_user_emb.detach().numpy()
    item = trainer.item_emb.detach().numpy()
    assert np.array_equal(warm_u, teacher[0])                    # the teacher's users, unchanged
    for t in (cold_u, item, losses):
        assert np.isfinite(t).all()
    res = dict(
        which="ALDI", d=a.emb_size, epochs=a.epochs, batch_size=a.bs, alpha=a.alpha, beta=a.beta, gamma=a.gamma, tws=a.tws,
        freq_coef_M=a.freq_coef_M, aldi_hidden=a.aldi_hidden, lr=a.lr, reg=a.reg, seed=2024, data_seed=1,
        user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data), n_steps=losses.shape[0],
        teacher_U=teacher[0], teacher_V=teacher[1], item_freq=freq, weights_tws0=w0, weights_tws1=w1, losses=losses,
        warm_user_emb=warm_u, cold_user_emb=cold_u, item_emb=item,
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **lists)
    np.savez_compressed(os.path.join(HERE, "g22_aldi.npz"), **res)
    print("g22 ALDI: %d steps; last losses %s; best %s" % (losses.shape[0], losses[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g22()
