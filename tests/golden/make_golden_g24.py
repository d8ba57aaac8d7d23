"""Generate G24 under tests/golden/ by RUNNING THE REFERENCE's MF.run() (the backbone, saved with save_emb) and then its
GAR.run() (model/GAR.py:15-62 through model/BaseRecommender.py:353-370), once per cold object.

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g24.py

g24_gar_item.npz   the toy item-cold split (make_dataset("toy", "item", seed=1), = toy_item.npz), d = 64, bs = 512.
g24_gar_user.npz   the toy user-cold split of the SAME data seed, make_dataset("toy", "user", seed=1) -- not toy_user.npz,
    which is seed 2: the tests build this split themselves (tests/gar_restate.py toy_data) --, the same settings.
    Backbone: MF, 3 epochs, set_seed(2024), on a builder of its own, inside a temporary working directory (./emb).
    GAR on a FRESH builder (the sampler shuffles the training pairs in place), set_seed(2024), epochs=2, alpha / beta
    at their defaults (0.05, 0.1).
    Observed from outside: the reference forms the loss inline in train(), so Tensor.backward is wrapped and reads the
    calling frame's [gen_loss, rec_loss, batch_loss] of every step.
    Stored: data only -- the saved backbone tables (the GAR run's input), the loss terms, the final (best-epoch)
    user_emb / item_emb, the three settings' test metrics and top-20 lists, the ``training:`` lines, the settings.
    Regenerates byte for byte.
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

BACKBONE = dict(model="MF", emb_size=64, epochs=3, bs=512, save_emb=True)
SETTINGS = dict(model="GAR", emb_size=64, epochs=2, bs=512, backbone="MF", alpha=0.05, beta=0.1)
TERMS = ("gen_loss", "rec_loss", "batch_loss")


def g24(cold):
    split = make_dataset("toy", cold, seed=1)
    mod = importlib.import_module("model.GAR")
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            os.makedirs("emb")
            mg.set_seed(2024, False)
            mg._run_quiet(mg.MF(mg.ref_config(mg.ref_builder(split), cold_object=cold, **BACKBONE)))
            loaded = [torch.load(f"./emb/toy_cold_{cold}_MF_{s}_emb.pt", map_location="cpu").detach().numpy().copy()
                      for s in ("user", "item")]

            data = mg.ref_builder(split)
            cfg = mg.ref_config(data, cold_object=cold, **SETTINGS)
            mg.set_seed(2024, False)
            trainer = mod.GAR(cfg)
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
    user, item = trainer.user_emb.detach().numpy(), trainer.item_emb.detach().numpy()
    for t in (user, item, losses):
        assert np.isfinite(t).all()
    res = dict(
        which="GAR", cold_object=cold, d=a.emb_size, epochs=a.epochs, batch_size=a.bs, alpha=a.alpha, beta=a.beta, lr=a.lr,
        reg=a.reg, seed=2024, data_seed=1, user_num=data.user_num, item_num=data.item_num,
        n_train=len(data.training_data), n_steps=losses.shape[0], loaded_U=loaded[0], loaded_V=loaded[1], losses=losses,
        user_emb=user, item_emb=item,
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **lists)
    np.savez_compressed(os.path.join(HERE, f"g24_gar_{cold}.npz"), **res)
    print("g24 GAR %s: %d steps; last losses %s; best %s" % (cold, losses.shape[0], losses[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g24("item")
    g24("user")
