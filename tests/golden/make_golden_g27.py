"""Generate G27 under tests/golden/ by RUNNING THE REFERENCE's MF.run() (the backbone, saved with save_emb) and then its
MetaEmbedding.run() (model/MetaEmbedding.py:16-74) and DeepMusic.run() (model/DeepMusic.py:12-60), once per cold object.

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g27.py

g27_metaemb_{item,user}.npz, g27_deepmusic_{item,user}.npz
    The toy splits of data seed 1, make_dataset("toy", cold, seed=1) (the user-cold one is not toy_user.npz, which is seed
    2: the tests build the split themselves, tests/gar_restate.py toy_data), d = 64, bs = 512.
    Backbone: MF, 3 epochs, set_seed(2024), on a builder of its own, inside a temporary working directory (./emb).
    The trainer on a FRESH builder (the sampler shuffles the training pairs in place), set_seed(2024), epochs = 2,
    lr = 0.001, reg = 0.0001, MetaEmbedding's alpha at its default 0.5.
    Observed from outside: the reference forms the loss inline in train(), so Tensor.backward is wrapped and reads the
    calling frame of every step: MetaEmbedding's [batch_loss_a, batch_loss_b, ME_loss]; DeepMusic's frame holds the
    total only, so its two terms are formed from the frame's two (B, d) blocks with the reference's own mse_loss and
    l2_reg_loss, [mse, reg, batch_loss].
    Stored: data only -- the saved backbone tables (the run's input), the generator's parameters before and after the
    run (in named_parameters() order, the frozen tables left out), the loss terms, the final (best-epoch) user_emb /
    item_emb, the three settings' test metrics and top-20 lists, the ``training:`` lines, the settings.
g27_metaemb_item_hi.npz
    At lr = 0.001 the inner step moves a score by cold_lr |o|^2 / N = 1e-4 |o|^2 / 1024, below float32 resolution: a
    kernel that ignored the inner step would pass the runs above.  This run is the item-cold one again at HI's lr and bs,
    one epoch, chosen by measuring |o|^2 = the squared norm of a row of the G27 item-cold backbone's USER table (the
    frozen side of item mode): mean |o|^2 = 0.3499 (printed by this script, the bound asserted below), so with lr = 0.25,
    cold_lr = 0.025 and bs = 4 (N = 8) cold_lr mean|o|^2 / N = 1.09e-3 >= 1e-3 (905 steps; the largest |loss_b -
    loss_a| of a step is 7.9e-4).
    Stored: the loss terms, the generator's parameters before and after, the final item_emb (the user table and the
    loaded tables are g27_metaemb_item.npz's loaded ones), the settings and the measured mean |o|^2.
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
SETTINGS = dict(MetaEmbedding=dict(model="MetaEmbedding", emb_size=64, epochs=2, bs=512, backbone="MF", alpha=0.5),
                DeepMusic=dict(model="DeepMusic", emb_size=64, epochs=2, bs=512, backbone="MF"))
HI = dict(model="MetaEmbedding", emb_size=64, epochs=1, bs=4, lr=0.25, backbone="MF", alpha=0.5)
FILES = dict(MetaEmbedding="metaemb", DeepMusic="deepmusic")


def _terms(which, cold, frame, loss):
    if which == "MetaEmbedding":
        assert frame["ME_loss"] is loss
        return [float(frame[k].item()) for k in ("batch_loss_a", "batch_loss_b", "ME_loss")]
    from util.utils import l2_reg_loss, mse_loss
    assert frame["batch_loss"] is loss
    real, made = (frame[f"pos_{cold}_emb"], frame[f"pos_{cold}_content_emb"])
    with torch.no_grad():
        return [float(mse_loss(real, made)), float(l2_reg_loss(frame["self"].reg, made)), float(loss.item())]


def _generator_params(trainer):
    return [p.detach().numpy().copy() for n, p in trainer.model.named_parameters() if not n.startswith("embedding_dict")]


def _run(which, cold, settings, with_lists=True):
    split = make_dataset("toy", cold, seed=1)
    mod = importlib.import_module("model." + which)
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
            cfg = mg.ref_config(data, cold_object=cold, **settings)
            mg.set_seed(2024, False)
            trainer = getattr(mod, which)(cfg)
            init = _generator_params(trainer)
            losses = []
            real_backward = torch.Tensor.backward

            def backward_spy(self, *args, **kw):
                losses.append(_terms(which, cold, sys._getframe(1).f_locals, self))
                return real_backward(self, *args, **kw)

            torch.Tensor.backward = backward_spy
            try:
                with contextlib.redirect_stdout(io.StringIO()) as buf:
                    trainer.run()
            finally:
                torch.Tensor.backward = real_backward
            lists = mg._final_lists(trainer, data) if with_lists else {}
        finally:
            os.chdir(cwd)
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    losses = np.array(losses, np.float64)
    final = _generator_params(trainer)
    a = cfg.args
    user, item = trainer.user_emb.detach().numpy(), trainer.item_emb.detach().numpy()
    for t in [user, item, losses] + final:
        assert np.isfinite(t).all()
    res = dict(
        which=which, cold_object=cold, d=a.emb_size, epochs=a.epochs, batch_size=a.bs, lr=a.lr, reg=a.reg, seed=2024,
        data_seed=1, user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data),
        n_steps=losses.shape[0], n_params=len(init), losses=losses, epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__,
        **{f"gen_init_{k}": p for k, p in enumerate(init)}, **{f"gen_final_{k}": p for k, p in enumerate(final)}, **lists)
    if which == "MetaEmbedding":
        res["alpha"] = a.alpha
    return res, loaded, (user, item), trainer


def g27(which, cold):
    res, loaded, (user, item), trainer = _run(which, cold, SETTINGS[which])
    res.update(loaded_U=loaded[0], loaded_V=loaded[1], user_emb=user, item_emb=item,
               test_overall=np.array(trainer.overall_test_results, np.float64),
               test_cold=np.array(trainer.cold_test_results, np.float64),
               test_warm=np.array(trainer.warm_test_results, np.float64))
    np.savez_compressed(os.path.join(HERE, f"g27_{FILES[which]}_{cold}.npz"), **res)
    print("g27 %s %s: %d steps; last losses %s; best %s" % (which, cold, res["n_steps"], res["losses"][-1],
                                                             trainer.bestPerformance))


def g27_hi():
    res, loaded, (user, item), trainer = _run("MetaEmbedding", "item", HI, with_lists=False)
    assert np.array_equal(user, loaded[0])                                  # item mode: the user table is the loaded one
    oo = float((loaded[0].astype(np.float64) ** 2).sum(1).mean())
    move = HI["lr"] / 10. * oo / (2 * HI["bs"])
    print("g27 hi: mean |o|^2 of the user table %.4f; cold_lr mean|o|^2 / N = %.3e" % (oo, move))
    assert move >= 1e-3
    gap = np.abs(res["losses"][:, 1] - res["losses"][:, 0])
    res.update(item_emb=item, mean_oo=oo, move=move)
    np.savez_compressed(os.path.join(HERE, "g27_metaemb_item_hi.npz"), **res)
    print("g27 hi: %d steps; last losses %s; |loss_b - loss_a| mean %.3e max %.3e" % (res["n_steps"], res["losses"][-1],
                                                                                       gap.mean(), gap.max()))


if __name__ == "__main__":
    for which in ("MetaEmbedding", "DeepMusic"):
        for cold in ("item", "user"):
            g27(which, cold)
    g27_hi()
