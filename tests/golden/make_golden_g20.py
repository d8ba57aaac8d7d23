"""Generate G20 under tests/golden/ by RUNNING THE REFERENCE's CLCRec.run() (model/CLCRec.py:9-157 through
model/BaseRecommender.py:353-370).

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g20.py

g20_clcrec.npz   the toy item-cold split (make_dataset("toy", "item", seed=1), = toy_item.npz), emb_size=64, epochs=2,
    bs=512, num_neg=16, temp_value=2.0, lr_lambda=0.5, num_sample=0.5, set_seed(2024): 3 619 records, 8 steps per epoch.
    Observed from outside: the learner's forward is wrapped to record every step's [contrastive_loss_1, contrastive_loss_2,
    reg_loss, total] (the total as loss() forms it), and torch.randint to checksum the FIRST draw of the mixing index and
    count the draws (a torch whose CPU stream differs is detected by that checksum).
    Stored: outputs only -- the loss terms, the checksums of the initial tables and of the first index draw, the final
    (best-epoch) user and item tables, the three settings' test metrics and top-20 lists.  Regenerates byte for byte.
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

SETTINGS = dict(emb_size=64, epochs=2, bs=512, num_neg=16, temp_value=2.0, lr_lambda=0.5, num_sample=0.5)


def g20():
    split = make_dataset("toy", "item", seed=1)
    data = mg.ref_builder(split)
    cfg = mg.ref_config(data, model="CLCRec", **SETTINGS)
    mg.set_seed(2024, False)
    mod = importlib.import_module("model.CLCRec")
    trainer = mod.CLCRec(cfg)
    params = dict(trainer.model.embedding_dict.items())
    U0, V0 = params["user_emb"].detach().clone().numpy(), params["item_emb"].detach().clone().numpy()
    rec = dict(losses=[], crc=None, shape=None, high=None, draws=0)
    learner = trainer.model
    real_forward, real_randint = learner.forward, torch.randint
    a = cfg.args

    def forward_spy(*args, **kw):
        contrastive, reg = real_forward(*args, **kw)
        rec["losses"].append([float(learner.contrastive_loss_1.item()), float(learner.contrastive_loss_2.item()),
                              float(reg.item()), float((a.reg * reg + contrastive).item())])
        return contrastive, reg

    def randint_spy(*args, **kw):
        out_ = real_randint(*args, **kw)
        if rec["crc"] is None:
            rec["crc"], rec["shape"], rec["high"] = mg._crc(out_.numpy()), tuple(out_.shape), int(args[0])
            assert out_.dtype == torch.int64
        rec["draws"] += 1
        return out_

    learner.forward = forward_spy
    torch.randint = randint_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        del learner.forward
        torch.randint = real_randint
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    losses = np.array(rec["losses"], np.float64)
    n_steps = losses.shape[0]
    res = dict(
        which="CLCRec", d=a.emb_size, epochs=a.epochs, batch_size=a.bs, num_neg=a.num_neg, temp_value=a.temp_value,
        lr_lambda=a.lr_lambda, num_sample=a.num_sample, lr=a.lr, reg=a.reg, seed=2024, data_seed=1,
        user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data), n_steps=n_steps,
        losses=losses, randint_crc=np.int64(rec["crc"]), randint_shape=np.array(rec["shape"], np.int64),
        randint_high=np.int64(rec["high"]), randint_draws=np.int64(rec["draws"]),
        U0_crc=np.int64(mg._crc(U0)), V0_crc=np.int64(mg._crc(V0)),
        U=trainer.user_emb.detach().numpy(), V=trainer.item_emb.detach().numpy(),
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **mg._final_lists(trainer, data))
    np.savez_compressed(os.path.join(HERE, "g20_clcrec.npz"), **res)
    print("g20 CLCRec: %d steps, %d index draws; last losses %s; best %s"
          % (n_steps, rec["draws"], losses[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g20()
