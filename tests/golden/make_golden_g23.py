"""Generate G23 under tests/golden/ by RUNNING THE REFERENCE's NCL (model/NCL.py).

Run in the build container only (the reference does not exist on the GPU box), beside make_golden.py, whose helpers
(the reference imported in place, the toy split's builder, the final top-20 lists) it uses:

    OMP_NUM_THREADS=1 MKL_NUM_THREADS=1 python tests/golden/make_golden_g23.py

model/NCL.py imports faiss at its top, which is absent here.  This maker -- and nothing else in the repository -- puts an
empty stand-in module named faiss into sys.modules so that the import succeeds; nothing of it is called before epoch 20
(e_step), and no fixture below gets that far.

g23_ssl.npz   NCL.ssl_layer_loss (model/NCL.py:68-94) called on a stub ``self`` (data.user_num / item_num, ssl_temp, ssl_reg,
    alpha), with autograd gradients of context_emb and initial_emb.  The inputs are drawn in float32 (stored so: what a kernel
    is fed) and handed to the reference's method as float64 tensors of the same values, so that the stored outputs are the
    reference's formula and not its float32 rounding: in float32 the method's own error reached 1.6e-6 of the gradient's
    maximum on case c, above the 1e-6 the fixture is read at.  Three seeded cases, inputs and outputs stored:
    a  U = 33, I = 45, d = 36, B = 40 with repeated ids;  b  U = 129, I = 7, d = 64, B = 5;  c  the context IS the initial
    table (one tensor, one gradient).
g23_ncl.npz   NCL.run() on the toy item-cold split (make_dataset("toy", "item", seed=1), = toy_item.npz): layers=3,
    hyper_layers=1, emb_size=64, epochs=2, bs=512, tau=0.2, alpha=1.0, set_seed(2024).  The reference's default
    ssl_reg = 1e-6 leaves the structure term seven orders under BPR, where no test would see it; ssl_reg = 1e-4 is used
    instead, which puts the first batch's weighted term at 0.44 x its BPR term (asserted below to lie within 0.1x .. 10x).
    Observed from outside, as G19 is: bpr_loss / l2_reg_loss as the trainer's module sees them and the trainer's
    ssl_layer_loss are wrapped to record every batch's terms [bpr, l2, ssl_user, ssl_item] (the ssl terms unscaled: the user
    term from a second call of the reference's method with ssl_reg = 1, alpha = 0 on a stub, the item term as the
    difference to the call with alpha = 1; ssl_total is what the trainer's own call returned).  Stored: outputs only -- the
    loss terms, the checksums of the initial tables, the final (best-epoch) user and item tables, the three settings' test
    metrics and top-20 lists.  Regenerates byte for byte.
"""
import contextlib
import importlib
import io
import json
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (puts the reference on sys.path and imports it in place)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from coldrec_amd.data.synth import make_dataset  # noqa: E402  (ours: input generator only)

sys.modules.setdefault("faiss", types.ModuleType("faiss"))      # see the docstring
ncl_mod = importlib.import_module("model.NCL")                  # (reference)

SSL_REG = 1e-4
SETTINGS = dict(layers=3, hyper_layers=1, emb_size=64, epochs=2, bs=512, tau=0.2, alpha=1.0, ssl_reg=SSL_REG,
                proto_reg=1e-7, num_clusters=20)


def stub(user_num, item_num, tau, ssl_reg, alpha):
    return types.SimpleNamespace(data=types.SimpleNamespace(user_num=user_num, item_num=item_num), ssl_temp=tau,
                                 ssl_reg=ssl_reg, alpha=alpha)


def g23_ssl():
    res = dict(cases=np.array(["a", "b", "c"]))
    shapes = dict(a=(33, 45, 36, 40, False), b=(129, 7, 64, 5, False), c=(20, 30, 32, 24, True))
    for k, (name, (U, I, d, B, alias)) in enumerate(shapes.items()):
        g = torch.Generator().manual_seed(2300 + k)
        init32 = torch.randn(U + I, d, generator=g) * 0.3
        ctx32 = init32 if alias else init32 * 0.5 + torch.randn(U + I, d, generator=g) * 0.2
        initial = init32.double().requires_grad_()
        context = initial if alias else ctx32.double().requires_grad_()
        user = torch.randint(0, U, (B,), generator=g)
        item = torch.randint(0, I, (B,), generator=g)
        if name == "a":
            user[5], user[9], item[7] = user[0], user[0], item[1]                      # repeated ids, whatever the draw
        user[B // 2], item[B // 2] = U - 1, I - 1
        tau, ssl_reg, alpha = 0.2, 0.5, 0.7
        loss = ncl_mod.NCL.ssl_layer_loss(stub(U, I, tau, ssl_reg, alpha), context, initial, user, item)
        loss.backward()
        assert loss.dtype == torch.float64 and init32.dtype == ctx32.dtype == torch.float32
        res.update({f"{name}_U": U, f"{name}_I": I, f"{name}_tau": tau, f"{name}_ssl_reg": ssl_reg, f"{name}_alpha": alpha,
                    f"{name}_alias": alias, f"{name}_initial": init32.numpy(),
                    f"{name}_context": ctx32.numpy(), f"{name}_user": user.numpy(), f"{name}_item": item.numpy(),
                    f"{name}_loss": np.float64(loss.item()), f"{name}_g_initial": initial.grad.numpy(),
                    f"{name}_g_context": context.grad.numpy()})
        print("g23 ssl %s: loss %.6f" % (name, loss.item()))
    np.savez_compressed(os.path.join(HERE, "g23_ssl.npz"), **res)


def g23_ncl():
    split = make_dataset("toy", "item", seed=1)
    data = mg.ref_builder(split)
    cfg = mg.ref_config(data, model="NCL", **SETTINGS)
    mg.set_seed(2024, False)
    trainer = ncl_mod.NCL(cfg)
    params = dict(trainer.model.embedding_dict.items())
    U0, V0 = params["user_emb"].detach().clone().numpy(), params["item_emb"].detach().clone().numpy()
    rec = dict(bpr=[], l2=[], ssl=[], ssl_u=[], ssl_i=[])
    real_bpr, real_l2, real_ssl = ncl_mod.bpr_loss, ncl_mod.l2_reg_loss, trainer.ssl_layer_loss

    def spy(real, key):
        def f(*a, **kw):
            out_ = real(*a, **kw)
            rec[key].append(float(out_.item()))
            return out_
        return f

    def ssl_spy(context_emb, initial_emb, user, item):
        out_ = real_ssl(context_emb, initial_emb, user, item)
        with torch.no_grad():
            a = trainer.args
            only_u = ncl_mod.NCL.ssl_layer_loss(stub(data.user_num, data.item_num, a.tau, 1.0, 0.0), context_emb, initial_emb,
                                                user, item)
            both = ncl_mod.NCL.ssl_layer_loss(stub(data.user_num, data.item_num, a.tau, 1.0, 1.0), context_emb, initial_emb,
                                              user, item)
        rec["ssl"].append(float(out_.item()))
        rec["ssl_u"].append(float(only_u.item()))
        rec["ssl_i"].append(float(both.item()) - float(only_u.item()))
        return out_

    ncl_mod.bpr_loss, ncl_mod.l2_reg_loss = spy(real_bpr, "bpr"), spy(real_l2, "l2")
    trainer.ssl_layer_loss = ssl_spy
    try:
        with contextlib.redirect_stdout(io.StringIO()) as buf:
            trainer.run()
    finally:
        ncl_mod.bpr_loss, ncl_mod.l2_reg_loss = real_bpr, real_l2
    loss_lines = [ln for ln in buf.getvalue().splitlines() if ln.startswith("training:")]
    n_steps = len(rec["bpr"])
    assert len(rec["l2"]) == n_steps and len(rec["ssl"]) == n_steps
    losses = np.stack([np.array(rec[k], np.float64) for k in ("bpr", "l2", "ssl_u", "ssl_i")], 1)
    a = cfg.args
    weighted = a.ssl_reg * (losses[0, 2] + a.alpha * losses[0, 3])
    assert 0.1 * losses[0, 0] <= weighted <= 10 * losses[0, 0], (weighted, losses[0, 0])
    res = dict(
        which="NCL", layers=a.layers, hyper_layers=a.hyper_layers, d=a.emb_size, epochs=a.epochs, batch_size=a.bs,
        tau=a.tau, alpha=a.alpha, ssl_reg=a.ssl_reg, proto_reg=a.proto_reg, num_clusters=a.num_clusters, lr=a.lr, reg=a.reg,
        seed=2024, data_seed=1, user_num=data.user_num, item_num=data.item_num, n_train=len(data.training_data),
        n_steps=n_steps, losses=losses, ssl_total=np.array(rec["ssl"], np.float64),
        U0_crc=np.int64(mg._crc(U0)), V0_crc=np.int64(mg._crc(V0)),
        U=trainer.user_emb.detach().numpy(), V=trainer.item_emb.detach().numpy(),
        test_overall=np.array(trainer.overall_test_results, np.float64),
        test_cold=np.array(trainer.cold_test_results, np.float64),
        test_warm=np.array(trainer.warm_test_results, np.float64), epochs_ran=trainer.epochs_ran,
        best_epoch=trainer.bestPerformance[0], best_metrics=json.dumps(trainer.bestPerformance[1]),
        loss_lines=json.dumps(loss_lines), torch_version=torch.__version__, **mg._final_lists(trainer, data))
    np.savez_compressed(os.path.join(HERE, "g23_ncl.npz"), **res)
    print("g23 NCL: %d steps; first weighted ssl / bpr = %.3f; last losses %s; best %s"
          % (n_steps, weighted / losses[0, 0], losses[-1], trainer.bestPerformance))


if __name__ == "__main__":
    g23_ssl()
    g23_ncl()
