"""CPU-only: the one epoch loop of the fused-loss trainers (coldrec_amd/model/FusedLossTrainer.py), driven by a stub that
supplies fixed batches and known loss rows: the order of the recorded rows, the every-50-steps print, early stopping,
eval_every, and that checkpoint, restore and --save_emb go by the trainer's table names."""
import argparse
import os
import types

import numpy as np
import pytest
import torch

from tests.test_host_logic import builder

STEPS = 120
TWO, THREE = ("user_emb", "item_emb"), ("warm_user_emb", "cold_user_emb", "item_emb")


def _stub(monkeypatch, names, **kw):
    import coldrec_amd.model.FusedLossTrainer as mod
    monkeypatch.setattr(mod, "_require_gpu", lambda device: None)
    a = dict(dataset="toy", model="Stub", epochs=5, layers=2, topN="10,20", bs=512, emb_size=16, lr=1e-3, reg=1e-4,
             early_stop=3, eval_every=1, cold_object="item", save_emb=False)
    a.update(kw)

    class Stub(mod.FusedLossTrainer):
        LOSS_TERMS = ("first", "second", "total")
        TABLES = names

        def _optimizers(self, model):
            return []

        def _epoch_batches(self):
            for n in range(STEPS):
                yield (n,)

        def _step(self, model, opts, batch):
            assert model.training and opts == [] and batch == (len(self.seen) % STEPS,)
            g = float(len(self.seen))                      # the run's step number
            self.seen.append(batch[0])
            return torch.tensor([g, 2 * g, 1000 + g])

        def _current_tables(self):
            assert not self.model.training and not torch.is_grad_enabled()
            self.made += 1                                  # every table says which call made it and which table it is
            return tuple(torch.tensor([self.made, k]) for k in range(len(names)))

        def fast_evaluation(self, epoch, valid_type="all"):
            self.evals.append(epoch)
            if epoch == 0:
                self.save()
            if epoch == 1 and self.early_stop_flag:         # trips early stopping in epoch 2
                self.early_stop_patience = 0

    tr = Stub(types.SimpleNamespace(args=argparse.Namespace(**a), data=builder()[1], device=torch.device("cpu")))
    tr.model = torch.nn.Linear(1, 1)
    tr.seen, tr.evals, tr.made = [], [], 0
    return tr


@pytest.mark.parametrize("names", [TWO, THREE], ids=["two-tables", "three-tables"])
def test_loop_records_prints_stops_restores_and_saves_by_name(names, monkeypatch, tmp_path, capsys):
    monkeypatch.chdir(tmp_path)
    tr = _stub(monkeypatch, names, save_emb=True)
    before = set(vars(tr))
    capsys.readouterr()
    tr.train()
    g = np.arange(2 * STEPS, dtype=float)
    assert tr.batch_losses.shape == (2 * STEPS, 3) and tr.batch_losses.dtype == np.float64
    assert np.array_equal(tr.batch_losses, np.stack([g, 2 * g, 1000 + g], 1))                     # the rows, in order
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("training:")]
    assert lines == [f"training: {e} batch {n} batch_loss: {1000.0 + (e - 1) * STEPS + n}" for e in (1, 2) for n in (0, 50, 100)]
    assert tr.epochs_ran == 2 and tr.evals == [0, 1] and tr.seen == list(range(STEPS)) * 2
    assert not tr.model.training
    # published after epochs 1 and 2 (calls 1 and 3), checkpointed by save() in epoch 1 (call 2): the checkpoint comes back
    assert tr.made == 3
    for k, name in enumerate(names):
        assert getattr(tr, name) is getattr(tr, "best_" + name) and getattr(tr, name).tolist() == [2, k]
    assert {n for n in set(vars(tr)) - before if n.endswith("_emb")} == set(names) | {"best_" + n for n in names}
    assert sorted(os.listdir(tmp_path / "emb")) == sorted(f"toy_cold_item_Stub_{n}.pt" for n in names)
    for k, name in enumerate(names):
        assert torch.load(tmp_path / "emb" / f"toy_cold_item_Stub_{name}.pt").tolist() == [2, k]


def test_loop_evaluates_every_other_epoch_and_writes_nothing_unasked(monkeypatch, tmp_path):
    monkeypatch.chdir(tmp_path)
    tr = _stub(monkeypatch, TWO, eval_every=2, early_stop=0)
    tr.train()
    assert tr.evals == [0, 2, 4] and tr.epochs_ran == 5 and tr.batch_losses.shape == (5 * STEPS, 3)
    assert tr.made == 6 and tr.user_emb.tolist() == [2, 0]                  # five publications and epoch 1's checkpoint
    assert not (tmp_path / "emb").exists()


def test_loop_without_epochs_and_the_stock_batch_predict(monkeypatch):
    from coldrec_amd.model.BaseRecommender import _is_stock_batch_predict
    from coldrec_amd.model.FusedLossTrainer import FusedLossTrainer
    assert _is_stock_batch_predict(FusedLossTrainer.batch_predict)
    tr = _stub(monkeypatch, TWO, epochs=0)
    tr.best_user_emb, tr.best_item_emb = torch.eye(3), torch.arange(12.).reshape(4, 3)
    tr.train()
    assert tr.epochs_ran == 0 and tr.batch_losses.shape == (0, 3) and tr.seen == [] and tr.made == 0
