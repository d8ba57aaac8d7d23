"""What the trainers around a fused HIP loss (CLCRec, CCFCRec, ALDI, GAR, MTPR, VBPR, AMR, MetaEmbedding, DeepMusic, DUIF) share: the epoch loop, the checkpoint of
the published tables, ``--save_emb``, the stock ``predict`` pair, and the loading of a backbone's saved tables.

A trainer states the names of its loss terms and of the tables it publishes, and supplies ``_optimizers``,
``_current_tables`` and, where the defaults do not fit, ``_epoch_batches`` and ``_step``.
"""
import os

import numpy as np
import torch

from ..train import dp_from_env
from ..util.utils import epoch_triples
from .BaseRecommender import BaseColdStartTrainer
from .MF import _require_gpu


def load_backbone_tables(who, args, data, emb_size=None, save_flag=' --save_emb true'):
    """The (user, item) tables a backbone run saved under ./emb, float32 on the CPU.  ``who`` fronts the messages (the
    trainer, with the flag that asks for the tables if there is one); ``emb_size`` is the width they must have (None: the
    two must agree); ``save_flag`` is what the suggested backbone command ends in."""
    stem = f'./emb/{args.dataset}_cold_{args.cold_object}_{args.backbone}'
    paths = (stem + '_user_emb.pt', stem + '_item_emb.pt')
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(
                f'{who} requires {p}. Train the backbone first '
                f'(e.g. main.py --model {args.backbone} --dataset {args.dataset} '
                f'--cold_object {args.cold_object}{save_flag}) or set --backbone to match '
                f'existing files under ./emb/.')
    tables = [torch.load(p, map_location='cpu').detach().float().contiguous() for p in paths]
    width = tables[0].shape[1] if emb_size is None else emb_size
    if tables[0].shape != (data.user_num, width) or tables[1].shape != (data.item_num, width):
        raise ValueError(f'{who}: the tables under {stem}_*_emb.pt do not fit this dataset'
                         + ('' if emb_size is None else f' and --emb_size {emb_size}'))
    return tables


VBPR_FILES = {'user_emb_main': 'user_emb_main_P', 'item_emb_main': 'item_emb_main_Q', 'user_emb_aux': 'user_emb_aux',
              'item_emb_aux': 'item_emb_aux', 'w_value': 'W'}      # table -> the reference's file name (model/VBPR.py:50-54)


def load_vbpr_tables(who, args, data, emb_size, content_dim):
    """The five tensors a VBPR run saved under ./emb (either implementation's: the file names are the reference's), float32
    on the CPU, in VBPR_FILES' order; ``who`` fronts the messages."""
    stem = f'./emb/{args.dataset}_cold_{args.cold_object}_VBPR'
    paths = [f'{stem}_{suffix}.pt' for suffix in VBPR_FILES.values()]
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(
                f'{who} requires {p}. Train VBPR first '
                f'(e.g. main.py --model VBPR --dataset {args.dataset} --cold_object {args.cold_object} '
                f'--emb_size {emb_size} --save_emb true).')
    tensors = [torch.load(p, map_location='cpu').detach().float().contiguous() for p in paths]
    shapes = [(data.user_num, emb_size), (data.item_num, emb_size), (data.user_num, emb_size), (data.item_num, emb_size),
              (content_dim, emb_size)]
    for p, t, shape in zip(paths, tensors, shapes):
        if tuple(t.shape) != shape:
            raise ValueError(f'{who}: {p} is {tuple(t.shape)}, this dataset and --emb_size {emb_size} need {shape}')
    return tensors


class FusedLossTrainer(BaseColdStartTrainer):
    LOSS_TERMS = ()                         # the names of model.last_terms' entries; the last one is the step's total
    TABLES = ('user_emb', 'item_emb')       # the attributes _current_tables() fills, in its order
    SAVE_FILES = None                       # {table: file name's last part} of --save_emb; None: every table as '<table>.pt'
    UPLOAD_BATCHES = 64                     # _block_batches: batches of ids uploaded at once

    def _optimizers(self, model):
        """The optimizers of one run, built once the model is on the device."""
        return [torch.optim.Adam(model.parameters(), lr=self.lr)]

    def _epoch_batches(self):
        """One epoch's argument tuples of ``model.loss``, on the device: here the pairwise sampler's triples, the whole
        epoch from the reference's stream in one upload, with the ids' ranges measured once on the host."""
        B = self.batch_size
        ep = epoch_triples(self.data, B)
        id_range = ((int(ep[0].min()), int(ep[0].max())),
                    (int(min(ep[1].min(), ep[2].min())), int(max(ep[1].max(), ep[2].max()))))
        eu, ei, ej = (torch.from_numpy(x).to(self.device) for x in ep)
        for lo in range(0, eu.shape[0], B):
            yield eu[lo:lo + B], ei[lo:lo + B], ej[lo:lo + B], id_range

    def _block_batches(self, arrays):
        """The batches of an epoch drawn on the host as ``arrays`` (one row per record), uploaded UPLOAD_BATCHES at a time."""
        B = self.batch_size
        block = B * self.UPLOAD_BATCHES
        for lo in range(0, arrays[0].shape[0], B):
            if lo % block == 0:
                dev = [torch.from_numpy(a[lo:lo + block]).to(self.device) for a in arrays]
            o = lo % block
            yield tuple(t[o:o + B] for t in dev)

    def _step(self, model, opts, batch):
        """One optimizer step; returns the device row of the step's loss terms."""
        batch_loss = model.loss(*batch)
        for opt in opts:
            opt.zero_grad()
        batch_loss.backward()
        for opt in opts:
            opt.step()
        return model.last_terms

    def _current_tables(self):
        """The tables of TABLES as evaluation takes them (called with the model in eval mode, under no_grad)."""
        raise NotImplementedError

    def _set_tables(self, prefix, tables):
        for name, t in zip(self.TABLES, tables):
            setattr(self, prefix + name, t)

    def train(self):
        _require_gpu(self.device)
        if dp_from_env() is not None:
            raise RuntimeError(f'{type(self).__name__}: data-parallel training is not built; run it on one GPU')
        model = self.model.to(self.device)
        opts = self._optimizers(model)
        width = len(self.LOSS_TERMS)
        self.batch_losses = np.zeros((0, width))
        self.timer(start=True)
        epoch = -1
        for epoch in range(self.maxEpoch):
            model.train()
            rows = [self._step(model, opts, batch) for batch in self._epoch_batches()]
            terms = torch.stack(rows) if rows else torch.zeros((0, width))
            host = terms.cpu().numpy().astype(float)                # the epoch's one copy to the host
            for n in range(0, len(rows), 50):
                print('training:', epoch + 1, 'batch', n, 'batch_loss:', float(host[n, -1]))
            self.batch_losses = np.concatenate([self.batch_losses, host])
            with torch.no_grad():
                model.eval()
                self._set_tables('', self._current_tables())
                if epoch % self.eval_every == 0:
                    self.fast_evaluation(epoch, valid_type='all')
                    if self.early_stop_flag and self.early_stop_patience <= 0:
                        break
        self.epochs_ran = (epoch + 1) if self.maxEpoch > 0 else 0
        self.timer(start=False)
        model.eval()
        self._set_tables('', [getattr(self, 'best_' + name) for name in self.TABLES])
        if self.args.save_emb:
            a = self.args
            os.makedirs('./emb', exist_ok=True)
            stem = f'./emb/{a.dataset}_cold_{a.cold_object}_{a.model}'
            for name, last in (self.SAVE_FILES or {name: name for name in self.TABLES}).items():
                torch.save(getattr(self, name), f'{stem}_{last}.pt')

    def save(self):
        with torch.no_grad():
            self._set_tables('best_', self._current_tables())

    def predict(self, u):
        with torch.no_grad():
            return (self.item_emb @ self.user_emb[self.data.get_user_id(u)]).cpu().numpy()

    def batch_predict(self, users):
        with torch.no_grad():
            users = torch.as_tensor(self.data.get_user_id_list(users), device=self.device)
            return self.user_emb[users] @ self.item_emb.T
