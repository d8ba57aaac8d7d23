"""NGCF warm-embedding trainer on the MI355X (reference: model/NGCF.py).

The reference recomputes the L-layer propagation for every batch -- per layer a sparse product, two d x d Linear layers
over all user_num + item_num rows, an elementwise product and a leaky ReLU -- and lets autograd replay it.  Here a step is
``train.NGCFEngine``: the LightGCN engine's CSR SpMM, fused BPR and Adam around one fused HIP kernel per layer and
direction (csrc/ngcf.hip), which reads the two tables of a layer once and never writes x * s.  The dense layers are stepped
by stock ``torch.optim.Adam``.  Same random streams as the reference: xavier user table, xavier item table, then per layer
``W_gc`` and ``W_bi`` as ``nn.Linear`` on the CPU generator, and NumPy's global stream for the triples; the encoder's
``state_dict`` has the reference's keys.  ``save()`` keeps a real snapshot, as the reference's does.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..sampler import EpochPrefetcher
from ..train import NGCFEngine, dp_from_env
from .LightGCN import LightGCN
from .MF import MF, _check_width, _require_gpu


class NGCF_Encoder(nn.Module):
    """The reference's parameters in the reference's draw order and under its names (model/NGCF.py:78-88); kept on the
    CPU: the initial state the engine is built from, and after ``train()`` the trained one."""

    def __init__(self, data, emb_size, n_layers, device):
        super().__init__()
        self.data, self.latent_size, self.layers, self.device = data, emb_size, n_layers, device
        init = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({
            'user_emb': nn.Parameter(init(torch.empty(data.user_num, emb_size))),
            'item_emb': nn.Parameter(init(torch.empty(data.item_num, emb_size)))})
        self.W_gc = nn.ModuleList()
        self.W_bi = nn.ModuleList()
        for _ in range(n_layers):
            self.W_gc.append(nn.Linear(emb_size, emb_size))
            self.W_bi.append(nn.Linear(emb_size, emb_size))

    @property
    def user0(self):
        return self.embedding_dict['user_emb'].detach()

    @property
    def item0(self):
        return self.embedding_dict['item_emb'].detach()

    def weights(self):
        return [(self.W_gc[k].weight, self.W_gc[k].bias, self.W_bi[k].weight, self.W_bi[k].bias)
                for k in range(self.layers)]

    def load_engine(self, eng) -> None:
        """Copy the engine's trained tables and dense layers into the parameters."""
        with torch.no_grad():
            self.embedding_dict['user_emb'].copy_(eng.user_emb)
            self.embedding_dict['item_emb'].copy_(eng.item_emb)
            for k in range(self.layers):
                self.W_gc[k].weight.copy_(eng.W_gc[k])
                self.W_gc[k].bias.copy_(eng.b_gc[k])
                self.W_bi[k].weight.copy_(eng.W_bi[k])
                self.W_bi[k].bias.copy_(eng.b_bi[k])


class NGCF(LightGCN):
    fused_eval = True

    def __init__(self, config):
        super(MF, self).__init__(config)
        a = self.args
        _check_width('NGCF', '--emb_size', self.emb_size)
        if getattr(a, 'optimizer', 'adam') != 'adam':
            raise ValueError('NGCF: --optimizer sgd is not built (the dense layers are stepped by torch.optim.Adam, as the '
                             'reference steps them); use --optimizer adam')
        if getattr(a, 'lazy_adam', 'auto') == 'on':
            raise ValueError('NGCF: --lazy_adam on is not built (every row of the table moves in every step: the '
                             'propagation reaches all of them); use auto or off')
        self.n_layers = a.layers
        self.model = NGCF_Encoder(self.data, self.emb_size, self.n_layers, self.device)
        self.engine = None

    def _make_engine(self):
        rowptr, col, val = self.data.norm_adj_csr()
        return NGCFEngine(self.model.user0, self.model.item0, rowptr, col, val, self.n_layers, self.lr, self.reg,
                          self.device, self.model.weights(), optimizer=getattr(self.args, 'optimizer', 'adam'))

    def train(self):
        _require_gpu(self.device)
        if dp_from_env() is not None:
            raise RuntimeError('NGCF: data-parallel training is not built; run it on one GPU')
        eng = self.engine = self._make_engine()
        B, n = self.batch_size, len(self.data.train_u)
        steps = [(lo, min(lo + B, n)) for lo in range(0, n, B)]
        losses = torch.zeros((len(steps), 2), dtype=torch.float32, device=self.device)
        triples = EpochPrefetcher(self.data.sampler, B, device=self.device)
        epoch = -1
        self.timer(start=True)
        try:
            for epoch in range(self.maxEpoch):
                if epoch == self.maxEpoch - 1:
                    triples.enabled = False            # nothing follows the last epoch
                u, i, j = triples.get()
                plans = ops.build_plans_device(u, i, j, B)         # deterministic BPR gradient rows
                for s, (lo, hi) in enumerate(steps):
                    eng.step(u[lo:hi], i[lo:hi], j[lo:hi], plans[s], losses[s])
                host = losses.cpu().numpy().astype(float)
                for s in range(0, len(steps), 50):
                    print('training:', epoch + 1, 'batch', s, 'batch_loss:', float(host[s].sum()))
                self.batch_losses = host if epoch == 0 else np.concatenate([self.batch_losses, host])
                self.user_emb, self.item_emb = eng.forward()
                if epoch % self.eval_every == 0:
                    self.fast_evaluation(epoch, valid_type='all')
                    if self.early_stop_flag and self.early_stop_patience <= 0:
                        break
        finally:
            triples.close()
        self.model.load_engine(eng)
        self.epochs_ran = (epoch + 1) if self.maxEpoch > 0 else 0
        self.timer(start=False)
        self.user_emb, self.item_emb = self.best_user_emb, self.best_item_emb
        if self.args.save_emb:
            self._save_tables()
