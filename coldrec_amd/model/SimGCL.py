"""SimGCL warm-embedding trainer on the MI355X (reference: model/SimGCL.py).

The reference runs three full-graph propagations per batch -- a clean one for the BPR loss and two perturbed views for the
InfoNCE term (model/SimGCL.py:25-29,53-60) -- and lets autograd replay all of them transposed.  Here the step is
``train.CLEngine``: 3L forward SpMMs, the perturbation as its own HIP kernel (csrc/perturb.hip), fused BPR / InfoNCE, and
ONE backward chain of L SpMMs for all three passes.  Same random streams as the reference for the tables and the triples;
the noise is generated on the device by default and drawn from torch's CPU generator with ``--cl_noise host``.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..sampler import EpochPrefetcher
from ..train import CLEngine, dp_from_env
from .LightGCN import LightGCN
from .MF import MF, _require_gpu


class SimGCL_Encoder(object):
    """Xavier tables (user first, model/SimGCL.py:93-99) + the normalised adjacency."""

    def __init__(self, args, data, emb_size, n_layers, device):
        self.args, self.data, self.eps = args, data, args.eps
        self.emb_size, self.n_layers, self.device = emb_size, n_layers, device
        init = nn.init.xavier_uniform_
        self.user0 = init(torch.empty(data.user_num, emb_size))
        self.item0 = init(torch.empty(data.item_num, emb_size))
        self.norm_adj = data.norm_adj


class SimGCL(LightGCN):
    fused_eval = True
    cl_mode = 'simgcl'

    def __init__(self, config):
        super(MF, self).__init__(config)
        self.n_layers = self.args.layers
        self.model = self._make_encoder()
        self.engine = None

    def _make_encoder(self):
        return SimGCL_Encoder(self.args, self.data, self.emb_size, self.n_layers, self.device)

    def _make_engine(self):
        a = self.args
        rowptr, col, val = self.data.norm_adj_csr()
        return CLEngine(self.model.user0, self.model.item0, rowptr, col, val, self.n_layers, self.lr, self.reg, self.device,
                        optimizer=getattr(a, 'optimizer', 'adam'), mode=self.cl_mode, eps=a.eps, tau=a.tau,
                        cl_rate=a.cl_rate, l_cl=getattr(a, 'l_cl', 1), noise=getattr(a, 'cl_noise', 'device'),
                        seed=getattr(a, 'seed', 0))

    def train(self):
        _require_gpu(self.device)
        if dp_from_env() is not None:
            raise RuntimeError(f'{type(self).__name__}: data-parallel training is not built; run it on one GPU')
        eng = self.engine = self._make_engine()
        B, n = self.batch_size, len(self.data.train_u)
        steps = [(lo, min(lo + B, n)) for lo in range(0, n, B)]
        losses = torch.zeros((len(steps), 4), dtype=torch.float32, device=self.device)
        triples = EpochPrefetcher(self.data.sampler, B, device=self.device)
        epoch = -1
        self.timer(start=True)
        try:
            for epoch in range(self.maxEpoch):
                if epoch == self.maxEpoch - 1:
                    triples.enabled = False            # nothing follows the last epoch
                u, i, j = triples.get()
                plans = ops.build_plans_device(u, i, j, B)         # deterministic BPR gradient rows
                for s, (lo, hi) in enumerate(steps):               # eager: torch.unique sizes each contrastive batch
                    eng.step(u[lo:hi], i[lo:hi], j[lo:hi], plans[s], losses[s])
                host = losses.cpu().numpy().astype(float)
                for s in range(0, len(steps), 50):
                    bpr, l2, cl_u, cl_i = host[s]
                    print('training:', epoch + 1, 'batch', s, 'batch_loss:', float(bpr + l2 + eng.cl_rate * (cl_u + cl_i)))
                self.batch_losses = host if epoch == 0 else np.concatenate([self.batch_losses, host])
                self.user_emb, self.item_emb = eng.forward()
                if epoch % self.eval_every == 0:
                    self.fast_evaluation(epoch, valid_type='all')
                    if self.early_stop_flag and self.early_stop_patience <= 0:
                        break
        finally:
            triples.close()
        self.epochs_ran = (epoch + 1) if self.maxEpoch > 0 else 0
        self.timer(start=False)
        self.user_emb, self.item_emb = self.best_user_emb, self.best_item_emb
        if self.args.save_emb:
            self._save_tables()
