"""NCL warm-embedding trainer on the MI355X (reference: model/NCL.py).

The reference's NCL cannot run where faiss is absent (its import fails) and stops at epoch 20 with a NameError in e_step;
its structure loss builds B x user_num and B x item_num logit matrices per batch and keeps both for autograd.  Here the
step is ``train.NCLEngine``: the LightGCN propagation with layer 2 * hyper_layers kept as the context table, fused BPR, the
structure contrast as two crh_table_nce_f32 calls (csrc/table_nce.hip: no logit matrix, dense table gradient), and one
backward chain of L SpMMs with the optimiser in the last one's epilogue.  Same random streams as the reference for the
tables and the triples.

The prototype phase starts at epoch ``--proto_start`` (the reference hard-codes 20).  Its clustering is this project's own
-- ``train.lloyd_kmeans``: 20 Lloyd iterations from ``--num_clusters`` rows drawn by a private CPU generator seeded with
``--seed``; an empty cluster keeps its centroid -- NOT faiss's k-means, so from that epoch on the run follows the reference's
formulas but not a run of it.
"""
import numpy as np
import torch

from .. import ops
from ..sampler import EpochPrefetcher
from ..train import NCLEngine, dp_from_env
from .LightGCN import LGCN_Encoder, LightGCN
from .MF import MF, _require_gpu


class NCL(LightGCN):
    fused_eval = True

    def __init__(self, config):
        super(MF, self).__init__(config)
        a = self.args
        self.n_layers = a.layers
        self.model = LGCN_Encoder(self.data, self.emb_size, self.n_layers, self.device)
        self.ssl_temp, self.ssl_reg, self.hyper_layers = a.tau, a.ssl_reg, a.hyper_layers
        if self.hyper_layers * 2 > self.n_layers:
            raise ValueError(
                "NCL expects emb_list[hyper_layers*2] with len(emb_list)==layers+1; "
                f"need hyper_layers*2 <= layers, got hyper_layers={self.hyper_layers}, layers={self.n_layers}."
            )
        if self.emb_size > 256:
            raise RuntimeError("NCL: embedding widths above 256 are not supported by the contrast kernels")
        self.alpha, self.proto_reg, self.k = a.alpha, a.proto_reg, a.num_clusters
        self.proto_start = getattr(a, 'proto_start', 20)
        self.engine = None

    def _make_engine(self):
        a = self.args
        rowptr, col, val = self.data.norm_adj_csr()
        return NCLEngine(self.model.user0, self.model.item0, rowptr, col, val, self.n_layers, self.lr, self.reg, self.device,
                         optimizer=getattr(a, 'optimizer', 'adam'), tau=self.ssl_temp, ssl_reg=self.ssl_reg,
                         alpha=self.alpha, hyper_layers=self.hyper_layers, proto_reg=self.proto_reg, num_clusters=self.k,
                         batch_size=self.batch_size, seed=getattr(a, 'seed', 0))

    def train(self):
        _require_gpu(self.device)
        if dp_from_env() is not None:
            raise RuntimeError('NCL: data-parallel training is not built; run it on one GPU')
        eng = self.engine = self._make_engine()
        B, n = self.batch_size, len(self.data.train_u)
        steps = [(lo, min(lo + B, n)) for lo in range(0, n, B)]
        losses = torch.zeros((len(steps), 6), dtype=torch.float32, device=self.device)
        triples = EpochPrefetcher(self.data.sampler, B, device=self.device)
        epoch = -1
        self.timer(start=True)
        try:
            for epoch in range(self.maxEpoch):
                if epoch == self.maxEpoch - 1:
                    triples.enabled = False            # nothing follows the last epoch
                warm_up = epoch < self.proto_start
                if not warm_up:
                    eng.e_step()
                u, i, j = triples.get()
                plans = ops.build_plans_device(u, i, j, B)         # deterministic BPR gradient rows
                for s, (lo, hi) in enumerate(steps):
                    eng.step(u[lo:hi], i[lo:hi], j[lo:hi], plans[s], losses[s])
                host = losses.cpu().numpy().astype(float)
                for s in range(0, len(steps), 50):
                    bpr, l2, ssl_u, ssl_i, p_u, p_i = host[s]
                    total = bpr + l2 + self.ssl_reg * (ssl_u + self.alpha * ssl_i) + self.proto_reg * B * (p_u + p_i)
                    print('training:', epoch + 1, 'batch', s, 'warm_up batch_loss:' if warm_up else 'batch_loss:',
                          float(total))
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
