"""MetaEmbedding cold-start trainer on the MI355X (reference: model/MetaEmbedding.py; Pan et al., SIGIR 2019), for cold
items and cold users.

A generator (one Linear, its output divided by 5) maps a content row to an embedding and is trained against the frozen
tables a backbone run saved with ``--save_emb``.  A step scores the 2B (user, item) pairs of a batch -- the B positives
with target 1, the B negatives with target 0 -- with the generated row in the cold object's place (loss_a), takes one
gradient step of ``cold_lr = lr / 10`` on the generated rows, scores again (loss_b) and minimises
``alpha loss_a + (1 - alpha) loss_b``; the inner gradient is a constant, as first-order MAML has it.  The reference does
that with six gathers, two forward passes, an ``autograd.grad`` call and the backward of all of it.  Here the generator
stays stock torch and everything after it is one call of the fused HIP kernel (csrc/metaemb.hip, ``ops.metaemb``): both
losses and the generated rows' gradient, deterministic, without atomics.  The tables are frozen and never copied per step.

After every epoch the cold rows of the item table (item mode) or of the user table (user mode) are replaced by the
generator's output in copies of the backbone tables, and evaluation is the base class's ordinary one-table fused ranking.

Same random streams as the reference: the generator is built on the CPU before the tables are loaded, the triples come
from the MT19937-exact pairwise sampler.

One step against the same step in float32 torch autograd on the MI355X (tools/metaemb_step_ab.py: B = 2048, d = 64,
content width 16, median of 60 steps after warm-up, two processes): 0.43 / 0.44 ms against 0.61 / 0.72 ms on the toy
tables (300 x 500), ratio 1.42 / 1.63; 0.39 / 0.43 ms against 0.61 / 0.70 ms on MovieLens-sized ones (6040 x 3706),
ratio 1.55 / 1.63.  The table size does not matter: at a few kilobytes per record both arms are bound by their launches,
and what is left of the fused step is the generator's Linear, its backward and Adam.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer, load_backbone_tables
from .MF import _check_width, _require_gpu


class _FusedLoss(torch.autograd.Function):
    """loss3 = [loss_a, loss_b, ME] of one step; forward computes the generated rows' gradient with it, backward scales it."""

    @staticmethod
    def forward(ctx, emb, table, ids, n_pos, alpha, cold_lr, id_range):
        loss3, grad, _ = ops.metaemb(table, ids, emb.detach().contiguous(), n_pos, alpha, cold_lr,
                                     want_grad=emb.requires_grad, id_range=id_range)
        ctx.grad = grad
        ctx.mark_non_differentiable(loss3)
        return loss3[2].clone(), loss3

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return (None if ctx.grad is None else ctx.grad * grad_out,) + (None,) * 6


class MetaEmbedding_Learner(nn.Module):
    def __init__(self, args, data, emb_size, device, cold_lr):
        super().__init__()
        self.args, self.data, self.emb_size, self.device, self.cold_lr = args, data, emb_size, device, float(cold_lr)
        _check_width('MetaEmbedding', '--emb_size', int(emb_size))
        self.cold_user = args.cold_object == 'user'
        content = data.mapped_user_content if self.cold_user else data.mapped_item_content
        self.register_buffer('content', torch.as_tensor(np.asarray(content), dtype=torch.float32), persistent=False)
        content_dim = data.user_content_dim if self.cold_user else data.item_content_dim
        self.emb_pred_Dense = nn.Linear(content_dim, emb_size)       # before the tables, as the reference draws it
        tables = load_backbone_tables('MetaEmbedding', args, data, emb_size)
        self.register_buffer('user_emb', tables[0], persistent=False)        # frozen
        self.register_buffer('item_emb', tables[1], persistent=False)
        self.last_terms = None        # device [loss_a, loss_b, ME] of the last loss() call

    def generated(self, idx):
        return self.emb_pred_Dense(self.content[idx]) / 5.

    def loss(self, users, pos, neg, id_range=None):
        """The step's ME loss (model/MetaEmbedding.py:28-44) of three (B,) id tensors: the generator on the 2B cold
        objects' content, then the fused kernel against the other side's frozen rows."""
        if not self.user_emb.is_cuda:
            _require_gpu(self.user_emb.device)
        uu, ii = torch.cat([users, users]), torch.cat([pos, neg])
        if self.cold_user:
            table, ids, own, r = self.item_emb, ii, uu, None if id_range is None else id_range[1]
        else:
            table, ids, own, r = self.user_emb, uu, ii, None if id_range is None else id_range[0]
        emb = self.generated(own.long())
        total, self.last_terms = _FusedLoss.apply(emb, table, ids, int(users.shape[0]), float(self.args.alpha),
                                                  self.cold_lr, r)
        return total


class MetaEmbedding(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('loss_a', 'loss_b', 'batch_loss')

    def __init__(self, config):
        super().__init__(config)
        self.model = MetaEmbedding_Learner(self.args, self.data, self.emb_size, self.device, self.args.lr / 10.)   # on the CPU
        self._cold_idx = None

    def _current_tables(self):
        """Copies of the two backbone tables with the cold object's cold rows generated; the generator in eval mode."""
        m = self.model.eval()
        if self._cold_idx is None or self._cold_idx.device != m.user_emb.device:
            cold = self.data.mapped_cold_user_idx if m.cold_user else self.data.mapped_cold_item_idx
            self._cold_idx = torch.as_tensor(np.asarray(cold), dtype=torch.long, device=m.user_emb.device)
        user_emb, item_emb = m.user_emb.detach().clone(), m.item_emb.detach().clone()
        if self._cold_idx.numel():
            (user_emb if m.cold_user else item_emb)[self._cold_idx] = m.generated(self._cold_idx).detach()
        return user_emb, item_emb
