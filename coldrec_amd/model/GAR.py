"""GAR cold-start trainer on the MI355X (reference: model/GAR.py; Chen et al., SIGIR 2022), for cold items and cold users.

A generator (Linear -> tanh -> Linear -> tanh) maps a content row to an embedding and is trained against the recommender:
the two tables a backbone run saved with ``--save_emb``, which GAR goes on training.  Per step the reference gathers three
table rows per record, runs the generator on the positives' content (item mode) or the users' (user mode) and forms
three batched BPR terms, a mean squared difference and four Frobenius norms.  Here the generator stays stock torch and
everything after it is one call of the fused HIP kernel (csrc/gar.hip, ``ops.gar``): the loss terms, the generator
output's gradient and the two dense table gradients with duplicate ids summed in a fixed order, deterministic, without
atomics.

After every epoch the cold rows of the item table (item mode) or of the user table (user mode) are replaced by the
generator's output, and evaluation is the base class's ordinary one-table fused ranking.

Same random streams as the reference: the generator is built on the CPU before the tables are loaded, the triples come
from the MT19937-exact pairwise sampler.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer, load_backbone_tables
from .MF import _check_width, _require_gpu


class _FusedLoss(torch.autograd.Function):
    """loss4 = [L_gen, L_rec, R, total] of one step; forward computes the three gradients with it, backward scales them."""

    @staticmethod
    def forward(ctx, gen, user_table, item_table, plan, coef, cold_user):
        need = [gen.requires_grad, user_table.requires_grad, item_table.requires_grad]
        loss4, du, di, dg = ops.gar(user_table.detach(), item_table.detach(), gen.detach().contiguous(), plan, *coef,
                                    cold_user=cold_user, want_gen=need[0], want_user=need[1], want_item=need[2])
        ctx.grads = (dg, du, di)
        ctx.mark_non_differentiable(loss4)
        return loss4[3].clone(), loss4

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return tuple(None if g is None else g * grad_out for g in ctx.grads) + (None,) * 3


class GAR_Learner(nn.Module):
    def __init__(self, args, data, emb_size, device):
        super().__init__()
        self.args, self.data, self.latent_size, self.device = args, data, emb_size, device
        _check_width('GAR', '--emb_size', int(emb_size))
        self.cold_user = args.cold_object == 'user'
        content = data.mapped_user_content if self.cold_user else data.mapped_item_content
        self.register_buffer('content', torch.as_tensor(np.asarray(content), dtype=torch.float32), persistent=False)
        content_dim = data.user_content_dim if self.cold_user else data.item_content_dim
        self.generator = nn.Sequential(nn.Linear(content_dim, 2 * emb_size), nn.Tanh(),
                                       nn.Linear(2 * emb_size, emb_size), nn.Tanh())
        tables = load_backbone_tables('GAR', args, data, emb_size)
        self.user_emb = nn.Parameter(tables[0].clone())       # trained, as the reference's ParameterDict has them
        self.item_emb = nn.Parameter(tables[1].clone())
        self.last_terms = None        # device [L_gen, L_rec, R, total] of the last loss() call

    def loss(self, users, pos, neg, id_range=None):
        """The step's total loss (model/GAR.py:24-31) of three (B,) id tensors: the generator on the positives' content
        (the users' in user mode), then the fused kernel."""
        if not self.user_emb.is_cuda:
            _require_gpu(self.user_emb.device)
        plan = ops.gar_plan(users, pos, neg, id_range=id_range)
        gen = self.generator(self.content[(users if self.cold_user else pos).long()])
        a = self.args
        total, self.last_terms = _FusedLoss.apply(gen, self.user_emb, self.item_emb, plan,
                                                  (float(a.alpha), float(a.beta), float(a.reg)), self.cold_user)
        return total

    def generated(self, idx):
        return self.generator(self.content[idx])


class GAR(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('L_gen', 'L_rec', 'R', 'total')

    def __init__(self, config):
        super().__init__(config)
        self.model = GAR_Learner(self.args, self.data, self.emb_size, self.device)      # built on the CPU
        self._cold_idx = None

    def _current_tables(self):
        """(user table, item table) with the cold object's cold rows generated; the generator in eval mode."""
        m = self.model.eval()
        if self._cold_idx is None or self._cold_idx.device != m.user_emb.device:
            cold = self.data.mapped_cold_user_idx if m.cold_user else self.data.mapped_cold_item_idx
            self._cold_idx = torch.as_tensor(np.asarray(cold), dtype=torch.long, device=m.user_emb.device)
        user_emb, item_emb = m.user_emb.detach().clone(), m.item_emb.detach().clone()
        if self._cold_idx.numel():
            (user_emb if m.cold_user else item_emb)[self._cold_idx] = m.generated(self._cold_idx)
        return user_emb, item_emb
