"""DeepMusic cold-start trainer on the MI355X (reference: model/DeepMusic.py; van den Oord et al., NIPS 2013), for cold
items and cold users.

A content MLP (Linear -> ReLU -> Linear) is regressed onto the frozen rows of the tables a backbone run saved with
``--save_emb``: per step the mean squared difference between the generated rows of a batch's positives (item mode) or
users (user mode) and their backbone rows, plus ``reg |G|_F / B``.  The MLP stays stock torch and everything after it is
one call of the fused HIP kernel (csrc/deepmusic.hip, ``ops.deepmusic``): both loss terms and the generated rows' gradient
in three launches, deterministic, without atomics.  The tables are frozen and never copied per step.

After every epoch the cold rows of the item table (item mode) or of the user table (user mode) are replaced by the
MLP's output in copies of the backbone tables, and evaluation is the base class's ordinary one-table fused ranking.

Same random streams as the reference: the tables are loaded, then the MLP is built on the CPU; the triples come from the
MT19937-exact pairwise sampler (the negatives are drawn and not used, as in the reference).

One step against the same step in float32 torch autograd on the MI355X (tools/metaemb_step_ab.py: B = 2048, d = 64,
content width 16, median of 60 steps after warm-up, two processes): 0.46 / 0.53 ms against 0.56 / 0.56 ms on the toy
tables (300 x 500), ratio 1.22 / 1.06; 0.46 / 0.53 ms against 0.49 / 0.56 ms on MovieLens-sized ones (6040 x 3706),
ratio 1.06 / 1.06.  The fused step is barely faster: the reference's loss is a handful of small launches (a gather,
mse_loss, norm and their backward), and the step is bound by the launches of what stays stock torch -- the two Linear
layers with their ReLU, their backward and Adam over four parameters -- so three launches in the loss's place save
little.  (Launch counts were not profiled; the explanation rests on the times not moving with the table size.)
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer, load_backbone_tables
from .MF import _check_width, _require_gpu


class _FusedLoss(torch.autograd.Function):
    """loss3 = [mse, reg, total] of one step; forward computes the generated rows' gradient with it, backward scales it."""

    @staticmethod
    def forward(ctx, gen, table, ids, reg, id_range):
        loss3, grad = ops.deepmusic(table, ids, gen.detach().contiguous(), reg, want_grad=gen.requires_grad,
                                    id_range=id_range)
        ctx.grad = grad
        ctx.mark_non_differentiable(loss3)
        return loss3[2].clone(), loss3

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return (None if ctx.grad is None else ctx.grad * grad_out,) + (None,) * 4


class DeepMusic_Encoder(nn.Module):
    def __init__(self, args, data, emb_size, device, reg):
        super().__init__()
        self.args, self.data, self.latent_size, self.device, self.reg = args, data, emb_size, device, float(reg)
        _check_width('DeepMusic', '--emb_size', int(emb_size))
        self.cold_user = args.cold_object == 'user'
        tables = load_backbone_tables('DeepMusic', args, data, emb_size)     # before the MLP, as the reference has it
        self.register_buffer('user_emb', tables[0], persistent=False)        # frozen
        self.register_buffer('item_emb', tables[1], persistent=False)
        content_dim = data.user_content_dim if self.cold_user else data.item_content_dim
        self.transformation = nn.Sequential(nn.Linear(content_dim, 2 * emb_size), nn.ReLU(),
                                            nn.Linear(2 * emb_size, emb_size))
        content = data.mapped_user_content if self.cold_user else data.mapped_item_content
        self.register_buffer('content', torch.as_tensor(np.asarray(content), dtype=torch.float32), persistent=False)
        self.last_terms = None        # device [mse, reg, total] of the last loss() call

    def generated(self, idx):
        return self.transformation(self.content[idx])

    def loss(self, users, pos, neg, id_range=None):
        """The step's loss (model/DeepMusic.py:19-29) of three (B,) id tensors: the MLP on the positives' content (the
        users' in user mode), then the fused kernel against their frozen rows.  The negatives are not used."""
        if not self.user_emb.is_cuda:
            _require_gpu(self.user_emb.device)
        if self.cold_user:
            table, ids, r = self.user_emb, users, None if id_range is None else id_range[0]
        else:
            table, ids, r = self.item_emb, pos, None if id_range is None else id_range[1]
        total, self.last_terms = _FusedLoss.apply(self.generated(ids.long()), table, ids, self.reg, r)
        return total


class DeepMusic(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('mse', 'reg', 'batch_loss')

    def __init__(self, config):
        super().__init__(config)
        self.model = DeepMusic_Encoder(self.args, self.data, self.emb_size, self.device, self.reg)      # built on the CPU
        self._cold_idx = None

    def _current_tables(self):
        """Copies of the two backbone tables with the cold object's cold rows generated; the MLP in eval mode."""
        m = self.model.eval()
        if self._cold_idx is None or self._cold_idx.device != m.user_emb.device:
            cold = self.data.mapped_cold_user_idx if m.cold_user else self.data.mapped_cold_item_idx
            self._cold_idx = torch.as_tensor(np.asarray(cold), dtype=torch.long, device=m.user_emb.device)
        user_emb, item_emb = m.user_emb.detach().clone(), m.item_emb.detach().clone()
        if self._cold_idx.numel():
            (user_emb if m.cold_user else item_emb)[self._cold_idx] = m.generated(self._cold_idx).detach()
        return user_emb, item_emb
