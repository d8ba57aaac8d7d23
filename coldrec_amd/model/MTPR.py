"""MTPR cold-start trainer on the MI355X (reference: model/MTPR.py; Du et al., "How to Learn Item Representation for
Cold-Start Multimedia Recommendation?", MM 2020), for cold items and cold users.

Two id tables P, Q -- the cold object's d wide, the other one 2 d --, a content projection W and two (2 d, d) projections
weu, wei.  The cold object's representation is [id row | content row @ W], its counterfactual twin has the id half
zeroed; four BPR terms rank normal and counterfactual representations against each other.  Per step the reference calls
``predict`` / ``predict_z`` eight times, each gathering rows and projecting them again, and lets autograd replay it all.
Here ``content[ids] @ W`` stays stock torch and everything after it is one call of the fused HIP kernel (csrc/mtpr.hip,
``ops.mtpr``): the four terms, the tables' regulariser, the gradients of the content rows and of weu / wei, and the two
table gradients with duplicate ids summed in a fixed order, deterministic, without atomics.  The tables are stepped by
the touched-rows Adagrad kernel (``ops.adagrad_rows``, torch.optim.Adagrad's defaults: a zero gradient moves nothing, so
stepping the rows of the batch equals the reference's dense step); W, weu and wei by stock ``torch.optim.Adam``.  No
step makes a dense pass over a table: the gradient buffers are zeroed once, the loss writes the touched rows and the
Adagrad kernel clears them again.

After every epoch the two derived tables (P weu and [Q | C W] wei, or [P | C W] weu and Q wei) are computed in torch
and evaluated by the base class's one-table fused ranking.

Same random streams as the reference run on the CPU: the learner draws Embedding P (normal_, then xavier_uniform_),
Embedding Q, then randn + xavier_uniform_ for W, weu, wei on the CPU generator; the triples come from the MT19937-exact
pairwise sampler.  (The reference draws on its device: run on a GPU it would take the device generator's stream.  This
trainer always draws on the CPU, as the G25 fixture's runs do.)
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer
from .MF import _require_gpu


def _check_width(width):
    if width % 4 != 0 or width < 4 or width > 128:
        raise ValueError(f'MTPR: --emb_size {width} must be a multiple of 4 in [4, 128] (the fused HIP loss loads rows in '
                         f'16-byte pieces and the wide table, 2 x emb_size, is at most 256 columns)')


class _FusedLoss(torch.autograd.Function):
    """(sum, loss6 = [L_i, L_f, L_if, L_fi, R_emb, sum]) of one step.  Autograd sees the content rows h and weu, wei; the
    two table gradients are written by forward into the caller's buffers grad_user / grad_item at the touched rows, as the
    gradients of the sum itself (backward scales the other three by what arrives)."""

    @staticmethod
    def forward(ctx, h, weu, wei, user_table, item_table, plan, wd1, cold_user, grad_user, grad_item, workspace):
        need = [h.requires_grad, weu.requires_grad, wei.requires_grad]
        loss6, _, _, dh, dweu, dwei = ops.mtpr(
            user_table, item_table, h.detach().contiguous(), weu.detach(), wei.detach(), plan, wd1, cold_user=cold_user,
            want_user=False, want_item=False, want_h=need[0], want_weu=need[1], want_wei=need[2], grad_user=grad_user,
            grad_item=grad_item, workspace=workspace)
        ctx.grads = (dh, dweu, dwei)
        ctx.mark_non_differentiable(loss6)
        return loss6[5].clone(), loss6

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return tuple(None if g is None else g * grad_out for g in ctx.grads) + (None,) * 8


class MTPR_Learner(nn.Module):
    def __init__(self, args, data, emb_size, device):
        super().__init__()
        self.args, self.data, self.latent_size, self.device = args, data, int(emb_size), device
        _check_width(self.latent_size)
        d = self.latent_size
        self.cold_user = args.cold_object == 'user'
        content = data.mapped_user_content if self.cold_user else data.mapped_item_content
        self.register_buffer('content', torch.as_tensor(np.asarray(content), dtype=torch.float32), persistent=False)
        content_dim = data.user_content_dim if self.cold_user else data.item_content_dim
        init = nn.init.xavier_uniform_
        # the reference's draws in the reference's order (model/MTPR.py:87-112)
        self.P = nn.Embedding(data.user_num, d if self.cold_user else 2 * d)
        init(self.P.weight)
        self.Q = nn.Embedding(data.item_num, 2 * d if self.cold_user else d)
        init(self.Q.weight)
        self.W = nn.Parameter(init(torch.randn(content_dim, d, dtype=torch.float32)))
        self.weu = nn.Parameter(init(torch.randn(2 * d, d, dtype=torch.float32)))
        self.wei = nn.Parameter(init(torch.randn(2 * d, d, dtype=torch.float32)))
        # the tables are stepped by ops.adagrad_rows from buffers of their own, never through autograd
        self.P.weight.requires_grad_(False)
        self.Q.weight.requires_grad_(False)
        self.grad_user = self.grad_item = self.sum_user = self.sum_item = self.workspace = None
        self.last_terms = None        # device loss6 of the last loss() call
        self.last_plan = None

    def _step_buffers(self, batch):
        P, Q = self.P.weight, self.Q.weight
        if self.grad_user is None or self.grad_user.device != P.device:
            self.grad_user, self.grad_item = torch.zeros_like(P), torch.zeros_like(Q)
            self.sum_user, self.sum_item = torch.zeros_like(P), torch.zeros_like(Q)
            self.workspace = None
        need = ops.mtpr_workspace_bytes(batch, self.latent_size, self.cold_user, 2 * batch, batch)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=P.device)

    def loss(self, users, pos, neg, id_range=None):
        """The step's mtl_loss + the tables' part of regs (model/MTPR.py:181-202) of three (B,) id tensors: the content
        projection in torch, then the fused kernel.  Leaves the table gradients in grad_user / grad_item."""
        if not self.P.weight.is_cuda:
            _require_gpu(self.P.weight.device)
        self._step_buffers(int(users.shape[0]))
        plan = self.last_plan = ops.mtpr_plan(users, pos, neg, id_range=id_range)
        ids = users.long() if self.cold_user else torch.cat([pos.long(), neg.long()])
        h = self.content[ids] @ self.W
        total, self.last_terms = _FusedLoss.apply(h, self.weu, self.wei, self.P.weight, self.Q.weight, plan,
                                                  float(self.args.p_emb[1]), self.cold_user, self.grad_user, self.grad_item,
                                                  self.workspace)
        return total

    def weight_regs(self):
        """regs' part of the small tensors: wd2 (|W|^2 + |weu|^2) + wd3 |wei|^2."""
        wd2, wd3 = float(self.args.p_ctx[1]), float(self.args.p_proj[1])
        return wd2 * ((self.W * self.W).sum() + (self.weu * self.weu).sum()) + wd3 * (self.wei * self.wei).sum()

    def step_tables(self):
        """Adagrad over the rows the last loss() touched; clears the gradient rows it consumed."""
        lr1 = float(self.args.p_emb[0])
        ops.adagrad_rows(self.P.weight.data, self.grad_user, self.sum_user, self.last_plan['user_ids'], lr1)
        ops.adagrad_rows(self.Q.weight.data, self.grad_item, self.sum_item, self.last_plan['item_ids'], lr1)

    def forward(self):
        """(user_emb, item_emb) of model/MTPR.py:114-121."""
        cw = self.content @ self.W
        if self.cold_user:
            return torch.cat([self.P.weight, cw], 1) @ self.weu, self.Q.weight @ self.wei
        return self.P.weight @ self.weu, torch.cat([self.Q.weight, cw], 1) @ self.wei


class MTPR(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('L_i', 'L_f', 'L_if', 'L_fi', 'regs', 'batch_loss')

    def __init__(self, config):
        super().__init__(config)
        a = self.args
        if getattr(a, 'optimizer', 'adam') != 'adam':
            raise ValueError('MTPR: --optimizer sgd is not built (the tables are stepped by Adagrad and the projections by '
                             'torch.optim.Adam, as the reference steps them); use --optimizer adam')
        if getattr(a, 'lazy_adam', 'auto') == 'on':
            raise ValueError('MTPR: --lazy_adam on is not built (the tables are stepped by Adagrad over the touched rows '
                             'already); use auto or off')
        if getattr(a, 'shard_graph', False):
            raise ValueError('MTPR: --shard_graph is not built (there is no graph to shard); run it on one GPU')
        self.model = MTPR_Learner(a, self.data, self.emb_size, self.device)      # built on the CPU

    def _optimizers(self, model):
        a = self.args
        return [torch.optim.Adam([model.W, model.weu], lr=float(a.p_ctx[0])),
                torch.optim.Adam([model.wei], lr=float(a.p_proj[0]))]

    def _step(self, model, opts, batch):
        total = model.loss(*batch)
        rw = model.weight_regs()
        batch_loss = total + rw
        for opt in opts:
            opt.zero_grad()
        batch_loss.backward()
        model.step_tables()
        for opt in opts:
            opt.step()
        with torch.no_grad():
            t = model.last_terms
            return torch.cat([t[:4], (t[4] + rw).reshape(1), batch_loss.reshape(1)])

    def _current_tables(self):
        return self.model()
