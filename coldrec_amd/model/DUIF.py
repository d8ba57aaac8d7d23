"""DUIF cold-start trainer on the MI355X (reference: model/DUIF.py; Geng et al., "Learning Image and User Features for
Recommendation in Social Networks", ICCV 2015), for cold items and cold users.

One side has a learned table, the other is ``content @ W.T`` with W an ``nn.Linear(content_dim, emb_size, bias=False)``;
one BPR term over their product and the reference's Frobenius-norm regulariser.  DUIF loads no backbone.  Per batch the
reference projects the WHOLE content table and lets autograd replay the transposed product over the whole table, though
only the batch's rows carry gradient.  Here a step is one call of the fused HIP kernel (csrc/duif.hip, ``ops.duif``): it
gathers the batch's content rows, projects them on the fp32 MFMAs, forms the loss and writes the dense gradient of the
table and the gradient of W, deterministic, without atomics.  The step costs O(B c d) whatever the catalogue's size.  The
whole-table projection once per epoch, for evaluation, stays a stock ``content @ W.T``.

Same random streams as the reference run on the CPU: xavier_uniform_ for the user table, then for the item table, then
the nn.Linear; the table of the cold side is drawn and never trained, as in the reference.  One stock
``torch.optim.Adam(model.parameters(), lr)`` steps both parameters; dense Adam on the free table is the reference's
behaviour (a row no batch touches still moves by its moments).  The triples come from the MT19937-exact pairwise sampler.

The reference's best_* of the free table is the live parameter (its forward() returns it as it is), so a run whose best
epoch is not its last publishes the last epoch's free table beside the best epoch's projected table; here the best
epoch's two tables are copies.

One training step including Adam on the MI355X (tools/duif_step_ab.py: B = 2048, d = 64; three arms interleaved in one
process, median of 60 individually timed steps, ms; a second run of the process in brackets): (a) this trainer's step,
(b) the reference's formulation, which projects the whole content table per batch, (c) torch gathering first and
projecting the batch's rows only.  Item mode / user mode:
    toy (300 x 500, c = 16)              (a) 0.81 / 0.78 (0.85 / 0.86)  (b) 0.94 / 0.88 (1.03 / 1.02)  (c) 0.86 / 0.82 (0.94 / 0.94)
    MovieLens-sized (6040 x 3706, 206)   (a) 0.77 / 0.79 (0.86 / 0.84)  (b) 0.86 / 0.86 (1.02 / 0.95)  (c) 0.77 / 0.78 (0.93 / 0.86)
    CiteULike-sized (5551 x 16980, 300)  (a) 0.77 / 0.79 (0.81 / 0.82)  (b) 0.92 / 0.85 (0.99 / 0.93)  (c) 0.77 / 0.78 (0.84 / 0.84)
    10^6 content rows (c = 128)          (a) 0.79 / 0.81 (0.82 / 0.82)  (b) 2.58 / 2.44 (2.64 / 2.51)  (c) 0.79 / 0.81 (0.85 / 0.85)
(a) does not grow with the content rows, (b) does (3.0 - 3.3x of (a) at 10^6 rows, 1.1 - 1.2x below).  Against (c) the
fused step only ties (c / a = 0.99 - 1.11): both are bound by the host's launches, the plan's grouping of the free side's
ids among them -- supposed from the times' indifference to c and to d c, not profiled.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer
from .MF import _check_width, _require_gpu


def _check_flags(who, a):
    if getattr(a, 'optimizer', 'adam') != 'adam':
        raise ValueError(f'{who}: --optimizer sgd is not built (the table and the projection are stepped by one '
                         f'torch.optim.Adam, as the reference steps them); use --optimizer adam')
    if getattr(a, 'lazy_adam', 'auto') == 'on':
        raise ValueError(f'{who}: --lazy_adam on is not built (the reference\'s Adam is dense: a row no batch touches '
                         f'still moves by its moments); use auto or off')
    if getattr(a, 'shard_graph', False):
        raise ValueError(f'{who}: --shard_graph is not built (there is no graph to shard); run it on one GPU')


class _FusedLoss(torch.autograd.Function):
    """(total, loss3 = [L_bpr, R, total]) of one step; forward computes the two gradients with it, backward scales them."""

    @staticmethod
    def forward(ctx, table, w, content, plan, reg, cold_user, workspace):
        loss3, dt, dw, _ = ops.duif(table.detach(), content, w.detach(), plan, reg, cold_user=cold_user,
                                    want_table=table.requires_grad, want_w=w.requires_grad, workspace=workspace)
        ctx.grads = (dt, dw)
        ctx.mark_non_differentiable(loss3)
        return loss3[2].clone(), loss3

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return tuple(None if g is None else g * grad_out for g in ctx.grads) + (None,) * 5


class DUIF_Encoder(nn.Module):
    """The reference's parameters under the reference's state_dict keys: embedding_dict.user_emb, embedding_dict.item_emb
    and item_projector.weight (cold items) or user_projector.weight (cold users)."""

    def __init__(self, args, data, emb_size, device):
        super().__init__()
        self.args, self.data, self.latent_size, self.device = args, data, int(emb_size), device
        _check_width('DUIF', '--emb_size', self.latent_size)
        d = self.latent_size
        self.cold_user = args.cold_object == 'user'
        # the reference's draws in the reference's order (model/DUIF.py:71-85)
        init = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({'user_emb': nn.Parameter(init(torch.empty(data.user_num, d))),
                                                'item_emb': nn.Parameter(init(torch.empty(data.item_num, d)))})
        if self.cold_user:
            self.user_projector = nn.Linear(data.user_content_dim, d, bias=False)
            content = data.mapped_user_content
        else:
            self.item_projector = nn.Linear(data.item_content_dim, d, bias=False)
            content = data.mapped_item_content
        self.register_buffer('content', torch.as_tensor(np.asarray(content), dtype=torch.float32).contiguous(),
                             persistent=False)
        self.workspace = None
        self.last_terms = None        # device [L_bpr, R, total] of the last loss() call

    @property
    def table(self):
        """The trained table: the side without content."""
        return self.embedding_dict['item_emb' if self.cold_user else 'user_emb']

    @property
    def projector(self):
        return self.user_projector if self.cold_user else self.item_projector

    def loss(self, users, pos, neg, id_range=None):
        """The step's total loss (model/DUIF.py:21-23) of three (B,) id tensors: the fused kernel."""
        table, w = self.table, self.projector.weight
        if not table.is_cuda:
            _require_gpu(table.device)
        B = int(users.shape[0])
        plan = ops.duif_plan(users, pos, neg, self.cold_user, id_range=id_range)
        # one workspace (every id distinct) holds any step of this batch size or a shorter one
        need = ops.duif_workspace_bytes(B, self.latent_size, self.content.shape[1], self.cold_user, 2 * B if self.cold_user else B)
        if self.workspace is None or self.workspace.numel() < need or self.workspace.device != table.device:
            self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=table.device)
        total, self.last_terms = _FusedLoss.apply(table, w, self.content, plan, float(self.args.reg), self.cold_user,
                                                  self.workspace)
        return total

    def forward(self):
        """(user table, item table) as the reference's forward() has them, as copies."""
        proj = self.content @ self.projector.weight.T
        free = self.table.detach().clone()
        return (proj, free) if self.cold_user else (free, proj)


class DUIF(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('bpr', 'reg', 'batch_loss')

    def __init__(self, config):
        super().__init__(config)
        _check_flags('DUIF', self.args)
        self.model = DUIF_Encoder(self.args, self.data, self.emb_size, self.device)      # built on the CPU

    def _current_tables(self):
        user_emb, item_emb = self.model()
        return user_emb.detach().clone(), item_emb.detach().clone()
