"""VBPR cold-start trainer on the MI355X (reference: model/VBPR.py; He & McAuley, "VBPR: Visual Bayesian Personalized
Ranking from Implicit Feedback", AAAI 2016), for cold items and cold users.

Two towers: the id tower <P[u], Q[i]> on the backbone's saved tables, and the content tower <PQ2[u], C[i] W> (cold items)
or <C[u] W, PQ2[i]> (cold users); one BPR term over their sum.  Per step the reference gathers the same rows two to six
times and lets autograd scatter them back with atomics.  Here ``content[ids] @ W`` stays stock torch and everything
after it is one call of the fused HIP kernel (csrc/vbpr.hip, ``ops.vbpr``): the term, the tables' regulariser, the
gradient of the content rows and the three table gradients with duplicate ids summed in a fixed order, deterministic,
without atomics.  P, Q and PQ2 are stepped by the touched-rows Adagrad kernel (``ops.adagrad_rows``), W by stock
``torch.optim.Adam``.  No step makes a dense pass over a table.

It publishes the reference's five tensors (user_emb_main, item_emb_main, user_emb_aux, item_emb_aux, w_value; saved by
``--save_emb`` under the reference's file names, so either implementation's files feed the other's AMR) and, for
ranking, user_emb = [main | aux] and item_emb = [main | aux], whose product is score1 + score2: the base class's
one-table fused ranking applies as it stands.

Same random streams as the reference run on the CPU: the Embeddings P, Q and PQ2 draw normal_ (P's and Q's draws are
overwritten by the loaded tables but advance the generator), PQ2 xavier_uniform_, then randn + xavier_uniform_ for W;
the triples come from the MT19937-exact pairwise sampler.

The reference's best_* of P, Q, PQ2 and W are the live parameters (its forward() returns them as they are), so a run
whose best epoch is not its last publishes the last epoch's values beside the best epoch's content rows; here the best
epoch's five tensors are copies.

One training step on the MI355X (tools/vbpr_step_ab.py: B = 2048, d = 64, content width 16; median of 60 steps), this
trainer's step against the same step in float32 torch (autograd, torch.optim.Adagrad / Adam) on the GPU: 1.38 ms against
1.45 ms on the toy tables (300 x 500; ratio 1.05), 1.40 ms against 1.30 ms on MovieLens-sized ones (6040 x 3706; ratio
0.92).  Neither time moves at B = 16384: both steps are bound by the host's launches, the plan's grouping of the ids
among them.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import VBPR_FILES, FusedLossTrainer, load_backbone_tables
from .MF import _require_gpu


def _check_width(who, width):
    if width % 4 != 0 or width < 4 or width > 128:
        raise ValueError(f'{who}: --emb_size {width} must be a multiple of 4 in [4, 128] (the fused HIP loss loads rows in '
                         f'16-byte pieces and the ranked tables, 2 x emb_size, are at most 256 columns)')


def _check_flags(who, a):
    if getattr(a, 'optimizer', 'adam') != 'adam':
        raise ValueError(f'{who}: --optimizer sgd is not built (the tables are stepped by Adagrad and the projection by '
                         f'torch.optim.Adam, as the reference steps them); use --optimizer adam')
    if getattr(a, 'lazy_adam', 'auto') == 'on':
        raise ValueError(f'{who}: --lazy_adam on is not built (the tables are stepped by Adagrad over the touched rows '
                         f'already); use auto or off')
    if getattr(a, 'shard_graph', False):
        raise ValueError(f'{who}: --shard_graph is not built (there is no graph to shard); run it on one GPU')


class _FusedLoss(torch.autograd.Function):
    """(sum, loss4 = [L_bpr, L_adv, R_emb, sum], grad_hsum or None) of one step.  Autograd sees the content rows h and
    h_adv (None: VBPR); the three table gradients are written by forward into the caller's buffers at the touched rows,
    as the gradients of the sum itself (backward scales the content rows' by what arrives)."""

    @staticmethod
    def forward(ctx, h, h_adv, user_table, item_table, aux_table, plan, wd1, lmd, cold_user, grad_user, grad_item,
                grad_aux, workspace, want_hsum):
        adv = None if h_adv is None else h_adv.detach().contiguous()
        loss4, _, _, _, dh, dh_adv, hsum = ops.vbpr(
            user_table, item_table, aux_table, h.detach().contiguous(), plan, wd1, h_adv=adv, lmd=lmd,
            cold_user=cold_user, want_user=False, want_item=False, want_aux=False, want_h=h.requires_grad,
            want_h_adv=h_adv is not None and h_adv.requires_grad, want_hsum=want_hsum, grad_user=grad_user,
            grad_item=grad_item, grad_aux=grad_aux, workspace=workspace)
        ctx.grads = (dh, dh_adv)
        ctx.mark_non_differentiable(loss4)
        if hsum is None:
            return loss4[3].clone(), loss4
        ctx.mark_non_differentiable(hsum)
        return loss4[3].clone(), loss4, hsum

    @staticmethod
    def backward(ctx, grad_out, *_unused):
        return tuple(None if g is None else g * grad_out for g in ctx.grads) + (None,) * 12


class VBPR_Learner(nn.Module):
    """P, Q, PQ2, W and the step's buffers; ``tensors`` = (P, Q, PQ2, W) to start from (AMR: VBPR's saved ones), None:
    the backbone's tables and the reference's draws."""

    def __init__(self, args, data, emb_size, device, tensors=None, who='VBPR'):
        super().__init__()
        self.args, self.data, self.latent_size, self.device = args, data, int(emb_size), device
        _check_width(who, self.latent_size)
        d = self.latent_size
        self.cold_user = args.cold_object == 'user'
        content = data.mapped_user_content if self.cold_user else data.mapped_item_content
        self.register_buffer('content', torch.as_tensor(np.asarray(content), dtype=torch.float32), persistent=False)
        content_dim = data.user_content_dim if self.cold_user else data.item_content_dim
        if tensors is None:
            p, q = load_backbone_tables(who, args, data, d)
            # the reference's draws in the reference's order (model/VBPR.py:91-114)
            self.P = nn.Embedding(data.user_num, d)
            self.Q = nn.Embedding(data.item_num, d)
            self.PQ2 = nn.Embedding(data.item_num if self.cold_user else data.user_num, d)
            nn.init.xavier_uniform_(self.PQ2.weight)
            self.W = nn.Parameter(nn.init.xavier_uniform_(torch.randn(content_dim, d, dtype=torch.float32)))
            with torch.no_grad():
                self.P.weight.copy_(p)
                self.Q.weight.copy_(q)
        else:
            p, q, pq2, w = tensors
            self.P, self.Q = nn.Embedding(data.user_num, d, _weight=p.clone()), nn.Embedding(data.item_num, d, _weight=q.clone())
            self.PQ2 = nn.Embedding(pq2.shape[0], d, _weight=pq2.clone())
            self.W = nn.Parameter(w.clone())
        # the tables are stepped by ops.adagrad_rows from buffers of their own, never through autograd
        for t in (self.P, self.Q, self.PQ2):
            t.weight.requires_grad_(False)
        self.grads = self.sums = self.workspace = None
        self.last_terms = None        # device loss4 of the last loss() call
        self.last_plan = None

    def tables(self):
        return self.P.weight, self.Q.weight, self.PQ2.weight

    def _step_buffers(self, batch):
        tables = self.tables()
        if self.grads is None or self.grads[0].device != tables[0].device:
            self.grads = [torch.zeros_like(t) for t in tables]
            self.sums = [torch.zeros_like(t) for t in tables]
            self.workspace = None
        need = ops.vbpr_workspace_bytes(batch, self.latent_size, self.cold_user, 2 * batch, batch)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(max(need, 1), dtype=torch.uint8, device=tables[0].device)

    def plan(self, users, pos, neg, id_range=None):
        """The step's plan and the rows of ``content`` its projections take, one per occurrence."""
        if not self.P.weight.is_cuda:
            _require_gpu(self.P.weight.device)
        self._step_buffers(int(users.shape[0]))
        self.last_plan = ops.vbpr_plan(users, pos, neg, id_range=id_range)
        return self.last_plan, users.long() if self.cold_user else torch.cat([pos.long(), neg.long()])

    def fused(self, plan, h, h_adv=None, lmd=1.0, want_hsum=False):
        """bpr_training + the tables' part of regs (model/VBPR.py:136-165) from the content projections: the fused kernel.
        Leaves the table gradients in ``grads``; returns (sum, grad_hsum or None)."""
        out = _FusedLoss.apply(h, h_adv, *self.tables(), plan, float(self.args.p_emb[1]), float(lmd), self.cold_user,
                               *self.grads, self.workspace, want_hsum)
        self.last_terms = out[1]
        return out[0], (out[2] if want_hsum else None)

    def loss(self, users, pos, neg, id_range=None):
        plan, ids = self.plan(users, pos, neg, id_range)
        return self.fused(plan, self.content[ids] @ self.W)[0]

    def weight_regs(self):
        """regs' part of W: wd2 |W|^2."""
        return float(self.args.p_ctx[1]) * (self.W * self.W).sum()

    def step_tables(self):
        """Adagrad over the rows the last step touched; clears the gradient rows it consumed."""
        lr1, plan = float(self.args.p_emb[0]), self.last_plan
        aux_ids = plan['item_ids'] if self.cold_user else plan['user_ids']
        for t, g, s, ids in zip(self.tables(), self.grads, self.sums, (plan['user_ids'], plan['item_ids'], aux_ids)):
            ops.adagrad_rows(t.data, g, s, ids, lr1)

    def forward(self):
        """The reference's five tensors (model/VBPR.py:116-125), as copies, and the concatenated pair that is ranked."""
        cw = self.content @ self.W
        p, q, a, w = (t.detach().clone() for t in (*self.tables(), self.W))
        user_aux, item_aux = (cw, a) if self.cold_user else (a, cw)
        return p, q, user_aux, item_aux, w, torch.cat([p, user_aux], 1), torch.cat([q, item_aux], 1)


class VBPR(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('bpr', 'regs', 'batch_loss')
    TABLES = tuple(VBPR_FILES) + ('user_emb', 'item_emb')
    SAVE_FILES = VBPR_FILES

    def __init__(self, config):
        super().__init__(config)
        _check_flags('VBPR', self.args)
        self.model = VBPR_Learner(self.args, self.data, self.emb_size, self.device)      # built on the CPU

    def _optimizers(self, model):
        return [torch.optim.Adam([model.W], lr=float(self.args.p_ctx[0]))]

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
            return torch.stack([t[0], t[2] + rw, batch_loss.detach()])

    def _current_tables(self):
        return self.model()
