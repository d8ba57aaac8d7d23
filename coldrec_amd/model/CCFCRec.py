"""CCFCRec item-cold-start trainer on the MI355X (reference: model/CCFCRec.py).

Per record the reference gathers 1 + P + P N + S item rows (246 with its defaults), builds several (B, P, N, d)
temporaries for norms, products and exponentials, and scatters as many gradient rows back with index_put.  Here the
attribute-attention encoder stays stock torch on the B rows of the batch and everything after it is one call of the fused
HIP kernel (csrc/ccfcrec.hip, ``ops.ccfcrec``): the five loss terms and the dense gradients of both tables and of the
encoder's output, deterministic, without atomics.  Same random streams as the reference: module construction order for
the tables, CPython's ``random`` and NumPy's generator for the samples (the C++ sampler).
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer, load_backbone_tables
from .MF import _check_width, _require_gpu


def _check_rows(args):
    P, N, S = int(args.positive_number), int(args.negative_number), int(args.self_neg_number)
    if min(P, N, S) < 1:
        raise ValueError('CCFCRec: --positive_number, --negative_number and --self_neg_number must be at least 1')
    rows, cap = ops.ccfcrec_rows(P, N, S), ops.ccfcrec_max_rows()
    if rows > cap:
        raise ValueError(f'CCFCRec: 1 + P + P N + S = {rows} item rows per record exceed the fused HIP loss\'s cap of {cap}')
    return P, N, S


class _FusedLoss(torch.autograd.Function):
    """loss5 = [L_c, L_s, L_r1, L_r2, total] of one step; forward computes the three gradients with it, backward scales
    them.  A table that does not require a gradient (frozen pretrained tables) is not given one by the kernel."""

    @staticmethod
    def forward(ctx, user_emb, item_emb, q, plan, tau, lambda1):
        need = [user_emb.requires_grad, item_emb.requires_grad, q.requires_grad]
        loss5, gu, gv, gq = ops.ccfcrec(user_emb.detach(), item_emb.detach(), q.detach().contiguous(), plan, tau, lambda1,
                                        want_user=need[0], want_item=need[1], want_q=need[2])
        ctx.grads = (gu, gv, gq)
        ctx.mark_non_differentiable(loss5)
        return loss5[4].clone(), loss5

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        gu, gv, gq = ctx.grads
        return (None if gu is None else gu * grad_out, None if gv is None else gv * grad_out,
                None if gq is None else gq * grad_out, None, None, None)


class CCFCRec_Learner(nn.Module):
    def __init__(self, args, data, emb_size, device):
        super().__init__()
        self.args, self.data, self.latent_size, self.device = args, data, emb_size, device
        content = torch.as_tensor(np.asarray(data.mapped_item_content), dtype=torch.float32)
        self.register_buffer('item_content', content, persistent=False)
        self.content_eps = 1e-8
        self.uses_missing_sentinel = float((content == -1).float().mean()) > 0.01     # a -1 marks a missing attribute
        # construction order = the reference's (model/CCFCRec.py:143-187): the global generator's stream fixes the
        # tables.  Uninitialised attribute tensors and tables first, then the two Linear layers (whose constructors
        # draw), then xavier_normal_ in the reference's order.
        A = int(args.attr_present_dim)
        self.attr_matrix = nn.Parameter(torch.empty(data.item_content_dim, A))
        self.attr_W1 = nn.Parameter(torch.empty(A, A))
        self.attr_b1 = nn.Parameter(torch.empty(A, 1))
        self.attr_W2 = nn.Parameter(torch.empty(A, 1))
        self.pretrained = bool(args.pretrain)
        if self.pretrained:
            update = bool(args.pretrain_update)
            tables = load_backbone_tables('CCFCRec --pretrain', args, data, save_flag='')
            self.user_embedding = nn.Parameter(tables[0], requires_grad=update)
            self.item_embedding = nn.Parameter(tables[1], requires_grad=update)
        else:
            self.user_embedding = nn.Parameter(torch.empty(data.user_num, int(args.implicit_dim)))
            self.item_embedding = nn.Parameter(torch.empty(data.item_num, int(args.implicit_dim)))
        _check_width('CCFCRec', '--implicit_dim', self.item_embedding.shape[1])
        self.gen_layer1 = nn.Linear(A, int(args.cat_implicit_dim))
        self.gen_layer2 = nn.Linear(int(args.cat_implicit_dim), self.item_embedding.shape[1])
        self.h = nn.LeakyReLU()
        for p in (self.attr_matrix, self.attr_W1, self.attr_W2, self.attr_b1):
            nn.init.xavier_normal_(p)
        if not self.pretrained:
            nn.init.xavier_normal_(self.user_embedding)
            nn.init.xavier_normal_(self.item_embedding)
        nn.init.xavier_normal_(self.gen_layer1.weight)
        nn.init.xavier_normal_(self.gen_layer2.weight)
        self.last_terms = None        # device [L_c, L_s, L_r1, L_r2, total] of the last loss() call

    def forward(self, u_idx, i_idx):
        """q_v_c of the items i_idx (model/CCFCRec.py:189-222): attention over the item's attributes, gated by their
        magnitude (for binary attributes: attention over the present ones); an item without an active attribute takes
        the plain attention weights.  u_idx only fixes the batch size, as in the reference."""
        attribute = self.item_content[i_idx]
        if self.uses_missing_sentinel:
            valid = attribute != -1
            value = attribute.masked_fill(~valid, 0.0)
        else:
            valid = torch.ones_like(attribute, dtype=torch.bool)
            value = attribute
        z_v = torch.matmul(torch.matmul(self.attr_matrix, self.attr_W1) + self.attr_b1.squeeze(), self.attr_W2).squeeze(dim=1)
        magnitude = value.abs()
        active = valid & (magnitude > self.content_eps)
        has_active = active.any(dim=1, keepdim=True)
        logits = z_v.unsqueeze(0).expand(u_idx.shape[0], -1) + torch.log(magnitude.clamp_min(self.content_eps))
        logits = logits.masked_fill(~torch.where(has_active, active, valid), -1e6)
        weight = torch.softmax(logits, dim=1)
        q_v_a = torch.matmul(torch.where(has_active, weight * value, weight), self.attr_matrix)
        return self.gen_layer2(self.h(self.gen_layer1(q_v_a)))

    def loss(self, u_idx, i_idx, neg_u_idx, pos_i, neg_i, self_neg):
        """The step's total loss (model/CCFCRec.py:53-87) of (B,), (B,), (B,), (B, P), (B, P, N), (B, S) id tensors."""
        U, V = self.user_embedding, self.item_embedding
        if not U.is_cuda:
            _require_gpu(U.device)
        plan = ops.ccfcrec_plan(u_idx, i_idx, neg_u_idx, pos_i, neg_i, self_neg, U.shape[0], V.shape[0])
        q = self.forward(u_idx, i_idx.long())
        total, self.last_terms = _FusedLoss.apply(U, V, q, plan, float(self.args.tau), float(self.args.lambda1))
        return total


class CCFCRec(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('L_c', 'L_s', 'L_r1', 'L_r2', 'total')
    UPLOAD_BATCHES = 16      # batches of ids uploaded at once (16 x 4096 records x 248 ids of the defaults are 65 MB)

    def __init__(self, config):
        super().__init__(config)
        if self.args.cold_object == 'user':
            raise Exception('Cold user is not supported in CCFCRec due to its specific design for item cold-start problem.')
        if not self.args.pretrain:
            _check_width('CCFCRec', '--implicit_dim', int(self.args.implicit_dim))
        self.shape = _check_rows(self.args)
        self.model = CCFCRec_Learner(self.args, self.data, self.emb_size, self.device)

    def _item_embeddings_for_eval(self):
        """The item table with the cold rows replaced by generated ones, as in the reference's inference."""
        item_emb = self.model.item_embedding.detach().clone()
        cold = torch.as_tensor(self.data.mapped_cold_item_idx, dtype=torch.long, device=item_emb.device)
        if cold.numel() == 0:
            return item_emb
        item_emb[cold] = self.model(cold, cold).detach()
        return item_emb

    def _current_tables(self):
        return self.model.user_embedding.detach().clone(), self._item_embeddings_for_eval()

    def _epoch_batches(self):
        s = self.data.sampler
        s.pull_python_state()
        s.pull_numpy_state()                        # (the positives come from NumPy's global stream)
        ep = s.epoch_ccfcrec(*self.shape)           # the whole epoch from the reference's streams, in one host call
        s.push_numpy_state()
        s.push_python_state()
        return self._block_batches(ep)
