"""CLCRec item-cold-start trainer on the MI355X (reference: model/CLCRec.py).

The reference gathers B (1 + num_neg) content rows through its encoder, builds about a dozen (B (1 + num_neg), d)
temporaries for two sampled softmaxes and a norm regulariser, and scatters as many gradient rows back with index_put.
Here the encoder (two stock Linear layers) runs once per DISTINCT item of the batch and everything after it is one call
of the fused HIP kernel (csrc/clcrec.hip, ``ops.clcrec``): loss terms and the dense gradients of both tables and of the
encoder's output, deterministic, without atomics.  Same random streams as the reference: module construction order for
the tables, CPython's ``random`` for the negatives (the C++ sampler), torch's CPU generator for the mixing index.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .FusedLossTrainer import FusedLossTrainer
from .MF import _check_width, _require_gpu


class _FusedLoss(torch.autograd.Function):
    """loss4 = [L1, L2, R, total] of one step; forward computes the three gradients with it, backward scales them."""

    @staticmethod
    def forward(ctx, user_emb, item_emb, feat, plan, mix_count, temp, lr_lambda, reg):
        need = [user_emb.requires_grad, item_emb.requires_grad, feat.requires_grad]
        loss4, gu, gv, ge = ops.clcrec(user_emb.detach(), item_emb.detach(), feat.detach().contiguous(), plan, mix_count,
                                       temp, lr_lambda, reg, want_user=need[0], want_item=need[1], want_feat=need[2])
        ctx.grads = (gu, gv, ge)
        ctx.mark_non_differentiable(loss4)
        return loss4[3].clone(), loss4

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        gu, gv, ge = ctx.grads
        return (None if gu is None else gu * grad_out, None if gv is None else gv * grad_out,
                None if ge is None else ge * grad_out, None, None, None, None, None)


class CLCRec_Learner(nn.Module):
    def __init__(self, args, data, emb_size, device):
        super().__init__()
        _check_width('CLCRec', '--emb_size', emb_size)
        self.args, self.data, self.latent_size, self.device = args, data, emb_size, device
        self.register_buffer('item_content', torch.as_tensor(np.asarray(data.mapped_item_content), dtype=torch.float32),
                             persistent=False)
        self.content_dim = data.item_content_dim
        # construction order = the reference's (model/CLCRec.py:88-96): the global generator's stream fixes the tables.
        # MLP, the attention weights, bias and att_sum_layer are never used by the loss; their gradients stay None.
        self.MLP = nn.Linear(emb_size, emb_size)
        self.encoder_layer1 = nn.Linear(self.content_dim, 256)
        self.encoder_layer2 = nn.Linear(256, emb_size)
        self.att_weight_1 = nn.Parameter(nn.init.kaiming_normal_(torch.rand((emb_size, emb_size))))
        self.att_weight_2 = nn.Parameter(nn.init.kaiming_normal_(torch.rand((emb_size, emb_size))))
        self.bias = nn.Parameter(nn.init.kaiming_normal_(torch.rand((emb_size, 1))))
        self.att_sum_layer = nn.Linear(emb_size, emb_size)
        self.num_sample = float(getattr(args, 'num_sample', 0.5))
        init = nn.init.xavier_uniform_
        self.embedding_dict = nn.ParameterDict({
            'user_emb': nn.Parameter(init(torch.empty(data.user_num, emb_size))),
            'item_emb': nn.Parameter(init(torch.empty(data.item_num, emb_size)))})
        self.last_terms = None        # device [L1, L2, R, total] of the last loss() call
        self.first_index_crc = None   # checksum of the first mixing index drawn (parity checks)

    def encoder(self, idx=None):
        feature = self.item_content if idx is None else self.item_content[idx]
        return self.encoder_layer2(F.leaky_relu(self.encoder_layer1(feature)))

    def mix_counts(self, n_rows):
        """The reference's ``torch.randint(M, (int(M * num_sample),))`` on the CPU generator, as per-row counts."""
        rand_index = torch.randint(n_rows, (int(n_rows * self.num_sample),))
        if self.first_index_crc is None:
            import zlib
            self.first_index_crc = zlib.crc32(rand_index.numpy().tobytes())
        return torch.bincount(rand_index, minlength=n_rows).to(torch.int32)

    def loss(self, user_tensor, item_tensor):
        """user_tensor (B,) or (B, 1 + num_neg) (the reference repeats the user per item), item_tensor (B, 1 + num_neg)."""
        U, V = self.embedding_dict['user_emb'], self.embedding_dict['item_emb']
        if not U.is_cuda:
            _require_gpu(U.device)
        if user_tensor.dim() == 2:
            user_tensor = user_tensor[:, 0]
        plan = ops.clcrec_plan(user_tensor, item_tensor, U.shape[0], V.shape[0])
        counts = self.mix_counts(item_tensor.numel()).to(U.device)
        feat = self.encoder(plan['slot_item'].long())
        a = self.args
        total, self.last_terms = _FusedLoss.apply(U, V, feat, plan, counts, float(a.temp_value), float(a.lr_lambda),
                                                  float(a.reg))
        return total

    def get_all_embs(self):
        feature = self.encoder()
        return self.embedding_dict['user_emb'], self.embedding_dict['item_emb'], feature[self.data.mapped_cold_item_idx]


class CLCRec(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('L1', 'L2', 'R', 'total')
    UPLOAD_BATCHES = 64      # batches of ids uploaded at once (an epoch of 800 k records x 129 ids is 413 MB)

    def __init__(self, config):
        super().__init__(config)
        if self.args.cold_object == 'user':
            raise Exception('Cold user is not supported in CLCRec due to its specific design for item cold-start problem.')
        _check_width('CLCRec', '--emb_size', self.emb_size)
        self.model = CLCRec_Learner(self.args, self.data, self.emb_size, self.device)

    def _current_tables(self):
        u, i, cold = self.model.get_all_embs()
        u, i = u.detach().clone(), i.detach().clone()
        i[torch.as_tensor(self.data.mapped_cold_item_idx, dtype=torch.long, device=i.device)] = cold
        return u, i

    def _epoch_batches(self):
        s = self.data.sampler
        s.pull_python_state()
        eu, ei = s.epoch_clcrec(int(self.args.num_neg))    # the whole epoch from the reference's stream, in one host call
        s.push_python_state()
        return self._block_batches((eu, ei))
