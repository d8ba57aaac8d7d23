"""ALDI item-cold-start trainer on the MI355X (reference: model/ALDI.py; Huang et al., SIGIR 2023).

A frozen teacher -- the user and item tables a backbone run saved with ``--save_emb`` -- is distilled into two student
towers (Linear -> BatchNorm1d -> tanh -> Linear): the user tower maps a teacher user row, the item tower an item's content
row.  Per step the reference gathers three teacher rows per record, forms eight batched dot products and a B x B product
(for its row means), two weighted binary cross entropies, two absolute differences and a BPR term.  Here the towers stay
stock torch (two separate item-tower calls, BatchNorm statistics per call, as the reference has them) and everything after
them is one call of the fused HIP kernel (csrc/aldi.hip, ``ops.aldi``): the five loss terms and the gradients of the three
tower outputs, deterministic, without atomics.

Warm items are ranked with the teacher's user table and cold items with the generated one.  ``_eval_parts`` hands both
tables to the base class, which ranks each over the item table with the fused scoring kernel and merges the lists
(``BaseColdStartTrainer._topk_parts``); ``batch_predict`` computes the same composed block for everything else.

Same random streams as the reference: the towers are built on the CPU in its order (user tower first; every Linear draws
its default initialisation before ``trunc_normal_`` overwrites the weight), the triples come from the MT19937-exact
pairwise sampler.
"""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .FusedLossTrainer import FusedLossTrainer, load_backbone_tables
from .MF import _check_width, _require_gpu


def item_frequency(data):
    """Per internal item: the sum of 1 / |the user's training items| over the item's distinct training users; 1 for an
    item without training pairs (the reference's ``_aldi_item_frequency``), on the builder's arrays.  The pairs are taken
    in training order, duplicates dropped, and added one by one in float64, as the reference walks its dicts."""
    tu, ti = data.train_u.astype(np.int64), data.train_i.astype(np.int64)
    _, first = np.unique(tu * int(data.item_num) + ti, return_index=True)
    first.sort()
    tu, ti = tu[first], ti[first]
    per_user = np.maximum(np.diff(data.rated_rowptr), 1).astype(np.float64)
    acc = np.zeros(data.item_num, np.float64)
    np.add.at(acc, ti, 1.0 / per_user[tu])
    freq = np.ones(data.item_num, np.float32)
    seen = np.zeros(data.item_num, bool)
    seen[ti] = True
    freq[seen] = acc[seen]
    return freq


def pos_item_weights(data, freq_coef_M, tws):
    """The weight table of the two distillation terms: min(tanh(a freq), tanh(M)) with a = M / the expected frequency
    when ``tws``, else ones (reference model/ALDI.py:226-239).  A float32 CPU tensor."""
    train_n = max(len(data.training_data), 1)
    x_expect = (train_n / float(max(data.item_num, 1))) * (1.0 / max(train_n / float(max(data.user_num, 1)), 1e-12))
    a = float(freq_coef_M) / float(x_expect)
    freq = torch.tensor(item_frequency(data), dtype=torch.float32)
    if int(tws):
        return torch.clamp(torch.tanh(a * freq), 0.0, float(np.tanh(float(freq_coef_M))))
    return torch.ones_like(freq)


class ALDITower(nn.Module):
    def __init__(self, in_dim, hidden_dim, out_dim):
        super().__init__()
        self.fc1 = nn.Linear(in_dim, hidden_dim)
        self.bn = nn.BatchNorm1d(hidden_dim)
        self.fc2 = nn.Linear(hidden_dim, out_dim)
        for layer in (self.fc1, self.fc2):                  # the reference's module order
            nn.init.trunc_normal_(layer.weight, std=0.01)
            nn.init.zeros_(layer.bias)

    def forward(self, x):
        return self.fc2(torch.tanh(self.bn(self.fc1(x))))


class _FusedLoss(torch.autograd.Function):
    """loss5 = [L_bpr, L_rate, L_rank, L_iden, total] of one step; forward computes the three gradients with it, backward
    scales them.  The teacher tables get none."""

    @staticmethod
    def forward(ctx, gen_user, gen_pos, gen_neg, user_table, item_table, users, pos, neg, weight, coef, id_range):
        need = [gen_user.requires_grad, gen_pos.requires_grad, gen_neg.requires_grad]
        loss5, du, dp, dn = ops.aldi(user_table, item_table, users, pos, neg, gen_user.detach().contiguous(),
                                     gen_pos.detach().contiguous(), gen_neg.detach().contiguous(), weight, *coef,
                                     want_user=need[0], want_pos=need[1], want_neg=need[2], id_range=id_range)
        ctx.grads = (du, dp, dn)
        ctx.mark_non_differentiable(loss5)
        return loss5[4].clone(), loss5

    @staticmethod
    def backward(ctx, grad_out, _grad_terms):
        return tuple(None if g is None else g * grad_out for g in ctx.grads) + (None,) * 8


class ALDI_Learner(nn.Module):
    def __init__(self, args, data, emb_size, device):
        super().__init__()
        self.args, self.data, self.latent_size, self.device = args, data, emb_size, device
        _check_width('ALDI', '--emb_size', int(emb_size))
        content = torch.as_tensor(np.asarray(data.mapped_item_content), dtype=torch.float32)
        self.register_buffer('item_content', content, persistent=False)
        hidden = int(getattr(args, 'aldi_hidden', 200))
        self.user_tower = ALDITower(emb_size, hidden, emb_size)
        self.item_tower = ALDITower(data.item_content_dim, hidden, emb_size)
        tables = load_backbone_tables('ALDI', args, data, emb_size)
        self.register_buffer('user_emb', tables[0], persistent=False)        # the frozen teacher
        self.register_buffer('item_emb', tables[1], persistent=False)
        self.register_buffer('pos_item_weights',
                             pos_item_weights(data, args.freq_coef_M, getattr(args, 'tws', 0)), persistent=False)
        self.last_terms = None        # device [L_bpr, L_rate, L_rank, L_iden, total] of the last loss() call

    def param_groups(self, weight_decay):
        """The reference's two groups: L2 on the Linear weights and biases only, none on BatchNorm's scale and shift."""
        decay, no_decay = [], []
        for tower in (self.user_tower, self.item_tower):
            decay += [tower.fc1.weight, tower.fc1.bias, tower.fc2.weight, tower.fc2.bias]
            no_decay += [tower.bn.weight, tower.bn.bias]
        return [{'params': no_decay, 'weight_decay': 0.0}, {'params': decay, 'weight_decay': weight_decay}]

    def loss(self, users, pos, neg, id_range=None):
        """The step's total loss (model/ALDI.py:47-82) of three (B,) id tensors: the user tower on the teacher's user rows,
        the item tower on the positives' and -- in a call of its own -- the negatives' content, then the fused kernel."""
        if not self.user_emb.is_cuda:
            _require_gpu(self.user_emb.device)
        u, p, n = users.long(), pos.long(), neg.long()
        gen_user = self.user_tower(self.user_emb[u])
        gen_pos = self.item_tower(self.item_content[p])
        gen_neg = self.item_tower(self.item_content[n])
        a = self.args
        total, self.last_terms = _FusedLoss.apply(gen_user, gen_pos, gen_neg, self.user_emb, self.item_emb, users, pos, neg,
                                                  self.pos_item_weights, (float(a.alpha), float(a.beta), float(a.gamma)),
                                                  id_range)
        return total

    def generated_users(self):
        return self.user_tower(self.user_emb)

    def generated_items(self, idx):
        return self.item_tower(self.item_content[idx])


class ALDI(FusedLossTrainer):
    fused_eval = False       # batch_predict composes two products; the fused route is _eval_parts'
    LOSS_TERMS = ('L_bpr', 'L_rate', 'L_rank', 'L_iden', 'total')
    TABLES = ('warm_user_emb', 'cold_user_emb', 'item_emb')

    def __init__(self, config):
        super().__init__(config)
        if self.args.cold_object == 'user':
            raise Exception('Cold user is not supported in ALDI due to its specific design for item cold-start problem.')
        self.model = ALDI_Learner(self.args, self.data, self.emb_size, self.device)      # built on the CPU
        self._warm_idx = self._cold_idx = None

    def _item_sets(self):
        dev = self.model.item_emb.device
        if self._warm_idx is None or self._warm_idx.device != dev:
            self._warm_idx = torch.as_tensor(np.asarray(self.data.mapped_warm_item_idx), dtype=torch.long, device=dev)
            self._cold_idx = torch.as_tensor(np.asarray(self.data.mapped_cold_item_idx), dtype=torch.long, device=dev)
        return self._warm_idx, self._cold_idx

    def _optimizers(self, model):
        return [torch.optim.Adam(model.param_groups(self.reg), lr=self.lr)]

    def _current_tables(self):
        """(teacher users, generated users, teacher items with the cold rows generated) with the towers in eval mode."""
        m = self.model.eval()
        _, cold = self._item_sets()
        item_emb = m.item_emb.clone()
        if cold.numel():
            item_emb[cold] = m.generated_items(cold)
        return m.user_emb.clone(), m.generated_users().clone(), item_emb

    def _eval_parts(self):
        if getattr(self, 'warm_user_emb', None) is None:
            return None
        return [(self.warm_user_emb, self.data.mapped_cold_item_idx), (self.cold_user_emb, self.data.mapped_warm_item_idx)]

    def predict(self, u):
        with torch.no_grad():
            return self._compose(torch.as_tensor([self.data.get_user_id(u)], device=self.item_emb.device))[0].cpu().numpy()

    def batch_predict(self, users):
        with torch.no_grad():
            return self._compose(torch.as_tensor(self.data.get_user_id_list(users), device=self.item_emb.device))

    def _compose(self, users):
        """Warm items scored with the teacher's users, cold items with the generated ones; anything else stays 0."""
        warm, cold = self._item_sets()
        score = torch.zeros(users.shape[0], self.data.item_num, dtype=torch.float32, device=self.item_emb.device)
        score[:, warm] = self.warm_user_emb[users] @ self.item_emb[warm].T
        score[:, cold] = self.cold_user_emb[users] @ self.item_emb[cold].T
        return score
