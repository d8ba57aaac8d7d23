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
import os

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..train import dp_from_env
from ..util.utils import epoch_triples
from .BaseRecommender import BaseColdStartTrainer
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
        stem = f'./emb/{args.dataset}_cold_{args.cold_object}_{args.backbone}'
        paths = (stem + '_user_emb.pt', stem + '_item_emb.pt')
        for p in paths:
            if not os.path.isfile(p):
                raise FileNotFoundError(
                    f'GAR requires {p}. Train the backbone first '
                    f'(e.g. main.py --model {args.backbone} --dataset {args.dataset} '
                    f'--cold_object {args.cold_object} --save_emb true) or set --backbone to match '
                    f'existing files under ./emb/.')
        tables = [torch.load(p, map_location='cpu').detach().float().contiguous() for p in paths]
        if tables[0].shape != (data.user_num, emb_size) or tables[1].shape != (data.item_num, emb_size):
            raise ValueError(f'GAR: the tables under {stem}_*_emb.pt do not fit this dataset and --emb_size {emb_size}')
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


class GAR(BaseColdStartTrainer):
    fused_eval = True        # batch_predict below is the stock user_emb[users] @ item_emb.T

    def __init__(self, config):
        super().__init__(config)
        self.model = GAR_Learner(self.args, self.data, self.emb_size, self.device)      # built on the CPU
        self._cold_idx = None

    def _tables(self):
        """(user table, item table) with the cold object's cold rows generated; the generator in eval mode."""
        m = self.model
        if self._cold_idx is None:
            cold = self.data.mapped_cold_user_idx if m.cold_user else self.data.mapped_cold_item_idx
            self._cold_idx = torch.as_tensor(np.asarray(cold), dtype=torch.long, device=m.user_emb.device)
        user_emb, item_emb = m.user_emb.detach().clone(), m.item_emb.detach().clone()
        if self._cold_idx.numel():
            (user_emb if m.cold_user else item_emb)[self._cold_idx] = m.generated(self._cold_idx)
        return user_emb, item_emb

    def train(self):
        _require_gpu(self.device)
        if dp_from_env() is not None:
            raise RuntimeError('GAR: data-parallel training is not built; run it on one GPU')
        model = self.model.to(self.device)
        self._cold_idx = None
        optimizer = torch.optim.Adam(model.parameters(), lr=self.lr)
        B = self.batch_size
        self.batch_losses = np.zeros((0, 4))
        self.timer(start=True)
        epoch = -1
        for epoch in range(self.maxEpoch):
            model.train()
            ep = epoch_triples(self.data, B)            # the whole epoch from the reference's stream, one upload
            id_range = ((int(ep[0].min()), int(ep[0].max())),
                        (int(min(ep[1].min(), ep[2].min())), int(max(ep[1].max(), ep[2].max()))))
            eu, ei, ej = (torch.from_numpy(x).to(self.device) for x in ep)
            n_steps = (eu.shape[0] + B - 1) // B
            terms = torch.zeros((n_steps, 4), dtype=torch.float32, device=self.device)
            for n, lo in enumerate(range(0, eu.shape[0], B)):
                batch_loss = model.loss(eu[lo:lo + B], ei[lo:lo + B], ej[lo:lo + B], id_range)
                optimizer.zero_grad()
                batch_loss.backward()
                optimizer.step()
                terms[n] = model.last_terms
            host = terms.cpu().numpy().astype(float)
            for n in range(0, n_steps, 50):
                print('training:', epoch + 1, 'batch', n, 'batch_loss:', float(host[n, 3]))
            self.batch_losses = np.concatenate([self.batch_losses, host])
            with torch.no_grad():
                model.eval()
                self.user_emb, self.item_emb = self._tables()
                if epoch % self.eval_every == 0:
                    self.fast_evaluation(epoch, valid_type='all')
                    if self.early_stop_flag and self.early_stop_patience <= 0:
                        break
        self.epochs_ran = (epoch + 1) if self.maxEpoch > 0 else 0
        self.timer(start=False)
        model.eval()
        self.user_emb, self.item_emb = self.best_user_emb, self.best_item_emb
        if self.args.save_emb:
            a = self.args
            os.makedirs('./emb', exist_ok=True)
            stem = f'./emb/{a.dataset}_cold_{a.cold_object}_{a.model}'
            torch.save(self.user_emb, stem + '_user_emb.pt')
            torch.save(self.item_emb, stem + '_item_emb.pt')

    def save(self):
        with torch.no_grad():
            self.model.eval()
            self.best_user_emb, self.best_item_emb = self._tables()

    def predict(self, u):
        with torch.no_grad():
            return (self.item_emb @ self.user_emb[self.data.get_user_id(u)]).cpu().numpy()

    def batch_predict(self, users):
        with torch.no_grad():
            users = torch.as_tensor(self.data.get_user_id_list(users), device=self.device)
            return self.user_emb[users] @ self.item_emb.T
