"""AMR cold-start trainer on the MI355X (reference: model/AMR.py; Tang et al., "Adversarial Training Towards Robust
Multimedia Recommender System", TKDE 2019), for cold items.

VBPR's two towers, started from a VBPR run's five saved tensors, trained on the BPR term plus lmd times the same term
with the items' content perturbed by eps times the row-normalised noise.  The reference's noise is
``item_content.grad``, which is never cleared and which both ``backward()`` calls of a step add to: step t perturbs with
the sum of all content gradients of the steps before it plus step t's plain-loss gradient.  That running sum is what is
kept here, in a persistent (item_num, content_dim) buffer that no step clears:

    1  h = C[ids] @ W
    2  ``ops.vbpr`` asked for nothing but grad_hsum (the plain term's content gradients summed per distinct item):
       noise[item_ids] += hsum @ W^T                      (distinct rows: deterministic)
    3  h_adv = (C[ids] + eps normalize(noise[ids])) @ W   (the noise is a constant)
    4  the full ``ops.vbpr`` call with h, h_adv and lmd: the loss, the three table gradients, dH and dH_adv (through
       autograd to W) and grad_hsum of both; noise[item_ids] += hsum @ W^T with W as it was before its step
    5  Adagrad over the touched rows of P, Q, PQ2; Adam on W

against the reference's three forward and two backward passes per step.  The reference cannot train cold users
(``predict_adv`` indexes the users' noise with item ids, model/AMR.py:148), so ``--cold_object user`` is refused.

The published tensors, the ranking and the ``--save_emb`` file names are VBPR's (with AMR in the name).

One training step on the MI355X (tools/vbpr_step_ab.py: B = 2048, d = 64, content width 16; median of 60 steps), this
trainer's step against the same step in float32 torch (the running-sum form under autograd, torch.optim.Adagrad / Adam)
on the GPU: 1.71 ms against 2.39 ms on the toy tables (300 x 500; ratio 1.39), 1.57 ms against 2.08 ms on
MovieLens-sized ones (6040 x 3706; ratio 1.32).  Neither time moves at B = 16384: both steps are bound by the host's
launches.
"""
import torch
import torch.nn.functional as F

from .. import ops
from .FusedLossTrainer import VBPR_FILES, FusedLossTrainer, load_vbpr_tables
from .VBPR import VBPR_Learner, _check_flags, _check_width


class AMR_Learner(VBPR_Learner):
    def __init__(self, args, data, emb_size, device):
        _check_width('AMR', int(emb_size))
        p, q, user_aux, _item_aux, w = load_vbpr_tables('AMR', args, data, int(emb_size), data.item_content_dim)
        super().__init__(args, data, emb_size, device, tensors=(p, q, user_aux, w), who='AMR')
        self.eps, self.lmd = float(args.eps), float(args.lmd)
        self.register_buffer('noise', torch.zeros_like(self.content), persistent=False)      # never cleared during a run
        self.noise_log = None         # a list: the noise's Frobenius norm (device scalars) after each of a step's two additions

    def _add_noise(self, plan, hsum):
        self.noise[plan['item_ids'].long()] += hsum @ self.W.detach().T
        if self.noise_log is not None:
            self.noise_log.append(torch.linalg.norm(self.noise))

    def loss(self, users, pos, neg, id_range=None):
        """bpr_training + the tables' part of regs (model/AMR.py:155-202): steps 1 to 4 above."""
        plan, ids = self.plan(users, pos, neg, id_range)
        rows = self.content[ids]
        h = rows @ self.W
        with torch.no_grad():
            hsum = self.fused_hsum_only(plan, h)
            self._add_noise(plan, hsum)
            shifted = rows + self.eps * F.normalize(self.noise[ids])
        total, hsum = self.fused(plan, h, shifted @ self.W, self.lmd, want_hsum=True)
        with torch.no_grad():
            self._add_noise(plan, hsum)
        return total

    def fused_hsum_only(self, plan, h):
        return ops.vbpr(*self.tables(), h.detach().contiguous(), plan, float(self.args.p_emb[1]), want_user=False,
                        want_item=False, want_aux=False, want_h=False, want_hsum=True, want_loss=False,
                        workspace=self.workspace)[6]


class AMR(FusedLossTrainer):
    fused_eval = True        # the base class's batch_predict is the stock user_emb[users] @ item_emb.T
    LOSS_TERMS = ('bpr', 'adv', 'regs', 'batch_loss')
    TABLES = tuple(VBPR_FILES) + ('user_emb', 'item_emb')
    SAVE_FILES = VBPR_FILES

    def __init__(self, config):
        super().__init__(config)
        a = self.args
        if a.cold_object == 'user':
            raise ValueError('AMR: --cold_object user is not built: the reference cannot train cold users (predict_adv '
                             'indexes the users\' noise with item ids, noise[iid] at model/AMR.py:148, which raises or '
                             'perturbs with the wrong rows), so there is nothing to pin it against; use --cold_object item')
        _check_flags('AMR', a)
        self.model = AMR_Learner(a, self.data, self.emb_size, self.device)      # built on the CPU

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
            return torch.stack([t[0], t[1], t[2] + rw, batch_loss.detach()])

    def _current_tables(self):
        return self.model()
