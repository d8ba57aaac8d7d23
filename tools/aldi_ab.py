"""A/B on one device.  Default: one fused ALDI loss call (forward + backward, csrc/aldi.hip through ops.aldi) against the
torch formula of the reference (model/ALDI.py:50-82, the B x B product included, as tests/aldi_restate.py states it) under
autograd, on the same tower outputs.
With --eval: one `all` evaluation of a synthetic catalogue on the two-table route (one fused scoring call per user table,
lists merged) against the batch_predict route (two products scattered into a zeroed (bs x items) block, ranked densely).

    python tools/aldi_ab.py [--batch 4096] [--d 64] [--users 6040] [--items 3706] [--rounds 30]
    python tools/aldi_ab.py --eval [--eval_users 4096] [--eval_items 300000] [--cold_share 0.1] [--bs 512] [--rounds 10]

The arms are interleaved round by round after a warm-up of every shape; the loss arms are timed with device events, the
evaluation arms with the host clock around a device synchronise (both routes have host work).  Prints one JSON line with
the medians, the extremes of every arm (the run-to-run spread) and the largest difference of the outputs.
"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from coldrec_amd import ops  # noqa: E402
from tests.aldi_restate import loss_terms  # noqa: E402  (the torch formula, the B x B product included)


def summary(times):
    return dict(ms_median={k: sorted(v)[len(v) // 2] for k, v in times.items()},
                ms_min={k: min(v) for k, v in times.items()}, ms_max={k: max(v) for k, v in times.items()})


def loss_ab(a, dev):
    g = torch.Generator().manual_seed(0)
    B, d = a.batch, a.d
    U, V = (torch.randn(a.users, d, generator=g) * 0.1).to(dev), (torch.randn(a.items, d, generator=g) * 0.1).to(dev)
    users, pos, neg = (torch.randint(n, (B,), generator=g).to(dev) for n in (a.users, a.items, a.items))
    gu, gp, gn = ((torch.randn(B, d, generator=g) * 0.1).to(dev).requires_grad_() for _ in range(3))
    w = (0.2 + 0.8 * torch.rand(a.items, generator=g)).to(dev)
    coef = (0.9, 0.05, 0.1)
    i32 = [t.to(torch.int32) for t in (users, pos, neg)]
    rng = ((0, a.users - 1), (0, a.items - 1))
    ws, bufs, loss = ops.aldi_workspace(B, d, dev), [torch.empty_like(gu) for _ in range(3)], torch.empty(5, device=dev)

    def fused():
        ops.aldi(U, V, *i32, gu.detach(), gp.detach(), gn.detach(), w, *coef, grad_user=bufs[0], grad_pos=bufs[1],
                 grad_neg=bufs[2], loss=loss, workspace=ws, id_range=rng)

    def formula():
        return torch.autograd.grad(loss_terms(U, V, users, pos, neg, gu, gp, gn, w, *coef)[4], (gu, gp, gn))

    arms = dict(fused=fused, torch_formula=formula)
    for f in arms.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k, f in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.calls):
                f()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1) / a.calls)
    ref = formula()
    fused()
    err = [float((b - r).abs().max() / r.abs().max()) for b, r in zip(bufs, ref)]
    out = summary(times)
    out.update(what="loss", shape=dict(batch=B, d=d, users=a.users, items=a.items), calls_per_sample=a.calls,
               ratio_formula_over_fused=out["ms_median"]["torch_formula"] / out["ms_median"]["fused"],
               arms_separated=out["ms_max"]["fused"] < out["ms_min"]["torch_formula"], grad_err_over_max=err)
    return out


class _Catalogue:
    """What the trainer base class reads of a data builder, for ids that are their own keys."""

    class _Identity:
        def __init__(self, n):
            self.n = n

        def __getitem__(self, k):
            return k

        def __len__(self):
            return self.n

    def __init__(self, n_users, n_items, cold_share, rated, seed=0):
        rng = np.random.default_rng(seed)
        self.user_num, self.item_num = n_users, n_items
        self.item, self.item_keys = self._Identity(n_items), np.arange(n_items)
        cold = np.sort(rng.choice(n_items, int(n_items * cold_share), replace=False))
        self.mapped_cold_item_idx = cold
        self.mapped_warm_item_idx = np.setdiff1d(np.arange(n_items), cold)
        self.rated_rowptr = np.arange(n_users + 1, dtype=np.int64) * rated
        self.rated_col = np.sort(rng.integers(0, n_items, (n_users, rated)), axis=1).reshape(-1).astype(np.int32)
        self.overall_test_set = {u: {int(i): 1.0 for i in rng.integers(0, n_items, 5)} for u in range(n_users)}

    def get_user_id_list(self, users):
        return np.asarray(users, np.int64)


def eval_ab(a, dev):
    from coldrec_amd.model.BaseRecommender import BaseColdStartTrainer
    data = _Catalogue(a.eval_users, a.eval_items, a.cold_share, 20)
    args = argparse.Namespace(topN="10,20", model="ALDI", dataset="synthetic", emb_size=a.d, epochs=0, bs=a.bs, lr=1e-3,
                              reg=1e-4, early_stop=0, eval_every=1, cold_object="item", score_dtype="fp32")
    g = torch.Generator().manual_seed(1)
    tables = [(torch.randn(n, a.d, generator=g) * 0.1).to(dev) for n in (a.eval_users, a.eval_users, a.eval_items)]
    warm = torch.from_numpy(data.mapped_warm_item_idx).to(dev)
    cold = torch.from_numpy(data.mapped_cold_item_idx).to(dev)

    class Dense(BaseColdStartTrainer):
        fused_eval = False

        def train(self): ...
        def predict(self, u): ...
        def save(self): ...

        def batch_predict(self, users):
            users = torch.as_tensor(self.data.get_user_id_list(users), device=self.device)
            score = torch.zeros(users.shape[0], self.data.item_num, dtype=torch.float32, device=self.device)
            score[:, warm] = self.warm_user_emb[users] @ self.item_emb[warm].T
            score[:, cold] = self.cold_user_emb[users] @ self.item_emb[cold].T
            return score

    class TwoTable(Dense):
        def _eval_parts(self):
            return [(self.warm_user_emb, self.data.mapped_cold_item_idx), (self.cold_user_emb, self.data.mapped_warm_item_idx)]

    arms, out_ids = {}, {}
    for name, cls in (("two_table", TwoTable), ("batch_predict", Dense)):
        tr = cls(types.SimpleNamespace(args=args, data=data, device=dev))
        tr.warm_user_emb, tr.cold_user_emb, tr.item_emb = tables
        arms[name] = tr

    def run(name):
        _, s, i = arms[name]._topk_device(data.overall_test_set, "all")
        out_ids[name] = (s, i)

    for k in arms:
        for _ in range(2):
            run(k)
    torch.cuda.synchronize()
    times = {k: [] for k in arms}
    for _ in range(a.rounds):
        for k in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(k)
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    same = float((out_ids["two_table"][1] == out_ids["batch_predict"][1]).float().mean())
    diff = float((out_ids["two_table"][0] - out_ids["batch_predict"][0]).abs().max())
    out = summary(times)
    out.update(what="eval", shape=dict(users=a.eval_users, items=a.eval_items, cold=len(data.mapped_cold_item_idx), d=a.d,
                                       bs=a.bs, k=20),
               ratio_batch_predict_over_two_table=out["ms_median"]["batch_predict"] / out["ms_median"]["two_table"],
               arms_separated=out["ms_max"]["two_table"] < out["ms_min"]["batch_predict"], same_id_share=same,
               max_score_diff=diff)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--d", type=int, default=64)
    ap.add_argument("--users", type=int, default=6040)
    ap.add_argument("--items", type=int, default=3706)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--calls", type=int, default=20, help="calls per timed sample of the loss arms")
    ap.add_argument("--eval", action="store_true")
    ap.add_argument("--eval_users", type=int, default=4096)
    ap.add_argument("--eval_items", type=int, default=300000)
    ap.add_argument("--cold_share", type=float, default=0.1)
    ap.add_argument("--bs", type=int, default=512)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aldi_ab: needs the GPU; there is no CPU path")
    dev = torch.device("cuda:0")
    print(json.dumps(eval_ab(a, dev) if a.eval else loss_ab(a, dev)))


if __name__ == "__main__":
    main()
