"""GPU parity tests added in round 2 (run with -m gpu on an MI355X), all through the C ABI:
lists of up to 128 entries, the SGD mode, l2_reg_loss / bpr_loss autograd Functions, embedding widths that are not
multiples of 4, the RCCL entry points (one rank), and two-rank runs of the REAL HIP ops on one GPU over gloo
(item-sharded and user-sharded evaluation, data-parallel MF / LightGCN steps)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import oracle_np as orc
from oracle import ref_port

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        x = x.to(dtype)
    return x.to(DEV)


# ------------------------------------------------------------------------------------------------ k up to 128
@pytest.mark.parametrize("n_users,n_items,d,k,splits", [
    (70, 900, 128, 65, 0), (70, 900, 128, 100, 3), (129, 5000, 64, 128, 0), (33, 20000, 128, 128, 8),
    (300, 70001, 32, 100, 0), (64, 150, 16, 128, 0), (40, 3000, 256, 77, 2)])
def test_topk_lists_up_to_128_bit_exact(n_users, n_items, d, k, splits):
    """The reference takes any --topN (model/BaseRecommender.py:27-29): k = 65..128 through the fused kernel (forced
    splits -> merge), the dense route (splits = 0 on small catalogues) and the row-major fallback, masks included."""
    from coldrec_amd import ops
    rng = np.random.default_rng(n_users * 31 + k)
    U = (rng.standard_normal((n_users, d)) * 0.2).astype(np.float32)
    V = (rng.standard_normal((n_items, d)) * 0.2).astype(np.float32)
    rated = [np.unique(rng.integers(0, n_items, rng.integers(0, 40))) for _ in range(n_users)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rated])]).astype(np.int64)
    col = np.concatenate(rated).astype(np.int32) if rowptr[-1] else np.zeros(0, np.int32)
    cold = np.where(rng.random(n_items) < 0.3)[0]
    rp, rc = ops.rated_csr(rated, DEV)
    bm = ops.make_bitmap(n_items, cold, DEV)
    want = orc.score_topk(U, None, V, k, rowptr, col, orc.make_bitmap(n_items, cold))
    for pack in (True, False):
        s, i = ops.score_topk(t(U), None, t(V), k, rp, rc, bm, n_splits=splits, pack=pack)
        torch.cuda.synchronize()
        assert np.array_equal(i.cpu().numpy(), want[1]), (pack, "indices")
        assert np.array_equal(s.cpu().numpy().view(np.uint32), want[0].view(np.uint32)), (pack, "scores")


def test_mask_topk_and_merge_with_k_100():
    from coldrec_amd import ops
    rng = np.random.default_rng(3)
    S = rng.standard_normal((50, 4000)).astype(np.float32)
    S[:, ::7] = S[:, 1::7]                                        # ties
    cold = np.where(rng.random(4000) < 0.2)[0]
    want = orc.mask_topk(S, 100, None, None, orc.make_bitmap(4000, cold))
    got = ops.mask_topk(t(S), 100, None, None, ops.make_bitmap(4000, cold, DEV), write_back=False)
    assert np.array_equal(got[1].cpu().numpy(), want[1])
    assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want[0].view(np.uint32))
    # 40 partial lists of 128 entries (the largest the merge stages in LDS: two waves per block)
    ls = -np.sort(-rng.standard_normal((40, 90, 128)).astype(np.float32), axis=2)
    li = rng.permutation(40 * 90 * 128).astype(np.int32).reshape(40, 90, 128)
    ws, wi = orc.merge_topk(ls, li, 128)
    gs, gi = ops.merge_topk(t(ls), t(li), 128)
    assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gs.cpu().numpy().view(np.uint32), ws.view(np.uint32))


def test_topn_above_the_list_limit_is_a_loud_error():
    import argparse
    import types
    from coldrec_amd.model.MF import MF
    args = argparse.Namespace(topN="10,200", model="MF", dataset="x", emb_size=8, epochs=1, bs=8, lr=1e-3, reg=1e-4,
                              early_stop=0, cold_object="item")
    with pytest.raises(ValueError, match="1..128"):
        MF(types.SimpleNamespace(args=args, data=types.SimpleNamespace(user_num=4, item_num=4), device=DEV))


# ------------------------------------------------------------------------------------------------ SGD mode
def _triples(rng, n_u, n_i, B):
    return (rng.integers(0, n_u, B).astype(np.int32), rng.integers(0, n_i, B).astype(np.int32),
            rng.integers(0, n_i, B).astype(np.int32))


@pytest.mark.parametrize("d,with_plan", [(16, True), (16, False), (128, True), (50, True)])
def test_mf_sgd_steps_match_torch_optim_sgd_port(d, with_plan):
    """north_star's "BPR loss + SGD update": MFEngine(optimizer='sgd') == the reference-call port with torch.optim.SGD
    (losses 1e-5, tables 1e-5 of their norm); with a plan only the touched rows move (sgd_rows), without it the dense
    pass runs -- same tables.  d = 50 exercises the zero-padded width."""
    from coldrec_amd import ops
    from coldrec_amd.train import MFEngine
    rng = np.random.default_rng(d + with_plan)
    n_u, n_i, B = 120, 260, 300
    U0 = (rng.standard_normal((n_u, d)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n_i, d)) * 0.1).astype(np.float32)
    eng = MFEngine(U0, V0, 0.05, 1e-3, DEV, optimizer="sgd")
    assert eng.M is None and eng.V is None
    port = ref_port.MFPort(U0, V0, 0.05, 1e-3, optimizer="sgd")
    for _ in range(8):
        u, i, j = _triples(rng, n_u, n_i, B)
        tu, ti, tj = t(u), t(i), t(j)
        plan = ops.build_plans_device(tu, ti, tj, B)[0] if with_plan else None
        eng.step(tu, ti, tj, plan=plan)
        want = port.step(u, i, j)
        assert abs(eng.last_loss() - want) <= 1e-5 * abs(want)
    got = torch.cat([eng.user_emb, eng.item_emb], 0).cpu().numpy()
    ref = np.concatenate([port.U.detach().numpy(), port.V.detach().numpy()])
    assert np.linalg.norm(got - ref) <= 1e-5 * np.linalg.norm(ref)
    assert eng.G.abs().max().item() == 0.0                         # consumed gradient rows were cleared


def test_mf_sgd_one_launch_epoch_matches_three_kernel_epoch():
    """EpochRunner with the SGD variant of the one-launch step (crh_mf_step_sgd_f32, hipGraph epochs) vs the eager
    three-kernel SGD step and vs the port."""
    from coldrec_amd.train import EpochRunner, MFEngine
    rng = np.random.default_rng(11)
    n_u, n_i, d, B, n = 400, 700, 64, 512, 512 * 5 + 77
    U0 = (rng.standard_normal((n_u, d)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n_i, d)) * 0.1).astype(np.float32)
    a = MFEngine(U0, V0, 0.05, 1e-3, DEV, optimizer="sgd")
    b = MFEngine(U0, V0, 0.05, 1e-3, DEV, optimizer="sgd")
    port = ref_port.MFPort(U0, V0, 0.05, 1e-3, optimizer="sgd")
    ra, rb = EpochRunner(a, n, B, fused=True), EpochRunner(b, n, B, fused=False)
    assert a.fused and not getattr(b, "fused", False)
    for _ in range(3):                                             # eager, captured, replayed
        u, i, j = _triples(rng, n_u, n_i, n)
        la = ra.run(u, i, j).sum(1).cpu().numpy()
        lb = rb.run(u, i, j).sum(1).cpu().numpy()
        lp = np.array([port.step(u[lo:lo + B], i[lo:lo + B], j[lo:lo + B]) for lo in range(0, n, B)])
        np.testing.assert_allclose(la, lp, rtol=1e-5)
        np.testing.assert_allclose(lb, lp, rtol=1e-5)
    ref = np.concatenate([port.U.detach().numpy(), port.V.detach().numpy()])
    for eng in (a, b):
        assert np.linalg.norm(eng.E.cpu().numpy() - ref) <= 1e-5 * np.linalg.norm(ref)


@pytest.mark.parametrize("L", [1, 3])
def test_lightgcn_sgd_steps_match_port(L):
    from coldrec_amd import ops
    from coldrec_amd.train import LGCNEngine
    from coldrec_amd.util.databuilder import bipartite_norm_adj_csr
    rng = np.random.default_rng(5 + L)
    n_u, n_i, d, B = 90, 140, 32, 200
    pairs = np.unique(np.stack([rng.integers(0, n_u, 1500), rng.integers(0, n_i - 6, 1500)], 1), axis=0)
    rowptr, col, val = bipartite_norm_adj_csr(pairs[:, 0], pairs[:, 1], n_u, n_i)
    U0 = (rng.standard_normal((n_u, d)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n_i, d)) * 0.1).astype(np.float32)
    eng = LGCNEngine(U0, V0, rowptr, col, val, L, 0.05, 1e-3, DEV, optimizer="sgd")
    port = ref_port.LGCNPort(U0, V0, ref_port.coo_adj(rowptr, col, val), L, 0.05, 1e-3, optimizer="sgd")
    for _ in range(6):
        u, i, j = _triples(rng, n_u, n_i, B)
        tu, ti, tj = t(u), t(i), t(j)
        eng.step(tu, ti, tj, plan=ops.build_plans_device(tu, ti, tj, B)[0])
        want = port.step(u, i, j)
        assert abs(eng.last_loss() - want) <= 1e-5 * abs(want)
    ref = np.concatenate([port.U.detach().numpy(), port.V.detach().numpy()])
    assert np.linalg.norm(eng.E.cpu().numpy() - ref) <= 1e-5 * np.linalg.norm(ref)


def test_sgd_dense_is_one_fma_per_element():
    from coldrec_amd import ops
    rng = np.random.default_rng(2)
    p = rng.standard_normal(4096 * 33).astype(np.float32)
    g = rng.standard_normal(p.shape).astype(np.float32)
    tp, tg = t(p), t(g)
    ops.sgd_dense(tp, tg, 0.0123, zero_grad=True)
    assert np.array_equal(tp.cpu().numpy().view(np.uint32), orc.sgd_dense(p, g, 0.0123).view(np.uint32))
    assert tg.abs().max().item() == 0.0


# ------------------------------------------------------------------------------------------------ autograd Functions
@pytest.mark.parametrize("d", [64, 50, 7])
def test_bpr_and_l2_functions_match_reference_autograd(d):
    """util.utils.bpr_loss / l2_reg_loss as plugins call them (any width, 2..6 tensors of different shapes): values
    and gradients vs the reference formulas through CPU autograd (oracle/ref_port.py)."""
    from coldrec_amd.util.utils import bpr_loss, l2_reg_loss
    rng = np.random.default_rng(d)
    B = 257
    arrs = [(rng.standard_normal((B, d)) * 0.3).astype(np.float32) for _ in range(3)]
    extra = [(rng.standard_normal(s) * 0.3).astype(np.float32) for s in ((31, d), (5, 2 * d + 1))]
    cpu = [torch.tensor(a, requires_grad=True) for a in arrs + extra]
    gpu = [torch.tensor(a, device=DEV, requires_grad=True) for a in arrs + extra]
    lc = ref_port.bpr_loss(*cpu[:3]) * 1.7 + ref_port.l2_reg_loss(0.02, *cpu)
    lg = bpr_loss(*gpu[:3]) * 1.7 + l2_reg_loss(0.02, *gpu)
    lc.backward()
    lg.backward()
    assert abs(float(lg.detach()) - float(lc.detach())) <= 1e-5 * abs(float(lc.detach()))
    for c, g in zip(cpu, gpu):
        sc = float(c.grad.abs().max())
        np.testing.assert_allclose(g.grad.cpu().numpy(), c.grad.numpy(), rtol=1e-4, atol=2e-6 * sc)


def test_engine_with_width_not_multiple_of_four_matches_port():
    """--emb_size 50: the engine pads to 52 zero columns internally; Adam leaves them at exactly 0 and the visible
    tables match the port."""
    from coldrec_amd import ops
    from coldrec_amd.train import MFEngine
    rng = np.random.default_rng(8)
    n_u, n_i, d, B = 80, 90, 50, 128
    U0 = (rng.standard_normal((n_u, d)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n_i, d)) * 0.1).astype(np.float32)
    eng = MFEngine(U0, V0, 1e-2, 1e-3, DEV)
    port = ref_port.MFPort(U0, V0, 1e-2, 1e-3)
    for _ in range(5):
        u, i, j = _triples(rng, n_u, n_i, B)
        tu, ti, tj = t(u), t(i), t(j)
        eng.step(tu, ti, tj, plan=ops.build_plans_device(tu, ti, tj, B)[0])
        want = port.step(u, i, j)
        assert abs(eng.last_loss() - want) <= 1e-5 * abs(want)
    assert eng.user_emb.shape == (n_u, 50) and eng.E.shape[1] == 52
    assert eng.E[:, 50:].abs().max().item() == 0.0
    ref = np.concatenate([port.U.detach().numpy(), port.V.detach().numpy()])
    got = torch.cat([eng.user_emb, eng.item_emb]).cpu().numpy()
    assert np.linalg.norm(got - ref) <= 2e-5 * np.linalg.norm(ref)
    s, i = ops.score_topk(eng.user_emb, None, eng.item_emb, 10)      # non-contiguous views are accepted by the ranker
    ws, wi = orc.score_topk(eng.user_emb.cpu().numpy(), None, eng.item_emb.cpu().numpy(), 10)
    assert np.array_equal(i.cpu().numpy(), wi)


# ------------------------------------------------------------------------------------------------ RCCL entry points
def test_crh_comm_single_rank_roundtrip():
    """crh_comm_* on a one-rank communicator (the box has one GPU; RCCL refuses two ranks on one device): the
    all-reduce leaves the buffer unchanged, the all-gather output equals the input and feeds crh_merge_topk."""
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    torch.cuda.set_device(0)
    uid = (ctypes.c_char * 128)()
    _lib.check(L.crh_comm_unique_id(ctypes.addressof(uid)), "crh_comm_unique_id")
    comm = L.crh_comm_init(0, 1, ctypes.addressof(uid))
    assert comm, L.crh_last_error()
    try:
        assert L.crh_comm_rank(comm) == 0 and L.crh_comm_world(comm) == 1
        x = torch.arange(1000, dtype=torch.float32, device=DEV) * 0.5
        want = x.clone()
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(L.crh_comm_allreduce_f32(comm, x.data_ptr(), x.numel(), st), "crh_comm_allreduce_f32")
        rng = np.random.default_rng(1)
        s = t(-np.sort(-rng.standard_normal((77, 20)).astype(np.float32), axis=1))
        i = t(rng.permutation(77 * 20).astype(np.int32).reshape(77, 20))
        gs, gi = torch.empty((1, 77, 20), device=DEV), torch.empty((1, 77, 20), dtype=torch.int32, device=DEV)
        ws_bytes = L.crh_comm_allgather_topk_workspace_bytes(1, 77, 20)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        _lib.check(L.crh_comm_allgather_topk(comm, s.data_ptr(), i.data_ptr(), 77, 20, gs.data_ptr(), gi.data_ptr(),
                                             ws.data_ptr(), ws_bytes, st), "crh_comm_allgather_topk")
        ms, mi = ops.merge_topk(gs, gi, 20)
        torch.cuda.synchronize()
        assert torch.equal(x, want) and torch.equal(gs[0], s) and torch.equal(gi[0], i)
        assert torch.equal(mi, i) and torch.equal(ms, s)
        # the touched-rows step's exchange through the C ABI alone (round 6): backward over the owned rows -> pack -> crh_comm_allgather_rows
        # -> unpack into a zeroed gradient table == the plain deterministic backward, bit for bit (world = 1: every row is owned here)
        n_u, n_i, d, B = 300, 500, 64, 700
        U0 = t((rng.standard_normal((n_u, d)) * 0.1).astype(np.float32))
        V0 = t((rng.standard_normal((n_i, d)) * 0.1).astype(np.float32))
        tri = [t(rng.integers(0, n, B).astype(np.int32)) for n in (n_u, n_i, n_i)]
        plan = ops.build_plans_device(*tri, B)[0]
        E = torch.cat([U0, V0]).contiguous()
        G_want, G_own, G_got = torch.zeros_like(E), torch.zeros_like(E), torch.zeros_like(E)
        loss = torch.zeros(2, device=DEV)
        ops.bpr_fwd_bwd(E[:n_u], E[n_u:], E[n_u:], *tri, 1e-3, G_want[:n_u], G_want[n_u:], G_want[n_u:], loss, plan=plan)
        wsb, sums, loss2 = ops.bpr_workspace(B, DEV), torch.zeros(4, device=DEV), torch.zeros(2, device=DEV)
        ops.bpr_fwd(E[:n_u], E[n_u:], E[n_u:], *tri, sums, wsb)
        ops.bpr_bwd_owned(E[:n_u], E[n_u:], *tri, 1e-3, sums, G_own[:n_u], G_own[n_u:], loss2, wsb, plan, 1, 0)
        cap = ops.rows_pack_cap(B, 1)
        ids, rows = torch.empty(cap, dtype=torch.int32, device=DEV), torch.zeros((cap, d), device=DEV)
        ops.rows_pack(G_own, plan, B, n_u, 1, 0, ids, rows)
        gids, grows = torch.empty_like(ids), torch.empty_like(rows)
        _lib.check(L.crh_comm_allgather_rows(comm, ids.data_ptr(), rows.data_ptr(), cap, d, gids.data_ptr(), grows.data_ptr(), st),
                   "crh_comm_allgather_rows")
        ops.rows_unpack(G_got, gids, grows)
        torch.cuda.synchronize()
        assert torch.equal(loss, loss2) and torch.equal(G_own.view(torch.int32), G_want.view(torch.int32))
        assert torch.equal(G_got.view(torch.int32), G_want.view(torch.int32)) and int((gids >= 0).sum()) == int(plan[0] + plan[1])
    finally:
        _lib.check(L.crh_comm_destroy(comm), "crh_comm_destroy")


# ------------------------------------------------------------------------------------------------ two ranks, real kernels
_TWO_RANK_WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["CR_ROOT"])
import numpy as np, torch, torch.distributed as dist
gpu = int(os.environ["LOCAL_RANK"]) if os.environ.get("CR_GPU_PER_RANK") == "1" else 0
torch.cuda.set_device(gpu)
dev = torch.device("cuda", gpu)
dist.init_process_group("gloo")                       # ranks share GPU 0 unless CR_GPU_PER_RANK=1; gloo stages through the host
rank, world = dist.get_rank(), dist.get_world_size()
from coldrec_amd import ops
from coldrec_amd.eval import ShardedTopK, UserShardedTopK, shard_bounds
from coldrec_amd.train import DPContext, LGCNEngine, MFEngine
from coldrec_amd.util.databuilder import bipartite_norm_adj_csr

# ---- evaluation: item-row shards + all-gather + canonical merge, and the user-sharded alternative
g = torch.Generator(device=dev).manual_seed(7)
n_users, n_items, d, k = int(os.environ.get("CR_NUSERS", "20000")), int(os.environ.get("CR_NITEMS", "200000")), 128, 20
U = (torch.rand((n_users, d), generator=g, device=dev) - 0.5) * 0.3
V = (torch.rand((n_items, d), generator=g, device=dev) - 0.5) * 0.3
rng = np.random.default_rng(5)
rated = [np.unique(rng.integers(0, n_items, 12)) for _ in range(n_users)]
rp, rc = ops.rated_csr(rated, dev)
bm = ops.make_bitmap(n_items, np.where(rng.random(n_items) < 0.2)[0], dev)
users = torch.arange(n_users, dtype=torch.int32, device=dev)
want = ops.score_topk(U, users, V, k, rp, rc, bm)                    # the one-rank result
lo, hi = shard_bounds(n_items, world, rank)
got = ShardedTopK(V[lo:hi].contiguous(), lo, n_items, k, world, rank).topk(U, users, rp, rc, bm)
torch.cuda.synchronize()
assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), "item shards"
got = UserShardedTopK(V, k, world, rank).topk(U, users, rp, rc, bm)
torch.cuda.synchronize()
assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), "user shards"

# ---- data-parallel training steps vs the one-rank engine (same triples on every rank: replicated sampler)
rng = np.random.default_rng(9)
n_u, n_i, dd, B = 300, 500, 64, int(os.environ.get("CR_B", "1001"))     # 1001: odd batch, uneven slices
U0 = (rng.standard_normal((n_u, dd)) * 0.1).astype(np.float32)
V0 = (rng.standard_normal((n_i, dd)) * 0.1).astype(np.float32)
pairs = np.unique(np.stack([rng.integers(0, n_u, 4000), rng.integers(0, n_i - 9, 4000)], 1), axis=0)
rowptr, col, val = bipartite_norm_adj_csr(pairs[:, 0], pairs[:, 1], n_u, n_i)
for name in ("mf", "lgcn", "mf-sgd"):
    opt = "sgd" if name.endswith("sgd") else "adam"
    mk = (lambda: LGCNEngine(U0, V0, rowptr, col, val, 2, 1e-2, 1e-3, dev, optimizer=opt)) if name == "lgcn" else \
         (lambda: MFEngine(U0, V0, 1e-2, 1e-3, dev, optimizer=opt))
    one, dp = mk(), mk()
    dp.enable_data_parallel(DPContext(world, rank))
    r2 = np.random.default_rng(77)
    for s in range(4):
        tri = [torch.from_numpy(r2.integers(0, n, B).astype(np.int32)).to(dev) for n in (n_u, n_i, n_i)]
        one.step(*tri, plan=ops.build_plans_device(*tri, B)[0])
        dp.step(*tri)
        a, b = one.last_loss(), dp.last_loss()
        assert abs(a - b) <= 1e-5 * abs(a), (name, s, a, b)
    err = float((one.E - dp.E).norm() / one.E.norm())
    assert err <= 1e-5, (name, err)
    gathered = [torch.empty_like(dp.E) for _ in range(world)]
    dist.all_gather(gathered, dp.E)
    assert all(torch.equal(gathered[0], x) for x in gathered), (name, "replicas differ")
    # the slice backward is reproducible: the same step from the same state gives the same bits
    again = mk(); again.enable_data_parallel(DPContext(world, rank))
    r2 = np.random.default_rng(77)
    for s in range(4):
        tri = [torch.from_numpy(r2.integers(0, n, B).astype(np.int32)).to(dev) for n in (n_u, n_i, n_i)]
        again.step(*tri)
    assert torch.equal(again.E, dp.E), (name, "data-parallel step not reproducible")
# ---- row-sharded LightGCN propagation (8(e) scalable variant): each rank multiplies ITS rows, layer states all-gathered;
# per row the arithmetic is the replicated engine's, so the tables must be bit-identical to the replicated DP run
for opt, L in (("adam", 3), ("sgd", 2), ("adam", 1)):
    rep = LGCNEngine(U0, V0, rowptr, col, val, L, 1e-2, 1e-3, dev, optimizer=opt)
    rep.enable_data_parallel(DPContext(world, rank))
    shd = LGCNEngine(U0, V0, rowptr, col, val, L, 1e-2, 1e-3, dev, optimizer=opt)
    shd.enable_row_sharding(DPContext(world, rank))
    one = LGCNEngine(U0, V0, rowptr, col, val, L, 1e-2, 1e-3, dev, optimizer=opt)
    r2 = np.random.default_rng(78)
    for s in range(4):
        tri = [torch.from_numpy(r2.integers(0, n, B).astype(np.int32)).to(dev) for n in (n_u, n_i, n_i)]
        rep.step(*tri); shd.step(*tri); one.step(*tri, plan=ops.build_plans_device(*tri, B)[0])
        a, b = one.last_loss(), shd.last_loss()
        assert abs(a - b) <= 1e-5 * abs(a), ("row-sharded", opt, L, s, a, b)
    assert torch.equal(rep.E, shd.E), ("row-sharded != replicated data-parallel", opt, L)
    fu, fi = shd.forward()
    ou, oi = one.forward()
    assert float((fu - ou).norm() / ou.norm()) <= 1e-5 and float((fi - oi).norm() / oi.norm()) <= 1e-5
    gathered = [torch.empty_like(shd.E) for _ in range(world)]
    dist.all_gather(gathered, shd.E.contiguous())
    assert all(torch.equal(gathered[0], x) for x in gathered), ("row-sharded replicas differ", opt, L)
# ---- the data-parallel TOUCHED-ROWS step (VERDICT r5 #4; train.MFEngine._lazy_step_dp: row-ownership split of the backward,
# one all-gather of (row id, row) slots): every replica AND the one-rank touched-rows engine agree bit for bit -- losses
# after every step, parameters and both Adam moments after the flush
one, dpl = MFEngine(U0, V0, 1e-2, 1e-3, dev), MFEngine(U0, V0, 1e-2, 1e-3, dev)
one.enable_lazy_adam()
dpl.enable_data_parallel(DPContext(world, rank)); dpl.enable_lazy_adam()
r2 = np.random.default_rng(79)
hot = r2.integers(0, n_i, 12)                              # a few items recur in most batches: heavy rows of the plan
for s in range(6):
    uu = r2.integers(0, n_u, B).astype(np.int32)
    ii = np.where(r2.random(B) < 0.3, hot[r2.integers(0, 12, B)], r2.integers(0, n_i, B)).astype(np.int32)
    jj = r2.integers(0, n_i, B).astype(np.int32)
    tri = [torch.from_numpy(x).to(dev) for x in (uu, ii, jj)]
    one.step(*tri); dpl.step(*tri)
    assert torch.equal(one.loss.view(torch.int32), dpl.loss.view(torch.int32)), ("touched-rows dp loss", s)
cap = -(-3 * B // world)
assert dpl.exchange_bytes_per_step == world * cap * (dd + 4) * 4, dpl.exchange_bytes_per_step
one.sync_tables(); dpl.sync_tables()
for a, b, what in ((one.E, dpl.E, "parameters"), (one.M, dpl.M, "first moments"), (one.V, dpl.V, "second moments")):
    assert torch.equal(a.view(torch.int32), b.view(torch.int32)), ("touched-rows dp != one rank", what)
assert float(dpl.G.abs().max()) == 0.0
gathered = [torch.empty_like(dpl.E) for _ in range(world)]
dist.all_gather(gathered, dpl.E)
assert all(torch.equal(gathered[0], x) for x in gathered), "touched-rows dp replicas differ"
# a rank with an EMPTY slice still reports the global loss
tiny = MFEngine(U0, V0, 1e-2, 1e-3, dev); tiny.enable_data_parallel(DPContext(world, rank))
tri = [torch.from_numpy(np.array([3], np.int32)).to(dev) for _ in range(3)]
full = MFEngine(U0, V0, 1e-2, 1e-3, dev); full.step(*tri)
tiny.step(*tri)
assert abs(tiny.last_loss() - full.last_loss()) <= 1e-5 * abs(full.last_loss()), (rank, tiny.last_loss(), full.last_loss())
dist.barrier()
if rank == 0:
    print("TWO_RANK_HIP_OK", world)
dist.destroy_process_group()
'''


def test_two_ranks_real_hip_kernels_on_one_gpu_over_gloo(tmp_path):
    """SURVEY.md 8(e) with the HIP kernels in the loop (the CPU gloo tests stand them in): 20 000 users x 200 000
    items ranked by two item shards + all-gather + merge == one rank, bit for bit; user shards likewise; four
    data-parallel MF / LightGCN / MF-SGD steps vs the one-rank engine (1e-5), replicas bitwise equal, repeatable; the
    row-sharded LightGCN propagation (all-gathered layer states) bit-identical to the replicated data-parallel run."""
    script = tmp_path / "two_rank_worker.py"
    script.write_text(_TWO_RANK_WORKER)
    env = dict(os.environ, CR_ROOT=ROOT, OMP_NUM_THREADS="4")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                          "--master-addr", "127.0.0.1", "--master-port", "29641", str(script)],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "TWO_RANK_HIP_OK 2" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


def test_eight_ranks_real_hip_kernels_on_one_gpu_over_gloo(tmp_path):
    """The node size the north_star names, with the HIP kernels in the loop: EIGHT ranks, one GPU each (gloo for the
    exchange).  4 096 users x 200 003 items: eight item shards whose sizes differ (200 003 = 8 x 25 000 + 3) + all-gather
    + the 160-candidate canonical merge == one rank, bit for bit; eight user slices likewise; the data-parallel slices of
    a 4 096-triple batch (MF, LightGCN, MF-SGD) and the row-sharded propagation (800 rows into 8 blocks) as in the
    two-rank test.  Eight processes must not share one device, so the test needs eight GPUs."""
    n_gpus = torch.cuda.device_count()
    if n_gpus < 8:
        pytest.skip(f"needs 8 GPUs (one per rank), found {n_gpus}")
    script = tmp_path / "eight_rank_worker.py"
    script.write_text(_TWO_RANK_WORKER)
    env = dict(os.environ, CR_ROOT=ROOT, OMP_NUM_THREADS="2", CR_NUSERS="4096", CR_NITEMS="200003", CR_B="4096",
               CR_GPU_PER_RANK="1")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=8",
                          "--master-addr", "127.0.0.1", "--master-port", "29648", str(script)],
                         env=env, capture_output=True, text=True, timeout=1500)
    assert out.returncode == 0 and "TWO_RANK_HIP_OK 8" in out.stdout, (out.stdout[-2000:], out.stderr[-4000:])


_COMM_WORKER = r'''
import ctypes, os, sys, time
sys.path.insert(0, os.environ["CR_ROOT"])
import numpy as np, torch
rank, world, uid_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
ndev = torch.cuda.device_count()
torch.cuda.set_device(rank % ndev)
dev = torch.device("cuda", rank % ndev)
from coldrec_amd import _lib, ops
L = _lib.lib()
uid = (ctypes.c_char * 128)()
if rank == 0:
    _lib.check(L.crh_comm_unique_id(ctypes.addressof(uid)), "crh_comm_unique_id")
    open(uid_path + ".tmp", "wb").write(bytes(uid)); os.replace(uid_path + ".tmp", uid_path)
else:
    t0 = time.time()
    while not os.path.exists(uid_path):
        assert time.time() - t0 < 60
        time.sleep(0.05)
    ctypes.memmove(uid, open(uid_path, "rb").read(), 128)
comm = L.crh_comm_init(rank, world, ctypes.addressof(uid))
if not comm:
    print("COMM_INIT_REFUSED", L.crh_last_error().decode()); sys.exit(0)
st = torch.cuda.current_stream().cuda_stream
n_users, n_items, d, k = 1000, 40001, 64, 20
g = torch.Generator(device=dev).manual_seed(11)
U = (torch.rand((n_users, d), generator=g, device=dev) - 0.5)
V = (torch.rand((n_items, d), generator=g, device=dev) - 0.5)
lo, hi = rank * n_items // world, (rank + 1) * n_items // world
s, i = ops.score_topk(U, None, V[lo:hi].contiguous(), k, item_base=lo)
gs = torch.empty((world, n_users, k), device=dev)
gi = torch.empty((world, n_users, k), dtype=torch.int32, device=dev)
ws_bytes = L.crh_comm_allgather_topk_workspace_bytes(world, n_users, k)
assert ws_bytes == (world + 1) * n_users * 2 * k * 4
ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
assert L.crh_comm_allgather_topk(comm, s.data_ptr(), i.data_ptr(), n_users, k, gs.data_ptr(), gi.data_ptr(),
                                 ws.data_ptr(), ws_bytes - 1, st) != 0          # a short workspace is refused, not overrun
_lib.check(L.crh_comm_allgather_topk(comm, s.data_ptr(), i.data_ptr(), n_users, k, gs.data_ptr(), gi.data_ptr(),
                                     ws.data_ptr(), ws_bytes, st), "crh_comm_allgather_topk")
ms, mi = ops.merge_topk(gs, gi, k)
ws, wi = ops.score_topk(U, None, V, k)
x = torch.full((1000,), float(rank + 1), device=dev)
_lib.check(L.crh_comm_allreduce_f32(comm, x.data_ptr(), x.numel(), st), "crh_comm_allreduce_f32")
cap, dd = 37, 16
rid = torch.arange(cap, dtype=torch.int32, device=dev) * world + rank
rrow = torch.full((cap, dd), float(rank), device=dev)
gid, grow = torch.empty(world * cap, dtype=torch.int32, device=dev), torch.empty((world * cap, dd), device=dev)
_lib.check(L.crh_comm_allgather_rows(comm, rid.data_ptr(), rrow.data_ptr(), cap, dd, gid.data_ptr(), grow.data_ptr(), st),
           "crh_comm_allgather_rows")
torch.cuda.synchronize()
assert all(torch.equal(gid[r * cap:(r + 1) * cap], torch.arange(cap, dtype=torch.int32, device=dev) * world + r) and
           float(grow[r * cap:(r + 1) * cap].min()) == float(r) == float(grow[r * cap:(r + 1) * cap].max()) for r in range(world))
torch.cuda.synchronize()
assert torch.equal(mi, wi) and torch.equal(ms.view(torch.int32), ws.view(torch.int32)), "shards + C-ABI all-gather + merge != one rank"
assert float(x[0]) == world * (world + 1) / 2 and float(x.min()) == float(x.max())
_lib.check(L.crh_comm_destroy(comm), "crh_comm_destroy")
print("COMM_OK", rank, world)
'''


def _comm_two_ranks(tmp_path):
    script = tmp_path / "comm_worker.py"
    script.write_text(_COMM_WORKER)
    env = dict(os.environ, CR_ROOT=ROOT, OMP_NUM_THREADS="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(r), "2", str(tmp_path / "uid.bin")], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=600) for p in procs]
    return procs, outs, "".join(o[0] for o in outs)


def test_comm_c_abi_two_ranks(tmp_path):
    """crh_comm_unique_id / _init / _allgather_topk / _allreduce_f32 / _destroy driven by TWO processes with no
    torch.distributed anywhere (what a non-Python caller of the C ABI does): item shards ranked per rank, the packed
    top-k exchanged by the library's RCCL all-gather, crh_merge_topk == the one-rank ranking, bit for bit.  Needs two
    GPUs: RCCL refuses two ranks on one device ("Duplicate GPU detected"); the next test pins that refusal down."""
    n_gpus = torch.cuda.device_count()
    if n_gpus < 2:
        pytest.skip(f"needs 2 GPUs, found {n_gpus}")
    procs, outs, text = _comm_two_ranks(tmp_path)
    assert all(p.returncode == 0 for p in procs), (text[-2000:], outs[0][1][-3000:], outs[1][1][-3000:])
    assert "COMM_OK 0 2" in text and "COMM_OK 1 2" in text


def test_comm_c_abi_two_ranks_on_one_gpu_are_refused(tmp_path):
    """The documented limitation of the two-rank C-ABI exchange on a one-GPU box: the ranks get a named error from
    crh_comm_init (RCCL refuses two ranks on one device) and exit cleanly -- no hang, no crash."""
    n_gpus = torch.cuda.device_count()
    if n_gpus >= 2:
        pytest.skip(f"{n_gpus} GPUs: the two ranks get one each (test_comm_c_abi_two_ranks)")
    procs, outs, text = _comm_two_ranks(tmp_path)
    assert all(p.returncode == 0 for p in procs), (text[-2000:], outs[0][1][-3000:], outs[1][1][-3000:])
    assert "COMM_INIT_REFUSED" in text and "COMM_OK" not in text, text[-2000:]


def test_comm_c_abi_one_rank_packed_allgather(tmp_path):
    """The same worker as ONE rank: what a one-GPU box can run of the C-ABI exchange on real hardware -- RCCL
    communicator of world 1, the pack kernel, ONE ncclAllGather of the packed (n_users, 2k) words, the unpack kernel,
    crh_merge_topk over the single gathered list == the direct ranking, bit for bit; the short-workspace refusal."""
    script = tmp_path / "comm_worker.py"
    script.write_text(_COMM_WORKER)
    env = dict(os.environ, CR_ROOT=ROOT, OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, str(script), "0", "1", str(tmp_path / "uid.bin")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0 and "COMM_OK 0 1" in out.stdout, (out.stdout[-2000:], out.stderr[-3000:])


def test_private_workspace_survives_bigger_calls_between_graph_replays():
    """a captured epoch keeps the raw pointer of its BPR scratch; a larger scoring call between replays
    must not move it (the engines own their scratch, the shared one is per stream and never captured)."""
    from coldrec_amd import ops
    from coldrec_amd.train import EpochRunner, LGCNEngine
    from coldrec_amd.util.databuilder import bipartite_norm_adj_csr
    rng = np.random.default_rng(4)
    n_u, n_i, d, B, n = 200, 300, 32, 256, 256 * 4
    pairs = np.unique(np.stack([rng.integers(0, n_u, 3000), rng.integers(0, n_i, 3000)], 1), axis=0)
    rowptr, col, val = bipartite_norm_adj_csr(pairs[:, 0], pairs[:, 1], n_u, n_i)
    U0 = (rng.standard_normal((n_u, d)) * 0.1).astype(np.float32)
    V0 = (rng.standard_normal((n_i, d)) * 0.1).astype(np.float32)
    a = LGCNEngine(U0, V0, rowptr, col, val, 2, 1e-2, 1e-3, DEV)
    b = LGCNEngine(U0, V0, rowptr, col, val, 2, 1e-2, 1e-3, DEV)
    ra, rb = EpochRunner(a, n, B), EpochRunner(b, n, B, use_graph=False)
    big_u = torch.randn(70000, 64, device=DEV)
    big_v = torch.randn(90000, 64, device=DEV)
    for e in range(4):
        u, i, j = _triples(rng, n_u, n_i, n)
        ra.run(u, i, j)
        rb.run(u, i, j)
        if e >= 1:
            ops.score_topk(big_u, None, big_v, 20)                    # grows the shared scratch after the capture
            junk = [torch.full((1 << 20,), float("nan"), device=DEV) for _ in range(8)]   # reuse freed blocks
            del junk
    torch.cuda.synchronize()
    assert ra.graph is not None
    assert torch.equal(a.E, b.E)
