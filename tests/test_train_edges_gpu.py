"""Edges of the training kernels (coldrec_amd/csrc/bpr.hip, bpr_plan.hip, optim.hip, mf_step.hip, l2_reg.hip, spmm.hip's SGD epilogue -- the SpMM's own
widths, cuts and heavy-row sum tree are tests/test_spmm_edges_gpu.py): the shapes, widths,
grid caps, heavy-row thresholds and row-ownership splits where a change of lane mapping, ownership or reduction order would
otherwise go unnoticed.  Every kernel is driven through coldrec_amd.ops or the C ABI and compared with either

  * an fp64 NumPy reference (oracle/oracle_np.py where it has the formula), to a tolerance derived in the test's docstring, or
  * a bitwise identity the code promises in its own comments (owned == plain, lazy == dense, epilogue == unfused, repeat ==
    first run, fma order of the oracle).

Tables that kernels write are allocated with a guard row before and after (filled with a sentinel) and must come back with
the guard rows untouched: no lane writes past the end of a row, and no idle lane of a lane group writes at all."""
import functools
import math
import os

import numpy as np
import pytest
import torch

from oracle import oracle_np as orc
from tests.test_train_gpu import _plan_views

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 2.0 ** -24                       # unit roundoff of fp32
SENT = -777.25                         # guard-row sentinel (exactly representable)


def t(a, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        x = x.to(dtype)
    return x.to(DEV)


def bits(x):
    return x.contiguous().view(torch.int32)


def beq(a, b):
    """bitwise equality of two fp32 tensors (torch.equal would call -0.0 == 0.0 and NaN != NaN)"""
    return torch.equal(bits(a), bits(b))


def guarded(rows, d, fill=0.0):
    """(buffer, view): a (rows, d) fp32 table between two guard rows holding SENT"""
    buf = torch.full((rows + 2, d), SENT, dtype=torch.float32, device=DEV)
    buf[1:-1] = fill
    return buf, buf[1:-1]


def guards_intact(buf):
    return bool((buf[0] == SENT).all()) and bool((buf[-1] == SENT).all())


def heavy_T():
    from coldrec_amd import _lib
    return int(_lib.lib().crh_bpr_heavy_threshold())


def bpr_scale(d):
    """entry scale that keeps the score differences x = u.(p - n) O(1) at every width (no saturated sigmoids)"""
    return (2.0 * d) ** -0.25


def rand_tables(rng, n_u, n_i, d):
    s = bpr_scale(d)
    return ((rng.standard_normal((n_u, d)) * s).astype(np.float32), (rng.standard_normal((n_i, d)) * s).astype(np.float32))


def rand_triples(rng, n_u, n_i, B, hot=0.3):
    u = rng.integers(0, n_u, B).astype(np.int32)
    i = np.where(rng.random(B) < hot, rng.integers(0, 3, B), rng.integers(0, n_i, B)).astype(np.int32)
    j = rng.integers(0, n_i, B).astype(np.int32)
    return u, i, np.where(j == i, (j + 1) % n_i, j).astype(np.int32)


def check_bpr(loss, gU, gV, U, V, ui, pi, ni, reg):
    """tolerances of tests/test_train_gpu.py::test_bpr_fwd_bwd_vs_oracle: losses 1e-5 (north_star); gradients are fp32 sums
    with cancellation in a different order from fp64's, 1e-4 relative plus 2e-6 of the largest entry"""
    bpr, l2, wU, wV, _ = orc.bpr_l2_fwd_bwd(U, V, ui, pi, ni, reg)
    np.testing.assert_allclose(loss[0], bpr, rtol=1e-5)
    np.testing.assert_allclose(loss[1], l2, rtol=1e-5)
    sc = max(np.abs(wU).max(), np.abs(wV).max())
    np.testing.assert_allclose(gU, wU, rtol=1e-4, atol=2e-6 * sc)
    np.testing.assert_allclose(gV, wV, rtol=1e-4, atol=2e-6 * sc)
    return wU, wV


def slot_rows(plan_np, n_u_table):
    """table row of every row slot w of a plan (users first, item rows offset by the user table's rows)"""
    pv = _plan_views(plan_np)
    return np.concatenate([pv["urow"].astype(np.int64), n_u_table + pv["irow"].astype(np.int64)])


# ================================================================================================ 1. L2 norm and backward
L2_NS = [1, 3, 4, 5, 1023, (1 << 20) - 4, 1 << 20, (1 << 20) + 4, (1 << 20) + 3, 50_000_003]


@functools.lru_cache(maxsize=2)
def _l2_data(n):
    """values over six decades (|x| in 1e-3 .. 1e3, both signs); the last four are 3e3 so that a lost tail (n % 4
    elements) moves the norm far beyond the bound at every n below 10^7"""
    rng = np.random.default_rng(n)
    x = (10.0 ** rng.uniform(-3.0, 3.0, n)).astype(np.float32)
    x *= np.where(rng.random(n) < 0.5, -1.0, 1.0).astype(np.float32)
    x[-4:] = np.float32(3e3) * np.float32([1, -1, 1, -1])[-min(4, n):]
    x64 = x.astype(np.float64)
    return x, t(x), float(np.sqrt(np.dot(x64, x64)))


def _l2_view(n, off):
    """x as a view starting `off` floats into a 16-byte aligned buffer: off = 0 takes l2_sumsq_kernel's f32x4 path,
    off = 1, 2, 3 its scalar path (what util.utils.l2_reg_loss meets with a view like E[n_u:] when n_u * d % 4 != 0)"""
    x_np, x_dev, nrm = _l2_data(n)
    buf = torch.empty(n + 4, dtype=torch.float32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    x = buf[off:off + n]
    x.copy_(x_dev)
    assert (x.data_ptr() % 16 == 0) == (off == 0)
    return x_np, x, nrm


def l2_norm_bound(n, aligned):
    """Relative error bound of crh_l2_norm_f32 from its summation order (l2_reg.hip:22-46).  Every term x_i^2 >= 0, so an fp32
    sum evaluated along a tree in which each term passes through at most h roundings (its product included) has relative
    error <= h u / (1 - h u).  Per term: the product (1); in the f32x4 path 2 adds inside the 4-vector, then the lane's serial
    chain over ceil(n/4 / threads) vectors and the one tail add; in the scalar path a chain of ceil(n / threads) adds;
    then the 256-lane block tree (6 shuffle levels + 2 cross-wave adds), the finishing block's serial chain over
    ceil(blocks / 256) partials and its own 8-level tree.  sqrt halves the relative error and rounds once more (+u)."""
    blocks = min(max((n // 4 + 255) // 256, 1), 1024)
    threads = blocks * 256
    chain = (math.ceil((n // 4) / threads) + 2 + 1) if aligned else math.ceil(n / threads)
    h = 1 + chain + 8 + math.ceil(blocks / 256) + 8
    return 0.5 * h * U32 / (1 - h * U32) + U32


@pytest.mark.parametrize("off", [0, 1, 2, 3])
@pytest.mark.parametrize("n", L2_NS)
def test_l2_norm_and_backward_vs_fp64(n, off):
    """crh_l2_norm_f32 / crh_l2_reg_bwd_f32 (l2_reg.hip:22 l2_sumsq_kernel: aligned f32x4 path + its n % 4 tail at :32, the
    unaligned scalar path at :34 for views 1-3 floats into a buffer; the 1 024-block cap with grid-stride at :71 for
    n > 2^20; n < 4) against the fp64 norm, to the bound of `l2_norm_bound`; bit-identical when repeated.  Backward
    (l2_reg.hip:49) for grad_out None and a tensor against fp64: c = (reg / rows) * gout / norm costs 3 roundings beyond the
    norm's error, reg as fp32 and rows as float one each, c * x one more: 6 u + the norm bound, relative, elementwise."""
    from coldrec_amd import ops
    x_np, x, want = _l2_view(n, off)
    bound = l2_norm_bound(n, off == 0)
    got = ops.l2_norm(x)
    again = ops.l2_norm(x)
    torch.cuda.synchronize()
    g = float(got.item())
    assert abs(g - want) <= bound * want, (n, off, g, want, abs(g - want) / want, bound)
    assert beq(got, again)
    rtol = 6 * U32 + bound
    reg = 0.02
    for gout in (None, 1.7):
        go = None if gout is None else torch.tensor(gout, dtype=torch.float32, device=DEV)
        gx = ops.l2_reg_bwd(x, reg, got, go).cpu().numpy()
        want_g = x_np.astype(np.float64) * (reg * (1.0 if gout is None else np.float64(np.float32(gout))) / (n * want))
        np.testing.assert_allclose(gx, want_g, rtol=rtol, atol=0)


@pytest.mark.parametrize("n,off", [(5, 1), (1023, 0), ((1 << 20) + 3, 2), ((1 << 20) + 4, 0)])
def test_l2_bwd_accumulate_through_c_abi(n, off):
    """crh_l2_reg_bwd_f32 with accumulate = 1 (l2_reg.hip:54) adds onto an existing gx (rows passed explicitly, here 3):
    gx0 + c * x rounds once more, so |err| <= (6 u + norm bound) |c x| + u |gx0 + c x| elementwise."""
    from coldrec_amd import _lib, ops
    L = _lib.lib()
    x_np, x, want = _l2_view(n, off)
    nrm = ops.l2_norm(x)
    rng = np.random.default_rng(n + off)
    gx0 = (rng.standard_normal(n) * 1e-3).astype(np.float32)
    gx = t(gx0)
    go = torch.tensor([0.5], dtype=torch.float32, device=DEV)
    reg, rows = 0.03, 3
    _lib.check(L.crh_l2_reg_bwd_f32(x.data_ptr(), n, rows, reg, nrm.data_ptr(), go.data_ptr(), gx.data_ptr(), 1,
                                    _lib.current_stream()), "crh_l2_reg_bwd_f32")
    torch.cuda.synchronize()
    cx = x_np.astype(np.float64) * (np.float64(np.float32(reg)) * 0.5 / (rows * want))
    res = gx0.astype(np.float64) + cx
    tol = (6 * U32 + l2_norm_bound(n, off == 0)) * np.abs(cx) + U32 * np.abs(res)
    err = np.abs(gx.cpu().numpy() - res)
    assert (err <= tol).all(), (n, off, float((err / np.maximum(tol, 1e-300)).max()))


@pytest.mark.parametrize("n,off", [(1, 0), (5, 1), ((1 << 20) + 3, 3), ((1 << 20) + 4, 0)])
def test_l2_zero_tensor_gives_zero_gradient(n, off):
    """|0|_F = 0 exactly and its gradient is exactly 0 -- not NaN -- as autograd's norm backward returns (l2_reg.hip:52);
    with accumulate = 1 the existing gx is left as it was, bit for bit."""
    from coldrec_amd import _lib, ops
    buf = torch.zeros(n + 4, dtype=torch.float32, device=DEV)
    x = buf[off:off + n]
    nrm = ops.l2_norm(x)
    gx = ops.l2_reg_bwd(x, 0.1, nrm, None)
    torch.cuda.synchronize()
    assert float(nrm.item()) == 0.0
    assert bool(torch.isfinite(gx).all()) and not bool(gx.any())
    g0 = torch.linspace(-1, 1, n, device=DEV)
    g1 = g0.clone()
    L = _lib.lib()
    _lib.check(L.crh_l2_reg_bwd_f32(x.data_ptr(), n, 1, 0.1, nrm.data_ptr(), None, g1.data_ptr(), 1, _lib.current_stream()),
               "crh_l2_reg_bwd_f32")
    torch.cuda.synchronize()
    assert beq(g0, g1)


# ================================================================================================ 2. lane-group widths
WIDTHS = [4, 12, 20, 36, 68, 132, 196, 252, 256]      # pick_group (train_common.h): idle lanes just past a power of two
WIDE = [260, 384, 512]                                # a 64-lane group walks each row twice (c += G loops)


@pytest.mark.parametrize("d", WIDTHS + WIDE)
def test_widths_bpr_atomics_vs_fp64(d):
    """Atomics forward / backward (bpr.hip: bpr_fwd_kernel, bpr_bwd_kernel) at every lane-group width, d > 256
    included, against fp64 with test_bpr_fwd_bwd_vs_oracle's tolerances; the gradient tables sit between guard rows and
    untouched rows stay exactly 0 (no idle lane, no lane past the row, writes anything)."""
    from coldrec_amd import ops
    rng = np.random.default_rng(d)
    n_u, n_i, B = 150, 211, 700
    U, V = rand_tables(rng, n_u, n_i, d)
    ui, pi, ni = rand_triples(rng, n_u, n_i, B)
    bu, gU = guarded(n_u, d)
    bv, gV = guarded(n_i, d)
    loss = ops.bpr_fwd_bwd(t(U), t(V), t(V), t(ui), t(pi), t(ni), 0.01, gU, gV, gV)
    torch.cuda.synchronize()
    assert guards_intact(bu) and guards_intact(bv)
    gu, gv = gU.cpu().numpy(), gV.cpu().numpy()
    check_bpr(loss.cpu().numpy(), gu, gv, U, V, ui, pi, ni, 0.01)
    assert not gu[np.setdiff1d(np.arange(n_u), ui)].any()
    assert not gv[np.setdiff1d(np.arange(n_i), np.concatenate([pi, ni]))].any()


@pytest.mark.parametrize("d", WIDTHS)
def test_widths_plan_backward_vs_fp64_and_repeat(d):
    """Plan backward (bpr.hip: bpr_bwd_rows_kernel, its light-row and its heavy-row loop -- three hot items put rows
    on the heavy list) at every width up to 256: fp64 with the tolerances above, two runs bit-identical, guard rows intact,
    untouched rows exactly 0."""
    from coldrec_amd import ops
    rng = np.random.default_rng(100 + d)
    n_u, n_i, B = 150, 211, 700
    U, V = rand_tables(rng, n_u, n_i, d)
    ui, pi, ni = rand_triples(rng, n_u, n_i, B)
    plan = ops.build_plans_device(t(ui), t(pi), t(ni), B)[0]
    assert len(_plan_views(plan.cpu().numpy())["heavy"]) > 0
    tU, tV = t(U), t(V)
    outs = []
    for _ in range(2):
        bu, gU = guarded(n_u, d)
        bv, gV = guarded(n_i, d)
        loss = ops.bpr_fwd_bwd(tU, tV, tV, t(ui), t(pi), t(ni), 0.01, gU, gV, gV, plan=plan)
        torch.cuda.synchronize()
        assert guards_intact(bu) and guards_intact(bv)
        outs.append((loss.clone(), gU, gV))
    assert all(beq(a, b) for a, b in zip(outs[0], outs[1]))
    gu, gv = outs[0][1].cpu().numpy(), outs[0][2].cpu().numpy()
    check_bpr(outs[0][0].cpu().numpy(), gu, gv, U, V, ui, pi, ni, 0.01)
    assert not gu[np.setdiff1d(np.arange(n_u), ui)].any()
    assert not gv[np.setdiff1d(np.arange(n_i), np.concatenate([pi, ni]))].any()


@pytest.mark.parametrize("d", WIDE)
def test_widths_beyond_256_refused_where_unsupported(d):
    """The plan backward holds one 16-B slice per lane (d <= 256) and refuses wider tables loudly (bpr.hip: bpr_launch), as
    does the row exchange of the ownership split (crh_rows_pack_f32, crh_rows_unpack_f32); MFEngine does not offer the one-launch step (whose entry
    point, mf_step.hip's mf_step_run, refuses d > 256) for such tables."""
    from coldrec_amd import ops
    rng = np.random.default_rng(d)
    U, V = rand_tables(rng, 10, 12, d)
    ui, pi, ni = rand_triples(rng, 10, 12, 16)
    plan = ops.build_plans_device(t(ui), t(pi), t(ni), 16)[0]
    gU, gV = torch.zeros((10, d), device=DEV), torch.zeros((12, d), device=DEV)
    with pytest.raises(RuntimeError, match="d <= 256"):
        ops.bpr_fwd_bwd(t(U), t(V), t(V), t(ui), t(pi), t(ni), 0.01, gU, gV, gV, plan=plan)
    cap = ops.rows_pack_cap(16, 2)
    ids, rows = torch.full((cap,), -1, dtype=torch.int32, device=DEV), torch.zeros((cap, d), device=DEV)
    with pytest.raises(RuntimeError, match="crh_rows_pack_f32"):
        ops.rows_pack(torch.cat([gU, gV]), plan, 16, 10, 2, 0, ids, rows)
    with pytest.raises(RuntimeError, match="crh_rows_unpack_f32"):
        ops.rows_unpack(torch.cat([gU, gV]), ids, rows)
    from coldrec_amd.train import MFEngine
    assert not MFEngine(U, V, 1e-2, 1e-3, DEV).can_fuse(1, 16)


@pytest.mark.parametrize("d", WIDTHS + WIDE)
def test_widths_optimisers_bitwise_vs_oracle_order(d):
    """optim.hip's sgd_dense_kernel, sgd_rows_kernel, adam_dense_kernel and adam_rows_kernel at every width: bit for bit the
    oracle's op order (oracle_np.sgd_dense: one fma; oracle_np.adam_dense: torch's separate rounded ops), as
    test_sgd_dense_is_one_fma_per_element.  The rows kernels touch exactly the plan's rows (guard rows and untouched rows
    unchanged, bitwise) and clear the gradient rows they consumed."""
    from coldrec_amd import ops
    rng = np.random.default_rng(200 + d)
    n_u, n_i, B, lr = 40, 57, 30, 0.0123
    R = n_u + n_i
    E0 = (rng.standard_normal((R, d)) * 0.1).astype(np.float32)
    ui, pi, ni = rand_triples(rng, n_u, n_i, B)
    plan = ops.build_plans_device(t(ui), t(pi), t(ni), B)[0]
    rows = slot_rows(plan.cpu().numpy(), n_u)
    touched = np.zeros(R, bool)
    touched[rows] = True
    G0 = np.zeros((R, d), np.float32)
    G0[touched] = rng.standard_normal((int(touched.sum()), d)).astype(np.float32) * 1e-2
    # sgd_dense over the flat table
    p, g = t(E0), t(G0)
    ops.sgd_dense(p, g, lr)
    assert beq(p, t(orc.sgd_dense(E0, G0, lr))) and not bool(g.any())
    # sgd_rows between guard rows
    pb, p = guarded(R, d)
    p.copy_(t(E0))
    gb, g = guarded(R, d)
    g.copy_(t(G0))
    ops.sgd_rows(p, g, plan, B, n_u, lr)
    torch.cuda.synchronize()
    assert guards_intact(pb) and guards_intact(gb)
    assert beq(p, t(orc.sgd_dense(E0, G0, lr))) and not bool(g.any())
    # adam_dense, three steps, against the oracle's op order
    p, m, v = t(E0), torch.zeros((R, d), device=DEV), torch.zeros((R, d), device=DEV)
    wp, wm, wv = E0, np.zeros_like(E0), np.zeros_like(E0)
    for step in (1, 2, 3):
        Gs = G0 * np.float32(step)
        ops.adam_dense(p, t(Gs), m, v, step, lr=lr)
        wp, wm, wv = orc.adam_dense(wp, Gs, wm, wv, step, lr=lr)
    assert beq(p, t(wp)) and beq(m, t(wm)) and beq(v, t(wv))
    # adam_rows: step 1 on the plan's rows, then a flush to step 2 (every row replays a zero-gradient step 2)
    sc = np.zeros((4, 2), np.float32)
    sc[1:] = ops.adam_step_scalars(1, 3, lr)
    sct = t(sc)
    pb, p = guarded(R, d)
    p.copy_(t(E0))
    mb, m = guarded(R, d)
    vb, v = guarded(R, d)
    gb, g = guarded(R, d)
    g.copy_(t(G0))
    last = torch.zeros(R, dtype=torch.int32, device=DEV)
    ops.adam_rows(p, None, m, v, last, plan, B, n_u, 1, sct, mode=0)
    ops.adam_rows(p, g, m, v, last, plan, B, n_u, 1, sct, mode=1)
    torch.cuda.synchronize()
    assert all(guards_intact(b) for b in (pb, mb, vb, gb)) and not bool(g.any())
    wp, wm, wv = orc.adam_dense(E0, G0, np.zeros_like(E0), np.zeros_like(E0), 1, lr=lr)
    assert beq(p[t(touched)], t(wp[touched])) and beq(m[t(touched)], t(wm[touched]))
    assert beq(p[t(~touched)], t(E0[~touched])) and not bool(m[t(~touched)].any())
    assert np.array_equal(last.cpu().numpy(), touched.astype(np.int32))
    ops.adam_rows(p, None, m, v, last, None, 0, n_u, 2, sct, mode=2)
    torch.cuda.synchronize()
    wp, wm, wv = orc.adam_dense(wp, np.zeros_like(E0), wm, wv, 2, lr=lr)
    assert beq(p, t(wp)) and beq(m, t(wm)) and beq(v, t(wv))
    assert all(guards_intact(b) for b in (pb, mb, vb)) and bool((last == 2).all())


# ================================================================================================ 3. forward grid cap
@pytest.mark.parametrize("d,B,use_plan", [(256, 4096, True), (256, 4097, True), (256, 8192, True),
                                          (128, 8193, False), (128, 20_000, False)])
def test_forward_grid_cap(d, B, use_plan):
    """The forward grid is capped at BPR_MAX_BLOCKS = 1 024 (bpr.hip: bpr_launch) and grid-strides beyond it (bpr_fwd_kernel); the
    backward's batch_totals then reduces 1 024 partials.  d = 256 (4 triples per block) reaches the cap at B = 4 096,
    d = 128 (8 per block) at 8 192.  Losses 1e-5 against fp64, gradients as test_bpr_fwd_bwd_vs_oracle."""
    from coldrec_amd import ops
    assert ops.bpr_fwd_parts(B, d) == min(1024, -(-B // (256 // (64 if d == 256 else 32))))
    rng = np.random.default_rng(B)
    n_u, n_i = 3000, 5000
    U, V = rand_tables(rng, n_u, n_i, d)
    ui, pi, ni = rand_triples(rng, n_u, n_i, B, hot=0.05)
    plan = ops.build_plans_device(t(ui), t(pi), t(ni), B)[0] if use_plan else None
    gU, gV = torch.zeros((n_u, d), device=DEV), torch.zeros((n_i, d), device=DEV)
    tV = t(V)
    loss = ops.bpr_fwd_bwd(t(U), tV, tV, t(ui), t(pi), t(ni), 0.01, gU, gV, gV, plan=plan)
    torch.cuda.synchronize()
    check_bpr(loss.cpu().numpy(), gU.cpu().numpy(), gV.cpu().numpy(), U, V, ui, pi, ni, 0.01)


# ================================================================================================ 4. heavy-row threshold
HEAVY_NU, HEAVY_NI = 300, 500


def heavy_batch(rng, T, B):
    """B triples in which user rows 0, 1, 2 hold exactly T-1, T, T+1 entries, item rows 0, 1, 2 exactly that many as
    POSITIVES, item rows 3, 4, 5 that many as NEGATIVES, item row 6 T+1 entries of both roles; every other entry comes
    from user rows >= 3 and item rows >= 7.  The triples are shuffled."""
    us = np.repeat([0, 1, 2], [T - 1, T, T + 1])
    ps = np.concatenate([np.repeat([0, 1, 2], [T - 1, T, T + 1]), np.full((T + 1) // 2, 6)])
    ns = np.concatenate([np.repeat([3, 4, 5], [T - 1, T, T + 1]), np.full(T + 1 - (T + 1) // 2, 6)])
    assert B >= len(us) and B >= len(ps) + len(ns)
    u = rng.integers(3, HEAVY_NU, B)
    u[:len(us)] = us
    i = rng.integers(7, HEAVY_NI, B)
    j = rng.integers(7, HEAVY_NI, B)
    j = np.where(j == i, 7 + (j - 7 + 1) % (HEAVY_NI - 7), j)
    i[:len(ps)] = ps                                       # fixed positives and negatives in different triples
    j[len(ps):len(ps) + len(ns)] = ns
    perm = rng.permutation(B)
    u, i, j = (x[perm].astype(np.int32) for x in (u, i, j))
    cu, ci = np.bincount(u, minlength=HEAVY_NU), np.bincount(np.concatenate([i, j]), minlength=HEAVY_NI)
    assert list(cu[:3]) == [T - 1, T, T + 1] and list(ci[:7]) == [T - 1, T, T + 1, T - 1, T, T + 1, T + 1]
    assert list(np.bincount(i, minlength=7)[:7]) == [T - 1, T, T + 1, 0, 0, 0, (T + 1) // 2]
    assert (i != j).all()
    return u, i, j


def one_user_batch(rng, B=8192):
    """B triples that all belong to user row 0 (one row holds every user-side entry of the batch)"""
    i = rng.integers(0, HEAVY_NI, B)
    j = rng.integers(0, HEAVY_NI, B)
    return np.zeros(B, np.int32), i.astype(np.int32), np.where(j == i, (j + 1) % HEAVY_NI, j).astype(np.int32)


def heavy_epoch(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "edges":
        B = 600
        b1, b2 = heavy_batch(rng, heavy_T(), B), heavy_batch(rng, heavy_T(), B)
        return B, tuple(np.concatenate([x, y]) for x, y in zip(b1, b2))
    return 8192, one_user_batch(rng)


@pytest.mark.parametrize("kind", ["edges", "one_user"])
@pytest.mark.parametrize("d", [20, 64])
def test_heavy_threshold_plan_backward_and_sgd_rows(kind, d):
    """Rows at exactly T - 1, T and T + 1 entries (T = crh_bpr_heavy_threshold(), as positive, as negative, and mixed) and
    one user row holding all 8 192 entries of a batch: the plan's heavy list is exactly the rows above T, the plan backward
    (bpr.hip: bpr_bwd_rows_kernel, light rows and heavy rows) equals fp64 within test_bpr_fwd_bwd_vs_oracle's tolerances, repeats
    bit for bit, and agrees with the atomics backward within the same bounds; sgd_rows on the result is bit for bit
    oracle_np.sgd_dense over the whole table."""
    from coldrec_amd import ops
    T = heavy_T()
    B, (u, i, j) = heavy_epoch(kind, 7 + d)
    u, i, j = u[:B], i[:B], j[:B]
    rng = np.random.default_rng(d)
    U, V = rand_tables(rng, HEAVY_NU, HEAVY_NI, d)
    plan = ops.build_plans_device(t(u), t(i), t(j), B)[0]
    pv = _plan_views(plan.cpu().numpy())                   # (asserts heavy list == rows with more than T entries)
    cnt = np.concatenate([np.diff(pv["uptr"]), np.diff(pv["iptr"])])
    if kind == "edges":
        assert sorted(cnt[pv["heavy"]].tolist()).count(T + 1) >= 4 and (cnt == T).sum() >= 3
    else:
        assert pv["heavy"][0] == 0 and cnt[0] == B
    E = t(np.concatenate([U, V]))
    outs = []
    for p in (plan, plan, None):
        G = torch.zeros_like(E)
        loss = ops.bpr_fwd_bwd(E[:HEAVY_NU], E[HEAVY_NU:], E[HEAVY_NU:], t(u), t(i), t(j), 0.01, G[:HEAVY_NU], G[HEAVY_NU:],
                               G[HEAVY_NU:], plan=p)
        torch.cuda.synchronize()
        outs.append((loss.clone(), G))
    assert beq(outs[0][0], outs[1][0]) and beq(outs[0][1], outs[1][1])
    for loss, G in (outs[0], outs[2]):
        g = G.cpu().numpy()
        check_bpr(loss.cpu().numpy(), g[:HEAVY_NU], g[HEAVY_NU:], U, V, u, i, j, 0.01)
    G = outs[0][1]
    Gn, En = G.cpu().numpy(), E.cpu().numpy()
    ops.sgd_rows(E, G, plan, B, HEAVY_NU, 0.05)
    torch.cuda.synchronize()
    assert beq(E, t(orc.sgd_dense(En, Gn, 0.05))) and not bool(G.any())


def _fp64_sgd_replay(U0, V0, batches, reg, lr):
    """fp64 gradients (oracle) and p <- p - lr g per step; returns (per-step [bpr, l2], final table, elementwise bound).
    Bound per step: the fp32 gradient element is within test_bpr_fwd_bwd_vs_oracle's bound of fp64 (1e-4 |g| + 2e-6 max|g|),
    times lr, and the fma rounds once more (u |p|); the tables then drift apart by those amounts, which moves the NEXT step's
    gradients by a second-order amount of the same kind -- a factor 2 over the summed first-order terms covers it."""
    n_u = U0.shape[0]
    E = np.concatenate([U0, V0]).astype(np.float64)
    tol = np.zeros_like(E)
    losses = []
    for (u, i, j) in batches:
        bpr, l2, gU, gV, _ = orc.bpr_l2_fwd_bwd(E[:n_u], E[n_u:], u, i, j, reg)
        g = np.concatenate([gU, gV])
        losses.append((bpr, l2))
        E = E - lr * g
        tol += lr * (1e-4 * np.abs(g) + 2e-6 * np.abs(g).max()) + U32 * np.abs(E)
    return np.array(losses), E, 2 * tol


@pytest.mark.parametrize("opt", ["adam", "sgd"])
@pytest.mark.parametrize("kind", ["edges", "one_user"])
def test_heavy_threshold_one_launch_step(kind, opt):
    """The one-launch step (mf_step.hip: mf_step_kernel; its light loop skips heavy rows, its heavy blocks take them) with
    Adam and with SGD, on the batches above, through EpochRunner(fused=True) against the three-kernel step
    (fused=False: plan backward + adam_dense / sgd_rows): the tolerances of test_fused_mf_step_matches_three_kernel_step
    (losses 2e-6, tables 2e-4 + 1e-5 of the largest entry: the two differ in the summation order of the norms only); two
    fused runs bit-identical; the first step's losses against fp64 at 1e-5; for SGD every step's losses (1e-5) and the
    final tables against an fp64 replay (bound derived in _fp64_sgd_replay).  Two epochs: eager, then captured."""
    from coldrec_amd.train import EpochRunner, MFEngine
    B, ep = heavy_epoch(kind, 31)
    n_rec = ep[0].shape[0]
    rng = np.random.default_rng(5)
    U0, V0 = rand_tables(rng, HEAVY_NU, HEAVY_NI, 64)
    lr, reg = (1e-2, 1e-3) if opt == "adam" else (0.5, 1e-3)
    runs = {}
    for tag, fused in (("fused", True), ("fused2", True), ("plain", False)):
        eng = MFEngine(U0, V0, lr, reg, DEV, optimizer=opt)
        runner = EpochRunner(eng, n_rec, B, fused=fused)
        assert eng.fused == fused
        losses = [runner.run(*ep).clone() for _ in range(2)]
        torch.cuda.synchronize()
        runs[tag] = (torch.cat(losses).cpu().numpy(), eng.E.cpu().numpy()) + \
            ((eng.M.cpu().numpy(), eng.V.cpu().numpy()) if opt == "adam" else ())
    for a, b in zip(runs["fused"], runs["fused2"]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    np.testing.assert_allclose(runs["fused"][0], runs["plain"][0], rtol=2e-6, atol=1e-9)
    for a, b in zip(runs["fused"][1:], runs["plain"][1:]):
        np.testing.assert_allclose(a, b, rtol=2e-4, atol=1e-5 * np.abs(b).max())
    batches = [tuple(x[lo:lo + B] for x in ep) for _ in range(2) for lo in range(0, n_rec, B)]
    bpr, l2, _, _, _ = orc.bpr_l2_fwd_bwd(U0, V0, *batches[0], reg)
    for tag in ("fused", "plain"):
        np.testing.assert_allclose(runs[tag][0][0], [bpr, l2], rtol=1e-5)
    if opt == "sgd":
        want_loss, E64, tol = _fp64_sgd_replay(U0, V0, batches, reg, lr)
        for tag in ("fused", "plain"):
            np.testing.assert_allclose(runs[tag][0], want_loss, rtol=1e-5)
            err = np.abs(runs[tag][1] - E64)
            assert (err <= tol).all(), (tag, float((err / tol).max()))


# ================================================================================================ 5. row-ownership partition
def _owned_case(seed, d, kind):
    """(tables, triples, plan, batch): 'heavy' = a heavy_batch (rows at T-1 / T / T+1 and hot items); 'short' = the
    short LAST batch of an epoch, 37 triples under a plan laid out for 600 (layout stride > batch)"""
    from coldrec_amd import ops
    rng = np.random.default_rng(seed)
    U, V = rand_tables(rng, HEAVY_NU, HEAVY_NI, d)
    if kind == "heavy":
        B = 600
        u, i, j = heavy_batch(rng, heavy_T(), B)
        plan = ops.build_plans_device(t(u), t(i), t(j), B)[0]
        return U, V, (u, i, j), plan, B
    L, S = 600, 37
    u, i, j = rand_triples(rng, HEAVY_NU, HEAVY_NI, L + S, hot=0.5)
    plans = ops.build_plans_device(t(u), t(i), t(j), L)
    assert plans.shape[0] == 2 and int(plans[1, 2]) == L
    return U, V, (u[L:], i[L:], j[L:]), plans[1].contiguous(), S


def check_owned_partition(U, V, tri, plan, B, own_mod):
    """The row-ownership split (bpr.hip: the own_mod tests of bpr_bwd_rows_kernel's light and heavy loops; rows_pack_kernel,
    rows_unpack_kernel) against the plain plan backward, all bitwise: for every own_rem, bpr_bwd_owned STORES exactly the rows of plan
    slots w % own_mod == own_rem with the plain backward's bits and leaves every other row (sentinel-filled) untouched, and
    reports the same loss; the owned slots partition the plan; rows_pack writes the owned slots' rows in slot order (-1
    past the plan, whose rows it leaves alone) as bitwise copies; packing every rank, concatenating (the all-gather) and
    unpacking into a zeroed table rebuilds the plain gradient table.  Returns None or a description of the first mismatch."""
    from coldrec_amd import ops
    n_u, d = U.shape[0], U.shape[1]
    R = n_u + V.shape[0]
    E = t(np.concatenate([U, V]))
    tu, ti, tj = (t(x) for x in tri)
    G_want, loss_want = torch.zeros_like(E), torch.zeros(2, device=DEV)
    ops.bpr_fwd_bwd(E[:n_u], E[n_u:], E[n_u:], tu, ti, tj, 0.01, G_want[:n_u], G_want[n_u:], G_want[n_u:], loss_want,
                    plan=plan, workspace=ops.bpr_workspace(B, DEV))
    ws, sums = ops.bpr_workspace(B, DEV), torch.zeros(4, device=DEV)
    ops.bpr_fwd(E[:n_u], E[n_u:], E[n_u:], tu, ti, tj, sums, ws)
    rows = slot_rows(plan.cpu().numpy(), n_u)
    cap = ops.rows_pack_cap(B, own_mod)
    seen = np.zeros(R, np.int32)
    all_ids, all_rows = [], []
    for rem in range(own_mod):
        gb, G = guarded(R, d, fill=SENT)
        loss = torch.zeros(2, device=DEV)
        ops.bpr_bwd_owned(E[:n_u], E[n_u:], tu, ti, tj, 0.01, sums, G[:n_u], G[n_u:], loss, ws, plan, own_mod, rem)
        mine = rows[rem::own_mod]
        seen[mine] += 1
        owned = np.zeros(R, bool)
        owned[mine] = True
        om = t(owned)
        if not guards_intact(gb):
            return "owned backward wrote a guard row (rem %d)" % rem
        if not beq(G[om], G_want[om]):
            return "owned rows differ from the plain backward (rem %d)" % rem
        if not bool((G[~om] == SENT).all()):
            return "owned backward wrote a row of another rank (rem %d)" % rem
        if not beq(loss, loss_want):
            return "owned loss differs (rem %d)" % rem
        ids = torch.full((cap,), -5, dtype=torch.int32, device=DEV)
        packed = torch.full((cap, d), SENT, device=DEV)
        ops.rows_pack(G, plan, B, n_u, own_mod, rem, ids, packed)
        want_ids = np.full(cap, -1, np.int64)
        want_ids[:len(mine)] = mine
        if not np.array_equal(ids.cpu().numpy(), want_ids):
            return "rows_pack ids (rem %d)" % rem
        k = len(mine)
        if not beq(packed[:k], G_want[t(mine)]) or not bool((packed[k:] == SENT).all()):
            return "rows_pack rows (rem %d)" % rem
        all_ids.append(ids)
        all_rows.append(packed)
    touched = np.zeros(R, bool)
    touched[rows] = True
    if not (seen[touched] == 1).all() or seen[~touched].any():
        return "owned slots do not partition the plan's rows"
    G_got = torch.zeros_like(E)
    ops.rows_unpack(G_got, torch.cat(all_ids).contiguous(), torch.cat(all_rows).contiguous())
    torch.cuda.synchronize()
    if not beq(G_got, G_want):
        return "pack -> all-gather -> unpack does not rebuild the plain gradient table"
    return None


@pytest.mark.parametrize("kind,own_mod", [("heavy", 2), ("heavy", 3), ("heavy", 8), ("short", 2), ("short", 3), ("short", 8),
                                          ("short", "beyond")])
@pytest.mark.parametrize("d", [20, 64])
def test_row_ownership_partition(d, kind, own_mod):
    """check_owned_partition for own_mod in {2, 3, 8} and one own_mod larger than the plan's touched rows (most ranks own
    nothing; rows_pack then writes only -1 ids), on a batch with rows at the heavy threshold and on a short last batch
    under a longer layout stride (the 'beyond' case on the short batch only: one pass per rank, ~100 ranks there, ~1 000
    on the heavy batch); d = 20 leaves idle lanes in each 8-lane group."""
    U, V, tri, plan, B = _owned_case(d + (0 if kind == "heavy" else 1), d, kind)
    n_rows = int(plan[0]) + int(plan[1])
    mod = n_rows + 3 if own_mod == "beyond" else own_mod
    err = check_owned_partition(U, V, tri, plan, B, mod)
    assert err is None, (err, d, kind, mod)


# ================================================================================================ 6. lazy Adam through adam_rows
@pytest.mark.parametrize("d", [4, 68, 256, 260])
def test_adam_rows_replay_equals_dense_adam(d):
    """crh_adam_rows_f32 driven directly (optim.hip: adam_rows_kernel -- catch-up mode 0, step mode 1, flush mode 2) over 12
    steps with random touched subsets against crh_adam_dense_f32 applied 12 times to the same gradients: p, m, v bit for
    bit.  Two lazy replicas: A flushes at three random steps (each compared whole with the dense tables, then flushed again
    with nothing stale: a no-op, bitwise); B never flushes before the end, so its final flush replays every stale row --
    row 0 (never touched) through all 12 steps, row 1 (touched at step 1 only) through steps 2 .. 12.  last_step ends at 12."""
    from coldrec_amd import ops
    rng = np.random.default_rng(d)
    n_u, n_i, steps, lr = 60, 90, 12, 1e-2
    R = n_u + n_i
    E0 = (rng.standard_normal((R, d)) * 0.1).astype(np.float32)
    sc = np.zeros((steps + 2, 2), np.float32)
    sc[1:] = ops.adam_step_scalars(1, steps + 1, lr)
    sct = t(sc)
    z = lambda: torch.zeros((R, d), device=DEV)                  # noqa: E731
    pd, md, vd = t(E0), z(), z()
    lazy = [dict(p=t(E0), m=z(), v=z(), g=z(), last=torch.zeros(R, dtype=torch.int32, device=DEV)) for _ in range(2)]
    flush_at = set(rng.choice(np.arange(1, steps), 3, replace=False).tolist())
    for s in range(1, steps + 1):
        B = int(rng.integers(3, 40))
        u = rng.integers(2, n_u, B).astype(np.int32)           # user row 0 never, row 1 at step 1 only
        if s == 1:
            u[0] = 1
        i, j = rng.integers(0, n_i, B).astype(np.int32), rng.integers(0, n_i, B).astype(np.int32)
        plan = ops.build_plans_device(t(u), t(i), t(j), B)[0]
        rows = slot_rows(plan.cpu().numpy(), n_u)
        G = np.zeros((R, d), np.float32)
        G[rows] = (rng.standard_normal((len(rows), d)) * 10.0 ** rng.uniform(-4, 0)).astype(np.float32)
        ops.adam_dense(pd, t(G), md, vd, s, lr=lr)
        for k, r in enumerate(lazy):
            ops.adam_rows(r["p"], None, r["m"], r["v"], r["last"], plan, B, n_u, s, sct, mode=0)
            r["g"].copy_(t(G))                                   # what the backward of step s would store
            ops.adam_rows(r["p"], r["g"], r["m"], r["v"], r["last"], plan, B, n_u, s, sct, mode=1)
            assert not bool(r["g"].any())
            if k == 0 and s in flush_at:
                ops.adam_rows(r["p"], None, r["m"], r["v"], r["last"], None, 0, n_u, s, sct, mode=2)
                assert beq(r["p"], pd) and beq(r["m"], md) and beq(r["v"], vd), s
                snap = [r[q].clone() for q in ("p", "m", "v", "last")]
                ops.adam_rows(r["p"], None, r["m"], r["v"], r["last"], None, 0, n_u, s, sct, mode=2)   # nothing stale
                assert all(beq(x, r[q]) for x, q in zip(snap[:3], ("p", "m", "v"))) and torch.equal(snap[3], r["last"])
    b = lazy[1]
    lv = b["last"].cpu().numpy()
    assert lv[0] == 0 and lv[1] == 1 and not beq(b["p"], pd)
    row1 = b["p"][1].clone()
    for r in lazy:
        ops.adam_rows(r["p"], None, r["m"], r["v"], r["last"], None, 0, n_u, steps, sct, mode=2)
    torch.cuda.synchronize()
    for r in lazy:
        assert beq(r["p"], pd) and beq(r["m"], md) and beq(r["v"], vd)
        assert bool((r["last"] == steps).all())
    assert not beq(row1, b["p"][1])                              # row 1 did move in the final flush (11 replayed steps)


# ================================================================================================ 7. SGD epilogue of the SpMM
def _skewed_graph():
    """the Zipf graph of tests/test_train_gpu.py::test_spmm_segment_schedule_on_skewed_graph (rows beyond 1 500 edges)"""
    rng = np.random.default_rng(11)
    n_u, n_i = 3000, 500
    w = 1.0 / np.arange(1, n_i + 1) ** 1.1
    items = rng.choice(n_i, 120_000, p=w / w.sum())
    key = np.unique(rng.integers(0, n_u, 120_000) * n_i + items)
    rowptr, col, val = orc.norm_adj_csr(key // n_i, key % n_i, n_u, n_i)
    assert np.diff(rowptr).max() > 1500
    return rowptr, col, val


@pytest.mark.parametrize("d", [32, 64, 128, 200])
def test_spmm_sgd_epilogue_ops_level(d):
    """crh_spmm_csr_sgd_f32 (spmm.hip:95, the SGD update in the last backward SpMM's epilogue) == crh_spmm_csr_f32 with the
    gradient into a table + crh_sgd_dense_f32, bit for bit on p, acc_out and (zero_acc_in) the cleared acc_in -- on the
    skewed graph with no schedule, the descriptor schedule (giant rows cut into column ranges) and the record stream; the
    SGD twin of test_spmm_adam_epilogue_ops_level.  p also equals oracle_np.sgd_dense on the gradient, bitwise."""
    from coldrec_amd import ops
    rowptr, col, val = _skewed_graph()
    n = len(rowptr) - 1
    rng = np.random.default_rng(d)
    rp, cl, vl = t(rowptr), t(col), t(val)
    x, z = t(rng.standard_normal((n, d)).astype(np.float32)), t(rng.standard_normal((n, d)).astype(np.float32))
    p0n = (rng.standard_normal((n, d)) * 0.1).astype(np.float32)
    p0 = t(p0n)
    lr = 0.037
    for sched in (None, ops.SpmmSchedule(rowptr, DEV), ops.SpmmSchedule(rowptr, DEV, col=cl, val=vl)):
        g = torch.empty_like(x)
        ops.spmm_csr(rp, cl, vl, x, acc_in=z, s_in=0.5, acc_out=g, s_out=0.25, sched=sched)
        p1 = p0.clone()
        ops.sgd_dense(p1, g.clone(), lr, zero_grad=False)
        p2, z2, g2 = p0.clone(), z.clone(), torch.empty_like(x)
        ops.spmm_csr_sgd(rp, cl, vl, x, z2, 0.5, g2, 0.25, sched, p2, lr, zero_acc_in=True)
        assert beq(g, g2) and beq(p1, p2) and not bool(z2.any())
        p3, z3 = p0.clone(), z.clone()
        ops.spmm_csr_sgd(rp, cl, vl, x, z3, 0.5, None, 0.25, sched, p3, lr)
        assert beq(p1, p3) and beq(z3, z)
        assert beq(p1, t(orc.sgd_dense(p0n, g.cpu().numpy(), lr)))


# ================================================================================================ the fuzzer, in the suite
@pytest.mark.parametrize("seed,only", [(606, None), (17, "owned,sgd")])
def test_train_fuzzer_short_run(seed, only):
    """Half a minute of tests/fuzz/fuzz_train_ops.py per arm inside the suite, as test_fuzzer_short_run does for the scoring
    fuzzer: one arm over every case kind, one over the ownership split and the SGD paths only."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cmd = [sys.executable, os.path.join(root, "tests", "fuzz", "fuzz_train_ops.py"), "--minutes", "0.5", "--seed", str(seed)]
    if only:
        cmd += ["--only", only]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "fuzz ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
