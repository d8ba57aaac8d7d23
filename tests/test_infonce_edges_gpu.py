"""GPU: the fused InfoNCE (csrc/infonce.hip) where tests/test_infonce_gpu.py never goes.  Reference: the float64
cancellation-free restatement (tests/infonce_restate.py; tests/test_infonce.py pins it to G18 and to float64 autograd) on
the same inputs.  Bars of the non-peaked cases: test_infonce_gpu.check_against_fp64's -- loss within 1e-5 relative (without
that helper's absolute floor), gradients within 1e-4 x max|g64| and within 2x the error of float32 torch on the formula.

What each group reaches:
  widths      d = 4, 32 | 36, 64 | 68, 96 | 100, 128 | 132, 160 | 164, 192 | 196, 224 | 228, 256: the lowest and highest
              width of every nce_pass_kernel<DP, COL> (DP = ceil32(d)), row and column pass (both gradients are asked for).
              DP = 96, 160, 192, 224 are launched by nothing else: their LD4 / `e / DP`, `e % DP` tile loads, their LDS
              stride DP + 4 and the finish's `lane + 64 k < dp` lanes.  n = 33 (a full wave and a one-row wave) and 129 (a
              full workgroup and a one-row one).  d = 68, 132, 228 again without b_cos.
  row counts  n = 63 .. 256 around the wave (32) and workgroup (128) edges at d = 36 (padded columns inside a
              register-resident X) and d = 132 (X re-read from memory per tile).
  splits      d = 8; n = 1025 (33 tiles, 2 per split, trailing splits without a tile: (-inf, 0, 0) partials), n = 2016
              (63 tiles, the last live split holds one), n = 2049 (65 tiles, 3 per split, empty splits).  The structure is
              restated from crh_infonce_splits and asserted first.
  n_dev       n_max = 300 (3 workgroups, 10 splits of one tile), rows1 != rows2, tables pre-filled with 3.0, the device
              count n = -3 .. 305: read_n's clamps, idle trailing workgroups, untouched rows.
  peaked      batches with P_ii within 1e-7 .. 1e-3 of 1 (and one whose diagonal lies > 100 binades under the row maximum:
              the row finish's p_ii <= 1e-30 branch), judged row by row: see test_peaked_and_mixed_batches_row_by_row.
  zero rows   exact-zero rows in v1, in v2, in both, at rows 0, 31, 32, 69 of 70; a row of norm 1e-20 (sum of squares
              subnormal or zero in fp32), one of norm 1e-11 (just above F.normalize's clamp).
  workspace   one oversized workspace of 0xFF bytes reused over shrinking n_max in the trainer's call shape.
  fuzzer      tests/fuzz/fuzz_loss_ops.py --only infonce in a child process.
"""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from coldrec_amd import _lib, ops
from tests import infonce_restate
from tests.test_infonce_gpu import formula_grads, views

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def check_against_restatement(v1, v2, tau, b_cos, loss, g1, g2, label):
    """check_against_fp64's bars with the float64 restatement as the reference; no absolute floor on the loss."""
    _, l64, a64, b64 = infonce_restate.infonce(v1, v2, tau, b_cos)
    _, a32, b32 = formula_grads(v1, v2, tau, b_cos, torch.float32)
    l64 = float(l64)
    assert abs(float(loss) - l64) <= 1e-5 * abs(l64), (label, float(loss), l64)
    for got, ref, t32 in ((g1, a64, a32), (g2, b64, b32)):
        assert torch.isfinite(got).all(), label
        big = ref.abs().max().item()
        err = (got.double().cpu() - ref).abs().max().item()
        err32 = (t32.double().cpu() - ref).abs().max().item()
        assert err <= 1e-4 * big + 1e-30, (label, err, big)
        assert err <= 2 * err32 + 1e-6 * big, (label, err, err32, big)


# ======================================================================================= a. every instantiation
WIDTHS = [4, 32, 36, 64, 68, 96, 100, 128, 132, 160, 164, 192, 196, 224, 228, 256]


@pytest.mark.parametrize("n", [33, 129])
@pytest.mark.parametrize("d", WIDTHS)
def test_every_width_instantiation_both_passes(n, d):
    v1, v2 = views(n, d, seed=40000 + n * 300 + d)
    loss, g1, g2 = ops.infonce(v1, v2, 0.2, True)
    check_against_restatement(v1, v2, 0.2, True, loss.item(), g1, g2, (n, d))


@pytest.mark.parametrize("n", [33, 129])
@pytest.mark.parametrize("d", [68, 132, 228])
def test_widths_on_raw_dot_products(n, d):
    v1, v2 = views(n, d, seed=50000 + n * 300 + d, scale=1.0 / np.sqrt(d))
    loss, g1, g2 = ops.infonce(v1, v2, 1.0, False)
    check_against_restatement(v1, v2, 1.0, False, loss.item(), g1, g2, (n, d, "raw"))


# ======================================================================================= b. row-count edges
@pytest.mark.parametrize("n", [63, 64, 65, 96, 97, 127, 128, 160, 161, 255, 256])
@pytest.mark.parametrize("d", [36, 132])
def test_row_counts_at_wave_and_workgroup_edges(n, d):
    v1, v2 = views(n, d, seed=60000 + n * 300 + d)
    loss, g1, g2 = ops.infonce(v1, v2, 0.2, True)
    check_against_restatement(v1, v2, 0.2, True, loss.item(), g1, g2, (n, d))


# ======================================================================================= c. split structure
def split_structure(n_max):
    """(tiles, splits, tiles per split, splits that hold a tile, tiles of the last of them): nce_pass_kernel's
    `per = ceil(tiles_all / splits)`, `t_begin = cs * per`, restated from crh_infonce_splits."""
    splits = _lib.lib().crh_infonce_splits(n_max)
    tiles = (n_max + 31) // 32
    per = -(-tiles // splits)
    live = -(-tiles // per)
    return tiles, splits, per, live, tiles - (live - 1) * per


@pytest.mark.parametrize("n,tiles,per,shape", [(1025, 33, 2, "empty"), (2016, 63, 2, "one-tile"), (2049, 65, 3, "empty")])
def test_column_splits_with_no_tile_and_with_one(n, tiles, per, shape):
    got = split_structure(n)
    why = f"crh_infonce_splits changed: n = {n} no longer has the split structure this case is here for: {got}"
    assert got[0] == tiles and got[2] == per, why
    if shape == "empty":
        assert got[3] < got[1], why                      # trailing splits without a tile
    else:
        assert got[3] == got[1] and got[4] == 1 and per > 1, why   # the last split holds one tile, the others more
    v1, v2 = views(n, 8, seed=70000 + n)
    loss, g1, g2 = ops.infonce(v1, v2, 0.2, True)
    check_against_restatement(v1, v2, 0.2, True, loss.item(), g1, g2, (n, 8))


# ======================================================================================= d. the device count
N_MAX = 300
_NDEV = {}


def ndev_setup(d):
    """Tables, row ids (permutations into larger tables, rows1 != rows2) and the n = 300 outputs, computed once per d."""
    if d not in _NDEV:
        g = torch.Generator(device=DEV).manual_seed(800 + d)
        T1 = (torch.randn(500, d, device=DEV, generator=g) * 0.3).contiguous()
        T2 = (T1[:400] + torch.randn(400, d, device=DEV, generator=g) * 0.2).contiguous()
        r1 = torch.randperm(500, device=DEV, generator=g)[:N_MAX].int()
        r2 = torch.randperm(400, device=DEV, generator=g)[:N_MAX].int()
        assert not torch.equal(r1, r2)
        _NDEV[d] = (T1, T2, r1, r2, ndev_call(T1, T2, r1, r2, N_MAX))
    return _NDEV[d]


def ndev_call(T1, T2, r1, r2, n):
    G1 = torch.full_like(T1, 3.0)
    G2 = torch.full_like(T2, 3.0)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    loss, _, _ = ops.infonce(T1, T2, 0.2, True, rows1=r1, rows2=r2, n_dev=n_dev, n_max=N_MAX, grad1=G1, grad2=G2)
    return loss.clone(), G1, G2


@pytest.mark.parametrize("n", [-3, 0, 1, 31, 32, 33, 100, 299, 300, 305])
@pytest.mark.parametrize("d", [36, 132])
def test_device_count_clamps_idle_workgroups_and_untouched_rows(n, d):
    T1, T2, r1, r2, full = ndev_setup(d)
    loss, G1, G2 = ndev_call(T1, T2, r1, r2, n)
    live = min(max(n, 0), N_MAX)
    for G, r in ((G1, r1), (G2, r2)):
        rest = torch.ones(G.shape[0], dtype=torch.bool, device=DEV)
        rest[r[:live].long()] = False
        assert (G[rest] == 3.0).all(), (n, d)
    if n <= 0:
        assert loss.item() == 0.0
    elif n == 1:
        assert loss.item() == 0.0
        assert (G1[r1[0].long()] == 0).all() and (G2[r2[0].long()] == 0).all()
    elif n >= N_MAX:
        assert all(torch.equal(x, y) for x, y in zip((loss, G1, G2), full)), (n, d)
    if n > 1:
        a, b = r1[:live].long(), r2[:live].long()
        check_against_restatement(T1[a], T2[b], 0.2, True, loss.item(), G1[a], G2[b], ("n_dev", n, d))


# ======================================================================================= e. peaked batches, row by row
def test_peaked_and_mixed_batches_row_by_row():
    """infonce.hip's promise that "the gradients carry the relative error of torch's (P - I) Z products even where P is
    peaked", which a bar over the whole matrix cannot see (a row with P_ii ~ 1 has a gradient millions of times smaller
    than a flat row's).  Per gradient rho = max over rows of max|got_row - ref_row| / max|ref_row|; the kernel's rho must
    be <= max(8 x the float32 restatement's on the same case, 1e-4) and its loss within max(8 x the float32 restatement's,
    1e-5) relative, with no absolute floor (the all-peaked losses are 4e-7 and 1e-5).  tests/test_infonce.py shows on the
    CPU that the float32 restatement is within 1e-4 / 8 on every case and plain float32 autograd is off by 6e-3 .. 1.3e-1.

    Measured on the MI355X, rho of g1, g2 and the loss's relative error, kernel | float32 restatement:
        mixed-256x64    9.4e-6  2.1e-6  3.7e-8  |  7.0e-6  2.7e-6  3.7e-8
        mixed-130x132   7.1e-6  1.2e-6  7.9e-8  |  6.7e-6  1.6e-6  5.1e-9
        peaked-256x64   8.8e-6  7.9e-6  1.6e-7  |  8.3e-6  7.4e-6  4.9e-7
        peaked-64x32    5.9e-6  4.4e-6  3.9e-7  |  4.4e-6  4.5e-6  6.5e-7
        anti-64x32      5.3e-6  7.0e-6  5.1e-8  |  3.7e-6  5.0e-6  1.5e-8
    (every bar is therefore its fixed part, 1e-4 and 1e-5).  With the column pass's expm1f(e * LN2) written as
    exp2f(e) - 1.f the all-peaked cases give rho(g2) = 5.0e-2 and 1.5e-3; with the diagonal back in the row pass's sum and
    logf(l / p_ii) in the finish rho(g1) = 1.5, 1.1, 2.1, 1.3e-1 on the four cases with peaked rows and the all-peaked
    losses are off by 1.4e-1 and 3.2e-3."""
    cases = infonce_restate.peaked_cases()
    assert (infonce_restate.diag_binades_under_max(*cases["anti-64x32"][:3]) > 100).any()   # p_ii <= 1e-30 in a row finish
    bad = []
    for name, (v1, v2, tau, _) in cases.items():
        _, l64, a64, b64 = infonce_restate.infonce(v1, v2, tau)
        _, l32, a32, b32 = infonce_restate.infonce(v1, v2, tau, dtype=torch.float32)
        loss, g1, g2 = ops.infonce(v1.to(DEV), v2.to(DEV), tau, True)
        assert torch.isfinite(loss).all() and torch.isfinite(g1).all() and torch.isfinite(g2).all(), name
        l64 = float(l64)
        rel, rel32 = abs(loss.item() - l64) / abs(l64), abs(float(l32) - l64) / abs(l64)
        rho = [infonce_restate.row_rho(g.cpu(), r) for g, r in ((g1, a64), (g2, b64))]
        rho32 = [infonce_restate.row_rho(g, r) for g, r in ((a32, a64), (b32, b64))]
        print(f"{name}: kernel rho {rho[0]:.2e} {rho[1]:.2e} loss {rel:.2e} | float32 restatement rho {rho32[0]:.2e} "
              f"{rho32[1]:.2e} loss {rel32:.2e}")
        if not (rel <= max(8 * rel32, 1e-5) and all(k <= max(8 * r, 1e-4) for k, r in zip(rho, rho32))):
            bad.append((name, rho, rho32, rel, rel32))
    assert not bad, bad


# ======================================================================================= f. zero-norm and below-clamp rows
def assert_row_groups_close(got, ref, groups, rel, label):
    """assert_rows_close's split (error <= rel x max|ref| over the clamped rows and over the others, each on its own), with
    the rows just above the clamp as a third group: their gradient is ~1e9, between the clamped rows' 1e10 and up and the
    other rows' 1e-2."""
    for k, sel in enumerate(groups):
        if sel.any():
            err = np.abs(got[sel] - ref[sel]).max()
            assert err <= rel * np.abs(ref[sel]).max() + 1e-30, (label, k, err)


@pytest.mark.parametrize("where", ["v1", "v2", "both"])
def test_zero_norm_and_below_clamp_rows(where):
    n, d = 70, 36
    v1, v2 = views(n, d, seed=900)
    for v in ((v1,) if where == "v1" else (v2,) if where == "v2" else (v1, v2)):
        v[[0, 31, 32, 69]] = 0.0
    v1[5] *= 1e-20 / v1[5].norm()
    v2[40] *= 1e-20 / v2[40].norm()
    v1[10] *= 1e-11 / v1[10].norm()
    v2[50] *= 1e-11 / v2[50].norm()
    assert float((v1[5].double() ** 2).sum()) < 1.2e-38                         # under fp32's normal range
    loss, g1, g2 = ops.infonce(v1, v2, 0.2, True)
    assert torch.isfinite(loss).all() and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    _, l64, a64, b64 = infonce_restate.infonce(v1, v2, 0.2, True)
    assert abs(loss.item() - float(l64)) <= 1e-5 * abs(float(l64))
    for v, got, ref in ((v1, g1, a64), (v2, g2, b64)):
        nr = v.double().norm(dim=1).cpu().numpy()
        clamped, near = nr < 1e-12, (nr >= 1e-12) & (nr < 1e-6)
        zeros = 4 if where in ("both", "v1" if v is v1 else "v2") else 0
        assert clamped.sum() == zeros + 1 and near.sum() == 1
        assert_row_groups_close(got.double().cpu().numpy(), ref.numpy(), (clamped, near, ~(clamped | near)), 1e-4, where)


# ======================================================================================= g. dirty, oversized workspace
@pytest.mark.parametrize("short", [0, 7])
def test_a_dirty_oversized_workspace_changes_no_bit(short):
    """train.py's _nce keeps one workspace sized for the largest batch so far and lays smaller layouts over its stale
    bytes.  One workspace of infonce_workspace(1000, 132), every byte 0xFF (NaNs), the trainer's call shape (rows1 = rows2,
    scale 0.1, accumulate, a caller's loss slot; separate gradient tables as XSimGCL has them and one shared table as
    SimGCL has), n_max = 1000, 257, 33, 1 without re-poisoning and then each once more freshly poisoned; ``short``: the
    same with n_dev = n_max - 7 (n_max = 1: a count below zero).  Every output is bit-equal to the same call on a fresh
    zero-filled workspace of exactly infonce_workspace_bytes(n_max, 132)."""
    d, sizes = 132, (1000, 257, 33, 1)
    g = torch.Generator(device=DEV).manual_seed(77)
    T1 = (torch.randn(1200, d, device=DEV, generator=g) * 0.3).contiguous()
    T2 = (T1 + torch.randn(1200, d, device=DEV, generator=g) * 0.2).contiguous()
    rows = torch.randperm(1200, device=DEV, generator=g)[:1000].int()
    pre1 = torch.randn(1200, d, device=DEV, generator=g)
    pre2 = torch.randn(1200, d, device=DEV, generator=g)

    def call(n_max, ws, shared):
        G1 = pre1.clone()
        G2 = G1 if shared else pre2.clone()
        loss = torch.full((4,), -7.0, device=DEV)
        n_dev = torch.tensor([n_max - short], dtype=torch.int32, device=DEV) if short else None
        ops.infonce(T1, T2, 0.2, True, rows1=rows[:n_max].contiguous(), rows2=rows[:n_max].contiguous(), n_dev=n_dev,
                    n_max=n_max, scale=0.1, accumulate=True, grad1=G1, grad2=G2, loss=loss[2:3], workspace=ws)
        return loss, G1, G2

    for shared in (False, True):
        want = {}
        for n_max in sizes:
            fresh = torch.zeros(ops.infonce_workspace_bytes(n_max, d), dtype=torch.uint8, device=DEV)
            want[n_max] = call(n_max, fresh, shared)
            assert all(torch.isfinite(t).all() for t in want[n_max])
            assert not torch.equal(want[n_max][1], pre1) or n_max - short <= 1       # the call did write gradients
        dirty = ops.infonce_workspace(1000, d, DEV)
        dirty.fill_(255)
        for n_max in sizes:                                # shrinking layouts over whatever the larger ones left
            got = call(n_max, dirty, shared)
            assert all(torch.equal(x, y) for x, y in zip(got, want[n_max])), ("stale", n_max, shared)
        for n_max in sizes:
            dirty.fill_(255)
            got = call(n_max, dirty, shared)
            assert all(torch.equal(x, y) for x, y in zip(got, want[n_max])), ("poisoned", n_max, shared)


# ======================================================================================================== fuzzer
FUZZ_CASES, FUZZ_SEED = 60, 2026


def test_infonce_fuzzer_short_run():
    """tests/fuzz/fuzz_loss_ops.py --only infonce --cases 60 --seed 2026 in a child process.
    Measured on the MI355X: 3.4 s for the whole child, the interpreter's start and the library's load included."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_loss_ops.py"), "--only", "infonce", "--cases",
           str(FUZZ_CASES), "--seed", str(FUZZ_SEED)]
    t0 = time.time()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    print(f"fuzzer: {time.time() - t0:.1f} s; {out.stdout.strip().splitlines()[-1:]}")
    assert out.returncode == 0 and "fuzz ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
