"""GPU: the fused NGCF layer (csrc/ngcf.hip) where its slabs, tiles and partial sums change -- the shapes its own test file
(tests/test_ngcf_gpu.py) never reaches -- against the same float64 restatement (tests/ngcf_restate.py), with that file's
helpers (_inputs, _check, _dist, _fwd_torch32, _bwd_torch32, C) and its rule unchanged.  No case is skipped.

Geometry.  ``geometry(N, d)`` restates the kernel's launch arithmetic (32-row tiles, ``tpw`` tiles per wave so that at most
2048 waves = partials exist, chunks of 32 partials, NgcfCut's slabs per DP = ceil32(d)).  Every case asserts the figures it
claims to reach AND that ``ops.ngcf_workspace_bytes`` equals round256(4 parts pe) + round256(4 chunks pe): a change of
NGCF_MAX_PARTS or NGCF_CHUNK fails here instead of moving the cases off their edges.

What each group reaches:
  widths   N = 65 (three tiles, the last of one row) at d = 36 | 68, 96 | 132, 160 | 164, 192 | 196, 224 | 228: both ends of
           DP = 96 (CS = 3, the only three-slab cut), 160 (NT = 5, CS = 10), 192 (CS = 12) and 224 (NT = 7, CS = 14), the low
           ends of 64 and 256.  DP 96, 160, 192, 224 are launched by nothing else; 160 and 224 are the odd tile counts, the
           only ones where OS * OT > NT and `if (og >= NT) continue;` is taken (phase W's loop and the write-out).
  chunks   N = 1024, 1025, 2048, 2049 -> 32, 33, 64, 65 partials -> 1, 2, 2, 3 chunks, the last chunk holding one partial
           twice: ngcf_chunk_sum_kernel's blockIdx.y > 0 and its `hi > n_in` clamp, ngcf_final_sum_kernel over n_in > 1.
           d = 12 (one kernel, idle lanes in the only column tile) and d = 132 (slab launch, odd tile count).
  tpw      the 2048-partial cap times 32 rows fixes these N: (65 536, 4) tpw 1 at the cap, 2048 partials, 64 full chunks;
           (65 537, 64) tpw 2, 1025 partials, 33 chunks, a last wave of one tile of one row, weights in LDS; (131 073, 4) tpw 3,
           1366 partials, 43 chunks, a last wave with 2 of its 3 tiles; (65 537, 132) tpw 2 under the slab launch and the
           odd skip (211 MB of workspace).  The tile loop's second trip, its `t_end > n_tiles` clamp, wacc / dbs carried over
           tiles and the early return of waves past the end, forward and all three backward modes.
  exact    (2049, 132), (65 537, 64), (131 073, 4) with small integers and c = 0.5: every product and partial sum is an
           integer or half-integer below 2^23, float32 is exact in any order, and ds, local, dw, db must EQUAL the int64
           result (torch.equal), with g and as the top layer.
  engine   one NGCFEngine.step at d = 96 (MODE 1 then MODE 2, local over g, the next SpMM reading it) on 700 x 900 = 1600
           rows (50 partials, 2 chunks), L = 2, B = 512: the assertions of the d = 64 engine test.
  fuzzer   tests/fuzz/fuzz_ngcf.py, 60 cases at a fixed seed, as a child process.

Bars.  tests/test_ngcf_gpu.py's rule through its ``_check``: every output's largest error over the float64 value's largest
magnitude, within 8x the same distance of the float32 torch formula on the same device at the same shape.  No bar is taken
from what the kernel produced.

Measured on the MI355X.  No case comes near the bar, so no host model of the sum tree was needed: the kernel's worst ratio
to the torch formula's own distance is 2.69 over the layer cases (N65-d228 bwd, db: 1.3e-7 against 4.9e-8) and 1.31 in the
engine step at d = 96; its largest distance is 8.9e-7 (x_k, N65-d192 without bias; torch 4.4e-7).  At the large N the kernel's
fixed tree is the closer one: dw lies 1.1e-7 .. 4.9e-7 from float64 where torch's GEMM lies 2.2e-6 .. 5.0e-6.  The exact cases
are equal bit for bit.  The fuzzer found the one defect: the forward began its accumulators at the bias, so each of the 2 d
fma steps rounded at the bias's magnitude -- x_k 1.49e-6 against torch's 1.59e-7 at N = 1042, d = 256 with x and s of size
0.05 (ratio 9.4).  csrc/ngcf.hip now adds the bias to the finished sum; that case and the other 59 pass.  Wall time: the
fuzzer's child 5.1 s; the slowest other test 1.1 s (test_tiles_per_wave_backward[N65537-d132]); the file 12 s.
"""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from tests import ngcf_restate as R
from tests import test_ngcf_gpu as ng
from tests.test_ngcf_gpu import C, _bwd_torch32, _check, _dist, _fwd_torch32, _guarded, _inputs, _intact  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ_CASES, FUZZ_SEED = 60, 2027


def _cdiv(a, b):
    return -(-a // b)


def _round256(nbytes):
    return (nbytes + 255) // 256 * 256


def geometry(n, d):
    """csrc/ngcf.hip's launch arithmetic, restated: ngcf_tiles, ngcf_tpw, ngcf_parts, NGCF_CHUNK = 32, NgcfCut<DP>,
    ngcf_part_floats and ngcf_layout's two 256-byte-rounded pieces."""
    tiles = _cdiv(n, 32)
    tpw = max(1, _cdiv(tiles, 2048))
    parts = _cdiv(tiles, tpw)
    chunks = _cdiv(parts, 32)
    dp = _cdiv(d, 32) * 32
    nt = dp // 32
    tb = nt if dp <= 64 else 1
    os_ = 1 if dp <= 128 else 2
    ot = _cdiv(nt, os_)
    pe = 2 * dp * dp + dp
    return dict(tiles=tiles, tpw=tpw, parts=parts, chunks=chunks, last_wave_tiles=tiles - (parts - 1) * tpw,
                last_chunk_parts=parts - (chunks - 1) * 32, DP=dp, NT=nt, TB=tb, OS=os_, OT=ot, CS=(nt // tb) * os_,
                odd_skip=os_ * ot > nt, pe=pe, ws=_round256(4 * parts * pe) + _round256(4 * chunks * pe))


def _reaches(n, d, **claims):
    """The case is where it says it is, and the library lays its workspace out as the restated geometry does."""
    from coldrec_amd import ops
    geo = geometry(n, d)
    for k, v in claims.items():
        assert geo[k] == v, (n, d, k, geo[k], v)
    assert ops.ngcf_workspace_bytes(n, d) == geo["ws"], (n, d, ops.ngcf_workspace_bytes(n, d), geo)
    return geo


def _case(n, d, tpw, parts, chunks, last_wave_tiles, cs, odd_skip, **more):
    return pytest.param(n, d, dict(tpw=tpw, parts=parts, chunks=chunks, last_wave_tiles=last_wave_tiles, CS=cs,
                                   odd_skip=odd_skip, **more), id="N%d-d%d" % (n, d))


#            N    d  tpw parts chunks last-wave CS  OS*OT>NT
WIDTHS = [_case(65, 36, 1, 3, 1, 1, 1, False, DP=64),
          _case(65, 68, 1, 3, 1, 1, 3, False, DP=96, OT=3, OS=1), _case(65, 96, 1, 3, 1, 1, 3, False, DP=96),
          _case(65, 132, 1, 3, 1, 1, 10, True, DP=160, NT=5, OS=2, OT=3), _case(65, 160, 1, 3, 1, 1, 10, True, DP=160),
          _case(65, 164, 1, 3, 1, 1, 12, False, DP=192), _case(65, 192, 1, 3, 1, 1, 12, False, DP=192),
          _case(65, 196, 1, 3, 1, 1, 14, True, DP=224, NT=7, OT=4), _case(65, 224, 1, 3, 1, 1, 14, True, DP=224),
          _case(65, 228, 1, 3, 1, 1, 16, False, DP=256)]
CHUNKS = [_case(1024, 12, 1, 32, 1, 1, 1, False, last_chunk_parts=32), _case(1025, 12, 1, 33, 2, 1, 1, False, last_chunk_parts=1),
          _case(2048, 12, 1, 64, 2, 1, 1, False, last_chunk_parts=32), _case(2049, 12, 1, 65, 3, 1, 1, False, last_chunk_parts=1),
          _case(1024, 132, 1, 32, 1, 1, 10, True, last_chunk_parts=32), _case(1025, 132, 1, 33, 2, 1, 10, True, last_chunk_parts=1),
          _case(2048, 132, 1, 64, 2, 1, 10, True, last_chunk_parts=32), _case(2049, 132, 1, 65, 3, 1, 10, True, last_chunk_parts=1)]
TPW = [_case(65536, 4, 1, 2048, 64, 1, 1, False, tiles=2048, last_chunk_parts=32),
       _case(65537, 64, 2, 1025, 33, 1, 1, False, tiles=2049, last_chunk_parts=1),
       _case(131073, 4, 3, 1366, 43, 2, 1, False, tiles=4097),
       _case(65537, 132, 2, 1025, 33, 1, 10, True, tiles=2049, last_chunk_parts=1)]


def _forward(n, d, forms):
    """The forms of tests/test_ngcf_gpu.py's test_layer_forward_matches_float64_restatement.  A: y and acc_in given, both
    scales off 1, acc_out its own buffer; B: no y, no acc_in; C: y alone, no bias, then acc_out over acc_in against A."""
    from coldrec_amd import ops
    tag = "N%d-d%d" % (n, d)
    inp = _inputs(n, d)
    x, s, w, b, acc = (inp[k].to(DEV) for k in ("x", "s", "w", "b", "acc"))
    x64, s64, w64, b64, acc64 = (R.f64(inp[k]) for k in ("x", "s", "w", "b", "acc"))
    xk64 = R.layer_fwd(x64, s64, w64[:d], b64[0], w64[d:], b64[1])
    worst = 0.0
    y, out = torch.empty_like(x), torch.empty_like(x)
    ops.ngcf_layer_fwd(x, s, w, b, y=y, acc_in=acc, s_in=0.75, acc_out=out, s_out=0.5)
    t_xk, t_out = _fwd_torch32(x, s, w, b, acc, 0.75, 0.5)
    worst = max(worst, _check(tag + " fwd", ("x_k", "acc_out"), (y, out), (t_xk, t_out), (xk64, (acc64 * 0.75 + xk64) * 0.5)))
    if "B" in forms:
        y2, out2 = ops.ngcf_layer_fwd(x, s, w, b, acc_out=torch.empty_like(x), s_out=C, want_y=False)
        assert y2 is None
        worst = max(worst, _check(tag + " fwd, no y, no acc_in", ("acc_out",), (out2,),
                                  (_fwd_torch32(x, s, w, b, None, 1.0, C)[1],), (xk64 * C,)))
    if "C" in forms:
        y3, none = ops.ngcf_layer_fwd(x, s, w)
        assert none is None
        nb = R.layer_fwd(x64, s64, w64[:d], 0.0, w64[d:], 0.0)
        worst = max(worst, _check(tag + " fwd, y alone, no bias", ("x_k",), (y3,),
                                  (_fwd_torch32(x, s, w, b * 0, None, 1.0, 1.0)[0],), (nb,)))
        acc_io = acc.clone()
        ops.ngcf_layer_fwd(x, s, w, b, acc_in=acc_io, s_in=0.75, acc_out=acc_io, s_out=0.5, want_y=False)
        assert torch.equal(acc_io, out)
    return worst


def _backward(n, d):
    """tests/test_ngcf_gpu.py's test_layer_backward_matches_float64_restatement, with g and as the top layer."""
    from coldrec_amd import ops
    inp = _inputs(n, d, seed=1)
    x64, s64, w64, b64 = (R.f64(inp[k]) for k in ("x", "s", "w", "b"))
    xk32 = torch.from_numpy(R.layer_fwd(x64, s64, w64[:d], b64[0], w64[d:], b64[1])).float()        # the signs all three use
    assert (xk32 > 0).any() and (xk32 < 0).any()
    x, s, w, g, dout = (inp[k].to(DEV) for k in ("x", "s", "w", "g", "dout"))
    xk = xk32.to(DEV)
    worst = 0.0
    for top in (False, True):
        g_dev, g64 = (None, None) if top else (g, R.f64(inp["g"]))
        ds, local, dw, db = ops.ngcf_layer_bwd(x, s, xk, g_dev, dout, C, w)
        want = R.layer_bwd(x64, s64, R.f64(xk32), g64, R.f64(inp["dout"]), C, w64[:d], w64[d:])
        want = (want[0], want[1], np.concatenate([want[2], want[3]]), want[4])
        worst = max(worst, _check("N%d-d%d" % (n, d) + (" bwd top" if top else " bwd"), ("ds", "local", "dw", "db"),
                                  (ds, local, dw, db), _bwd_torch32(x, s, xk, g_dev, dout, C, w), want))
    return worst


@pytest.mark.parametrize("n, d, claims", WIDTHS)
def test_widths_forward(n, d, claims):
    _reaches(n, d, **claims)
    _forward(n, d, "ABC")


@pytest.mark.parametrize("n, d, claims", WIDTHS)
def test_widths_backward(n, d, claims):
    _reaches(n, d, **claims)
    _backward(n, d)


@pytest.mark.parametrize("n, d, claims", CHUNKS)
def test_chunks_backward_and_one_forward(n, d, claims):
    """The backward is the point (the two reduction kernels); the forward runs once, in form A."""
    _reaches(n, d, **claims)
    _backward(n, d)
    _forward(n, d, "A")


@pytest.mark.parametrize("n, d, claims", TPW)
def test_tiles_per_wave_forward(n, d, claims):
    t0 = time.time()
    _reaches(n, d, **claims)
    _forward(n, d, "ABC")
    print(f"N{n}-d{d} forward: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("n, d, claims", TPW)
def test_tiles_per_wave_backward(n, d, claims):
    t0 = time.time()
    _reaches(n, d, **claims)
    _backward(n, d)
    print(f"N{n}-d{d} backward: {time.time() - t0:.1f} s")


# ---- exact arithmetic ---------------------------------------------------------------------------------------------------

EXACT = [_case(2049, 132, 1, 65, 3, 1, 10, True), _case(65537, 64, 2, 1025, 33, 1, 1, False),
         _case(131073, 4, 3, 1366, 43, 2, 1, False)]


def _int_matmul(a, b):
    """a @ b of int64 matrices as int64.  NumPy's integer matmul takes seconds at N = 65 537, so the products run in float64
    (every entry and partial sum is an integer far below 2^53: exact in any order) and are cast back, the cast checked; at
    the small shape the plain int64 product is checked against it as well."""
    f = np.ascontiguousarray(a, np.float64) @ np.ascontiguousarray(b, np.float64)
    r = f.astype(np.int64)
    assert (r == f).all() and np.abs(f).max() < 2 ** 40
    if a.size <= 2049 * 132:
        assert (r == a @ b).all()
    return r


@pytest.mark.parametrize("n, d, claims", EXACT)
def test_small_integers_come_out_exact_bit_for_bit(n, d, claims):
    """x in {-1, 0, 1}; s and both halves of w in {-2 .. 2}; g, dout in {-1, 0, 1}; c = 0.5; x_k > 0 everywhere (slope 1).
    Every product and every partial sum is an integer or a half-integer of magnitude at most 2 N = 262 146 < 2^23, so every
    float32 sum is exact in any order and the kernel must return the int64 result.  The int64 arithmetic runs on doubled
    values (2 dz = 2 g, or dout for the top layer, since 2 c = 1); halving a value below 2^24 is exact in float32."""
    from coldrec_amd import ops
    _reaches(n, d, **claims)
    rng = np.random.default_rng(4100 + n + d)
    x, g, dout = (rng.integers(-1, 2, (n, d)) for _ in range(3))
    s, w = rng.integers(-2, 3, (n, d)), rng.integers(-2, 3, (2 * d, d))
    xk = rng.integers(1, 4, (n, d))
    dev = lambda a: torch.from_numpy(a.astype(np.float32)).to(DEV)
    xd, sd, wd, gd, dd, xkd = (dev(a) for a in (x, s, w, g, dout, xk))
    for top in (False, True):
        dz2 = dout if top else 2 * g                                   # int64: twice dz
        t2 = _int_matmul(dz2, w[d:])
        want2 = (_int_matmul(dz2, w[:d]) + x * t2, dout + s * t2,
                 np.concatenate([_int_matmul(dz2.T, s), _int_matmul(dz2.T, x * s)]), dz2.sum(0))
        for name, a in zip(("ds", "local", "dw", "db"), want2):
            assert a.dtype == np.int64 and 0 < np.abs(a).max() <= 4 * n < 2 ** 24, (name, np.abs(a).max())
        got = ops.ngcf_layer_bwd(xd, sd, xkd, None if top else gd, dd, 0.5, wd)
        for name, f, a in zip(("ds", "local", "dw", "db"), got, want2):
            want = torch.from_numpy((a.astype(np.float64) / 2).astype(np.float32))
            assert (want.double().numpy() * 2 == a).all(), name        # the reference is what float32 holds
            f = f.cpu()
            bad = (f != want).nonzero()
            assert torch.equal(f, want), (name, "top" if top else "g", int(bad.shape[0]), bad[:4].tolist())


# ---- contracts at a shape with slabs and several chunks: tests/test_ngcf_gpu.py's parametrisations -----------------------
# (2049, 132) is added there, to test_nothing_is_written_outside_the_outputs_and_the_workspace,
# test_permitted_aliasing_gives_the_same_bits and test_two_identical_backward_calls_give_identical_bits.

def test_the_contract_tests_run_at_the_slab_and_chunk_shape():
    """The three contract tests of tests/test_ngcf_gpu.py carry (2049, 132): 65 partials, 3 chunks, CS = 10, the odd skip."""
    _reaches(2049, 132, parts=65, chunks=3, CS=10, odd_skip=True)
    for fn in (ng.test_nothing_is_written_outside_the_outputs_and_the_workspace, ng.test_permitted_aliasing_gives_the_same_bits,
               ng.test_two_identical_backward_calls_give_identical_bits):
        pairs = [m.args[1] for m in fn.pytestmark if m.name == "parametrize"]
        assert pairs and (2049, 132) in pairs[0], fn.__name__


# ---- one engine step in the two-launch form, over more than one chunk -------------------------------------------------------

@functools.lru_cache(maxsize=1)
def _builder_700_900():
    from coldrec_amd.data.synth import make_interactions, split_cold
    from coldrec_amd.util.databuilder import ColdStartDataBuilder
    split = split_cold(make_interactions(700, 900, 9000), "item")
    info = split.info
    return ColdStartDataBuilder(split.warm_train, split.warm_val, split.cold_val, split.overall_val, split.warm_test,
                                split.cold_test, split.overall_test, info["user_num"], info["item_num"], info["warm_user"],
                                info["warm_item"], info["cold_user"], info["cold_item"], None, split.content)


def test_one_engine_step_in_the_two_launch_form_over_two_chunks():
    """tests/test_ngcf_gpu.py's engine test at d = 96 (CS = 3: MODE 1, then MODE 2 with local over the g buffer, which the
    next SpMM reads) on 700 + 900 = 1600 rows (50 partials, 2 chunks)."""
    from coldrec_amd import ops
    from tests.test_ngcf import torch_step
    data = _builder_700_900()
    U, I, d, L, B, reg = data.user_num, data.item_num, 96, 2, 512, 1e-4
    assert (U, I) == (700, 900)
    _reaches(U + I, d, tpw=1, parts=50, chunks=2, last_chunk_parts=18, CS=3, odd_skip=False)
    g = torch.Generator().manual_seed(79)
    init = dict(u=torch.randn(U, d, generator=g) * 0.1, v=torch.randn(I, d, generator=g) * 0.1,
                w=[tuple(torch.randn(sh, generator=g) * sc for sh, sc in (((d, d), 0.1), ((d,), 0.05), ((d, d), 0.1), ((d,), 0.05)))
                   for _ in range(L)])
    users = torch.randint(U, (B,), generator=g, dtype=torch.int32)
    pos = torch.randint(I, (B,), generator=g, dtype=torch.int32)
    neg = torch.randint(I, (B,), generator=g, dtype=torch.int32)
    u_d, p_d, n_d = users.to(DEV), pos.to(DEV), neg.to(DEV)
    plan = ops.build_plans_device(u_d, p_d, n_d, B)[0]
    runs = []
    for _ in range(2):
        eng = ng._engine(data, init, L)
        eng.step(u_d, p_d, n_d, plan)
        torch.cuda.synchronize()
        runs.append(eng)
    a, b = runs
    assert torch.equal(a.G, b.G) and torch.equal(a.E, b.E) and torch.equal(a.loss, b.loss)
    for k in range(L):
        assert torch.equal(a.dWst[k], b.dWst[k]) and torch.equal(a.dbst[k], b.dbst[k])
        assert torch.equal(a.Wst[k], b.Wst[k]) and torch.equal(a.bst[k], b.bst[k])
        assert not torch.equal(a.Wst[k], torch.cat([init["w"][k][0], init["w"][k][2]]).to(DEV))      # the layers moved
    assert not torch.equal(a.E[:U].cpu(), init["u"])
    e0 = torch.cat([init["u"], init["v"]])
    w64 = [tuple(R.f64(t) for t in w) for w in init["w"]]
    (bpr, l2), de0, grads = R.step(R.f64(e0), data.norm_adj.tocsr().astype(np.float64), w64, U, users.numpy(), pos.numpy(),
                                   neg.numpy(), reg)
    adj = torch.from_numpy(data.norm_adj.toarray().astype(np.float32)).to(DEV)
    (t_bpr, t_l2), _, t_de0, t_grads = torch_step(e0.to(DEV), adj, [tuple(t.to(DEV) for t in w) for w in init["w"]], U,
                                                 users.long().to(DEV), pos.long().to(DEV), neg.long().to(DEV), reg)
    loss = a.loss.cpu().numpy()
    print(f"engine step, d = 96: bpr {loss[0]:.7f} (float64 {bpr:.7f}), l2 {loss[1]:.3e} (float64 {l2:.3e})")
    np.testing.assert_allclose(loss, [bpr, l2], rtol=1e-5)
    names, fused, t32, want = ["dE0"], [a.G], [t_de0], [de0]
    for k in range(L):
        for j, (nm, f) in enumerate((("dWgc", a.dWst[k][:d]), ("dbgc", a.dbst[k]), ("dWbi", a.dWst[k][d:]), ("dbbi", a.dbst[k]))):
            names.append(f"{nm}{k}")
            fused.append(f)
            t32.append(t_grads[k][j])
            want.append(grads[k][j])
    _check("engine step, d = 96", names, fused, t32, want)
    for k in range(L):
        assert a.W_gc[k].grad.data_ptr() == a.dWst[k].data_ptr() and a.b_bi[k].grad.data_ptr() == a.dbst[k].data_ptr()


# ---- the fuzzer ---------------------------------------------------------------------------------------------------------

def test_ngcf_fuzzer_short_run():
    """tests/fuzz/fuzz_ngcf.py --cases 60 --seed 2027 in a child process: 60 random (N, d, scales, forms) cases, five of
    them with two tiles per wave at this seed, every DP among them.  Measured on the MI355X: 5.1 s for the whole child."""
    cmd = [sys.executable, os.path.join(ROOT, "tests", "fuzz", "fuzz_ngcf.py"), "--cases", str(FUZZ_CASES), "--seed", str(FUZZ_SEED)]
    t0 = time.time()
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    print(f"fuzzer: {time.time() - t0:.1f} s; {out.stdout.strip().splitlines()[-1:]}")
    assert out.returncode == 0 and "fuzz ok" in out.stdout, (out.returncode, out.stdout[-1500:], out.stderr[-1500:])
