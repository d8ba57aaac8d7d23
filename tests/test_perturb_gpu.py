"""GPU: the layer perturbation of SimGCL / XSimGCL (csrc/perturb.hip: crh_perturb_rows_f32, crh_noise_uniform_f32) against
float64 and against the numpy Philox of tests/cl_restate.py.

Shapes: N in {1, 63, 65, 1000} (one row; one short of / one past a wave's worth of one-lane rows; several blocks) x
d in {4, 12, 64, 100, 128, 256} (lane groups of 1, 3 -> 4, 16, 25 -> 32, 32 and 64 lanes: every group width class, and the
two widths whose groups have idle lanes).

Bound of the buffer mode, per element:  |y_hip - y_f64| <= 2^-23 |y_f64| + eps (d + 8) 2^-24 -- the fp32 norm reduction
(d squares and sums), the square root, the quotient and the two products on a term of size <= eps, plus one rounding of
the sum y + term."""
import numpy as np
import pytest
import torch

from tests import cl_restate

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NS = (1, 63, 65, 1000)
DS = (4, 12, 64, 100, 128, 256)
EPS = 0.1
EPS32 = float(np.float32(EPS))          # what the kernel receives


def _bound(y64, d, eps=EPS32):
    return 2.0 ** -23 * np.abs(y64) + eps * (d + 8) * 2.0 ** -24


def _inputs(n, d, seed):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((n, d)) * 0.2).astype(np.float32)          # both signs
    y[rng.random((n, d)) < 0.1] = 0.0                                     # exact zeros
    y[0, 0] = 0.0
    r = rng.random((n, d)).astype(np.float32)
    r[n // 2] = 0.0                                                       # an all-zero noise row: the normalize clamp
    return y, r


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("d", DS)
def test_buffer_mode_matches_float64(d):
    from coldrec_amd import ops
    for n in NS:
        y, r = _inputs(n, d, 100 * d + n)
        want = cl_restate.perturb_f64(y, r, EPS32)
        yt = _t(y)
        assert ops.perturb_rows(yt, EPS, noise=_t(r)) is yt
        got = yt.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want)
        print(f"n={n} d={d}: worst error / bound = {(err / _bound(want, d)).max():.3f}")
        assert (err <= _bound(want, d)).all()
        assert (got[y == 0.0] == 0.0).all()                               # sign(0) = 0: exact zeros stay zeros
        assert np.array_equal(got[n // 2], y[n // 2])                     # zero noise row: the row is unchanged
        if n > 1:
            assert not np.array_equal(got, y)


@pytest.mark.parametrize("d", DS)
def test_accumulator_semantics(d):
    """acc_out = (acc_in * s_in + y_new) * s_out from the perturbed rows: three fp32 roundings of terms of these sizes."""
    from coldrec_amd import ops
    for n in NS:
        y, r = _inputs(n, d, 7 * d + n)
        acc = np.random.default_rng(n + d).standard_normal((n, d)).astype(np.float32)
        plain = _t(y)
        ops.perturb_rows(plain, EPS, noise=_t(r))                         # acc_out NULL: y alone is written
        y_new = plain.cpu().numpy()

        def check(got, a_in, s_in, s_out):
            s_in32, s_out32 = float(np.float32(s_in)), float(np.float32(s_out))
            a = (a_in.astype(np.float64) * s_in32) if a_in is not None else np.zeros_like(y_new, np.float64)
            want = (a + y_new) * s_out32
            tol = 2.0 ** -24 * ((np.abs(a) + np.abs(a + y_new)) * abs(s_out32) + np.abs(want)) * 1.0001
            assert (np.abs(got.astype(np.float64) - want) <= tol).all()

        # acc_in aliasing acc_out, s_out = 1/3
        yt, at, rt = _t(y), _t(acc), _t(r)
        ops.perturb_rows(yt, EPS, noise=rt, acc_in=at, s_in=1.0, acc_out=at, s_out=1.0 / 3.0)
        assert np.array_equal(yt.cpu().numpy(), y_new)                    # y is the same with and without the accumulator
        check(at.cpu().numpy(), acc, 1.0, 1.0 / 3.0)
        assert np.array_equal(rt.cpu().numpy(), r)                        # the noise buffer is only read
        # separate buffers, s_in = 0.5: acc_in is only read
        yt, at, ot = _t(y), _t(acc), torch.full((n, d), 7.0, device=DEV)
        ops.perturb_rows(yt, EPS, noise=rt, acc_in=at, s_in=0.5, acc_out=ot, s_out=1.0)
        check(ot.cpu().numpy(), acc, 0.5, 1.0)
        assert np.array_equal(at.cpu().numpy(), acc) and np.array_equal(yt.cpu().numpy(), y_new)
        # acc_in NULL = 0
        yt, ot = _t(y), torch.full((n, d), 7.0, device=DEV)
        ops.perturb_rows(yt, EPS, noise=rt, acc_out=ot, s_out=1.0 / 3.0)
        check(ot.cpu().numpy(), None, 1.0, 1.0 / 3.0)


@pytest.mark.parametrize("d", DS)
def test_device_noise_bits(d):
    from coldrec_amd import ops
    for n in NS:
        for seed, draw in ((2024, 0), ((0xABCDEF01 << 32) | 0x12345678, (3 << 32) | 9)):      # both key and counter words
            got = ops.noise_uniform(n, d, seed, draw=draw, device=DEV).cpu().numpy()
            assert np.array_equal(got, cl_restate.philox_uniform(n, d, seed, draw)), (n, d, seed, draw)
        five = torch.tensor([5], dtype=torch.int64, device=DEV)
        a = ops.noise_uniform(n, d, 2024, draw=2, draw_dev=five)
        b = ops.noise_uniform(n, d, 2024, draw=7, device=DEV)
        assert torch.equal(a, b)
        y, _ = _inputs(n, d, d + n)
        acc = np.ones((n, d), np.float32)
        y1, y2, a1, a2 = _t(y), _t(y), _t(acc), _t(acc)
        ops.perturb_rows(y1, EPS, seed=2024, draw=2, draw_dev=five, acc_in=a1, acc_out=a1, s_out=0.5)     # in registers
        ops.perturb_rows(y2, EPS, noise=b, acc_in=a2, acc_out=a2, s_out=0.5)                              # from the buffer
        assert torch.equal(y1, y2) and torch.equal(a1, a2)


@pytest.mark.parametrize("d", DS)
def test_device_noise_properties(d):
    from coldrec_amd import ops
    for n in NS:
        rng = np.random.default_rng(d * 13 + n)
        y = (rng.standard_normal((n, d)) * 0.2).astype(np.float32)
        y[y == 0.0] = 0.25                                                # rows without zeros
        outs = []
        for draw in (0, 1):
            yt = _t(y)
            ops.perturb_rows(yt, EPS, seed=11, draw=draw)
            got = yt.cpu().numpy().astype(np.float64)
            delta = got - y
            assert (delta * np.sign(y) >= 0).all()                        # pushed away from zero, never across
            b = _bound(y.astype(np.float64) + delta, d)
            assert (np.abs(np.linalg.norm(delta, axis=1) - EPS32) <= np.linalg.norm(b, axis=1)).all()
            outs.append(got)
        assert (np.abs(outs[0] - outs[1]).max(axis=1) > 0).all()          # another draw: every row differs


def test_argument_errors_are_reported_without_a_launch():
    from coldrec_amd import _lib
    L = _lib.lib()
    y = torch.ones((8, 264), device=DEV)
    before = y.clone()
    s = torch.cuda.current_stream().cuda_stream
    for d in (6, 260):
        assert L.crh_perturb_rows_f32(y.data_ptr(), 8, d, 0.1, None, 1, None, 0, None, 1.0, None, 1.0, s) == -1
        assert b"multiple of 4" in L.crh_last_error()
        assert L.crh_noise_uniform_f32(y.data_ptr(), 8, d, 1, None, 0, s) == -1
    assert L.crh_perturb_rows_f32(y.data_ptr(), 8, 64, 0.1, None, 1, None, 0, y.data_ptr(), 1.0, None, 1.0, s) == -1
    assert b"acc_in given without acc_out" in L.crh_last_error()
    assert L.crh_perturb_rows_f32(None, 8, 64, 0.1, None, 1, None, 0, None, 1.0, None, 1.0, s) == -1
    torch.cuda.synchronize()
    assert torch.equal(y, before)
    with pytest.raises(RuntimeError, match="no CPU path"):
        from coldrec_amd import ops
        ops.perturb_rows(torch.zeros(4, 8), 0.1)
