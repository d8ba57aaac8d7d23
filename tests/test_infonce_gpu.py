"""crh_infonce_f32 and the drop-in ``util.utils.InfoNCE`` on the MI355X.

Oracle: float64 autograd of the reference's formula (util/utils.py:61-76) on the same GPU inputs.  Bars: loss within 1e-5
relative, gradients within 1e-4 x max|g64| and no worse than 2x the error of the same formula run by torch in fp32.  G18(i)
(tests/golden/g18_infonce.npz) holds the reference's own numbers; tests/test_infonce.py pins the float64 restatement to it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from coldrec_amd import ops
from coldrec_amd.util.utils import InfoNCE
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def formula(v1, v2, tau, b_cos):
    if b_cos:
        v1, v2 = F.normalize(v1, dim=1), F.normalize(v2, dim=1)
    return -torch.diag(F.log_softmax((v1 @ v2.T) / tau, dim=1)).mean()


def formula_grads(v1, v2, tau, b_cos, dtype):
    a = v1.detach().to(dtype).requires_grad_()
    b = v2.detach().to(dtype).requires_grad_()
    loss = formula(a, b, tau, b_cos)
    loss.backward()
    return loss.item(), a.grad, b.grad


def views(n, d, seed, scale=0.3):
    g = torch.Generator(device=DEV).manual_seed(seed)
    v1 = torch.randn(n, d, device=DEV, generator=g) * scale
    v2 = v1 + torch.randn(n, d, device=DEV, generator=g) * (scale * 0.7)
    return v1.contiguous(), v2.contiguous()


def check_against_fp64(v1, v2, tau, b_cos, loss, g1, g2, label):
    l64, a64, b64 = formula_grads(v1, v2, tau, b_cos, torch.float64)
    _, a32, b32 = formula_grads(v1, v2, tau, b_cos, torch.float32)
    assert abs(float(loss) - l64) <= 1e-5 * abs(l64) + 1e-6, (label, float(loss), l64)
    for got, ref, t32 in ((g1, a64, a32), (g2, b64, b32)):
        big = ref.abs().max().item()
        err = (got.double() - ref).abs().max().item()
        err32 = (t32.double() - ref).abs().max().item()
        assert err <= 1e-4 * big + 1e-30, (label, err, big)
        assert err <= 2 * err32 + 1e-6 * big, (label, err, err32, big)


GRID_N = [1, 2, 31, 32, 33, 257, 1000, 4096, 5000]
GRID_D = [4, 8, 64, 128, 256]


@pytest.mark.parametrize("n", GRID_N)
@pytest.mark.parametrize("d", GRID_D)
def test_infonce_matches_float64_over_n_and_d(n, d):
    v1, v2 = views(n, d, seed=n * 1000 + d)
    loss, g1, g2 = ops.infonce(v1, v2, 0.2, True)
    check_against_fp64(v1, v2, 0.2, True, loss.item(), g1, g2, (n, d))


@pytest.mark.parametrize("n", [33, 1000, 4096])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("tau", [0.05, 0.2, 1.0])
@pytest.mark.parametrize("b_cos", [True, False])
def test_infonce_matches_float64_over_tau_and_b_cos(n, d, tau, b_cos):
    v1, v2 = views(n, d, seed=7 + n + d, scale=0.3 if b_cos else 1.0 / np.sqrt(d))
    loss, g1, g2 = ops.infonce(v1, v2, tau, b_cos)
    check_against_fp64(v1, v2, tau, b_cos, loss.item(), g1, g2, (n, d, tau, b_cos))


@pytest.mark.parametrize("tau", [0.05, 0.2, 1.0])
@pytest.mark.parametrize("b_cos", [True, False])
def test_drop_in_width_50_gathered_non_contiguous_autograd(tau, b_cos):
    n, d = 300, 50
    T1 = torch.randn(800, d, device=DEV) * 0.3
    T2 = torch.randn(d, 900, device=DEV) * 0.3                          # the second view is a transposed column gather
    idx1 = torch.randperm(800, device=DEV)[:n]
    idx2 = torch.randperm(900, device=DEV)[:n]
    a = T1.clone().requires_grad_()
    b = T2.clone().requires_grad_()
    v1, v2 = a[idx1], b[:, idx2].t()
    assert not v2.is_contiguous()
    loss = InfoNCE(v1, v2, tau, b_cos)
    loss.backward()
    ref = T1.double().requires_grad_()
    refb = T2.double().requires_grad_()
    l64 = formula(ref[idx1], refb[:, idx2].t(), tau, b_cos)
    l64.backward()
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item())
    for got, want in ((a.grad, ref.grad), (b.grad, refb.grad)):
        assert (got.double() - want).abs().max().item() <= 1e-4 * want.abs().max().item()


def test_raw_dot_products_with_large_logits_stay_finite():
    """b_cos = 0, tau = 1: every logit ~1e3 (a shared component of norm 32), spread by O(10) -> exp would overflow without
    the running max; the softmax is neither uniform nor one-hot."""
    n, d = 512, 64
    v1, v2 = views(n, d, seed=3, scale=0.3)
    common = torch.full((d,), 4.0, device=DEV)
    v1, v2 = (v1 + common).contiguous(), (v2 + common).contiguous()
    loss, g1, g2 = ops.infonce(v1, v2, 1.0, False)
    s = v1 @ v2.T
    assert s.min().item() > 800 and s.max().item() > 1000
    assert torch.isfinite(loss).all() and torch.isfinite(g1).all() and torch.isfinite(g2).all()
    l64, a64, b64 = formula_grads(v1, v2, 1.0, False, torch.float64)
    assert l64 > 0.1                                # not one-hot
    assert abs(loss.item() - l64) <= 1e-4 * abs(l64)
    for got, ref in ((g1, a64), (g2, b64)):
        assert (got.double() - ref).abs().max().item() <= 1e-3 * ref.abs().max().item()


def test_one_row_gives_zero_loss_and_zero_gradients():
    for b_cos in (True, False):
        v1, v2 = views(1, 64, seed=1)
        loss, g1, g2 = ops.infonce(v1, v2, 0.2, b_cos)
        assert loss.item() == 0.0
        assert (g1 == 0).all() and (g2 == 0).all()


def test_rows_scale_accumulate_match_the_gathered_call_bitwise():
    n, d = 700, 64
    T1 = torch.randn(2000, d, device=DEV) * 0.3
    T2 = torch.randn(1500, d, device=DEV) * 0.3
    r1 = torch.randperm(2000, device=DEV)[:n].int()
    r2 = torch.randperm(1500, device=DEV)[:n].int()
    loss, g1, g2 = ops.infonce(T1[r1.long()].contiguous(), T2[r2.long()].contiguous(), 0.2, True)
    G1 = torch.randn(2000, d, device=DEV)
    G2 = torch.randn(1500, d, device=DEV)
    pre1, pre2 = G1.clone(), G2.clone()
    loss_r, _, _ = ops.infonce(T1, T2, 0.2, True, rows1=r1, rows2=r2, scale=0.5, accumulate=True, grad1=G1, grad2=G2)
    assert torch.equal(loss_r, loss)
    assert torch.equal(G1[r1.long()], pre1[r1.long()] + 0.5 * g1)
    assert torch.equal(G2[r2.long()], pre2[r2.long()] + 0.5 * g2)
    untouched1 = torch.ones(2000, dtype=torch.bool, device=DEV)
    untouched1[r1.long()] = False
    assert torch.equal(G1[untouched1], pre1[untouched1])
    # overwrite mode writes the batch rows only
    H1 = torch.full((2000, d), 7.0, device=DEV)
    H2 = torch.full((1500, d), 7.0, device=DEV)
    ops.infonce(T1, T2, 0.2, True, rows1=r1, rows2=r2, grad1=H1, grad2=H2)
    assert torch.equal(H1[r1.long()], g1) and torch.equal(H2[r2.long()], g2)
    assert (H1[untouched1] == 7.0).all()


def test_device_count_reads_n_from_memory():
    n, n_max, d = 777, 1024, 64
    T1, T2 = views(n_max, d, seed=5)
    r = torch.randperm(n_max, device=DEV).int()
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    G1 = torch.full((n_max, d), 3.0, device=DEV)
    G2 = torch.full((n_max, d), 3.0, device=DEV)
    loss, _, _ = ops.infonce(T1, T2, 0.2, True, rows1=r, rows2=r, n_dev=n_dev, grad1=G1, grad2=G2)
    rl = r[:n].long()
    check_against_fp64(T1[rl], T2[rl], 0.2, True, loss.item(), G1[rl], G2[rl], "n_dev")
    rest = r[n:].long()
    assert (G1[rest] == 3.0).all() and (G2[rest] == 3.0).all()


def test_two_calls_are_bitwise_equal():
    v1, v2 = views(4096, 64, seed=11)
    a = ops.infonce(v1, v2, 0.2, True)
    b = ops.infonce(v1, v2, 0.2, True)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_peak_memory_is_workspace_plus_order_n_d():
    n, d = 32768, 64
    v1, v2 = views(n, d, seed=2)
    g1, g2 = torch.empty_like(v1), torch.empty_like(v2)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(DEV)
    base = torch.cuda.memory_allocated(DEV)
    loss, _, _ = ops.infonce(v1, v2, 0.2, True, grad1=g1, grad2=g2)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(DEV) - base
    ws = ops.infonce_workspace_bytes(n, d)
    assert peak <= ws + 4 * n * d * 4, (peak, ws)
    assert ws < (n * n * 4) // 16                   # the formula's logits alone: 4 GiB
    assert torch.isfinite(loss).all() and torch.isfinite(g1).all()


def g18_zero_rows(v, b_cos):
    """Rows whose gradient is grad / 1e-12 (F.normalize's clamp): 1e10 - 1e12 in G18, so they get a bar of their own."""
    return (np.abs(v).sum(1) == 0) & bool(b_cos)


def assert_rows_close(got, ref, zero, rel, label):
    """got vs ref with the bar rel x max|ref| taken separately over the clamped zero rows and over all other rows."""
    for sel in (zero, ~zero):
        if sel.any():
            err = np.abs(got[sel] - ref[sel]).max()
            assert err <= rel * np.abs(ref[sel]).max() + 1e-30, (label, bool(sel is zero), err)


def test_the_drop_in_reproduces_the_references_g18():
    g = load_golden("g18_infonce.npz")
    for name in g["cases"]:
        name = str(name)
        b_cos = bool(g[f"{name}_bcos"])
        v1 = torch.from_numpy(g[f"{name}_v1"]).to(DEV).requires_grad_()
        v2 = torch.from_numpy(g[f"{name}_v2"]).to(DEV).requires_grad_()
        loss = InfoNCE(v1, v2, float(g[f"{name}_tau"]), b_cos)
        loss.backward()
        want = float(g[f"{name}_loss"])
        assert abs(loss.item() - want) <= 1e-5 * abs(want) + 1e-6, name
        for v, got, ref in ((g[f"{name}_v1"], v1.grad, g[f"{name}_g1"]), (g[f"{name}_v2"], v2.grad, g[f"{name}_g2"])):
            assert_rows_close(got.double().cpu().numpy(), ref, g18_zero_rows(v, b_cos), 1e-4, name)


def test_loss_only_calls_skip_the_gradients():
    """Under no_grad the drop-in computes no gradient; ops.infonce without grad2 skips the column pass.  The loss is the
    same bits as the full call's, and grad1 alone equals the full call's grad1."""
    v1, v2 = views(1000, 64, seed=21)
    loss, g1, g2 = ops.infonce(v1, v2, 0.2, True)
    l1, h1, h2 = ops.infonce(v1, v2, 0.2, True, want_grad2=False)
    assert h2 is None and torch.equal(l1, loss) and torch.equal(h1, g1)
    l0, n1, n2 = ops.infonce(v1, v2, 0.2, True, want_grad1=False, want_grad2=False)
    assert n1 is None and n2 is None and torch.equal(l0, loss)
    a, b = v1.clone().requires_grad_(), v2.clone().requires_grad_()
    with torch.no_grad():
        ln = InfoNCE(a, b, 0.2)
    assert not ln.requires_grad and torch.equal(ln, loss[0])
    b.requires_grad_(False)
    InfoNCE(a, b, 0.2).backward()
    assert torch.equal(a.grad, g1) and b.grad is None


def test_caller_buffers_are_checked():
    v1, v2 = views(64, 8, seed=4)
    with pytest.raises(RuntimeError, match="gradient buffers"):
        ops.infonce(v1, v2, 0.2, grad1=torch.zeros(64, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="gradient buffers"):
        ops.infonce(v1, v2, 0.2, grad2=torch.zeros(8, 64, device=DEV).t())
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.infonce(v1, v2, 0.2, grad1=torch.zeros(64, 8))
    with pytest.raises(RuntimeError, match="loss"):
        ops.infonce(v1, v2, 0.2, loss=torch.zeros(1, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="n_dev"):
        ops.infonce(v1, v2, 0.2, n_dev=torch.tensor([3], device=DEV))
    with pytest.raises(RuntimeError, match="row ids"):
        ops.infonce(v1, v2, 0.2, rows1=torch.arange(64, device=DEV))


def test_a_simgcl_style_plugin_trains_through_the_drop_in():
    """A plugin's contrastive term as model/SimGCL.py:53-60 writes it (unique ids, two views, InfoNCE twice, cl_rate), with
    util.utils.InfoNCE swapped in: its gradients match torch's on the same views, and a few Adam steps lower the loss."""
    torch.manual_seed(0)
    U = torch.nn.Parameter(torch.randn(500, 64, device=DEV) * 0.1)
    I = torch.nn.Parameter(torch.randn(800, 64, device=DEV) * 0.1)
    noise_u, noise_i = torch.rand(500, 64, device=DEV), torch.rand(800, 64, device=DEV)

    def views_of(t, noise):
        return t + torch.sign(t) * F.normalize(noise, dim=-1) * 0.1, t - torch.sign(t) * F.normalize(noise.flip(0), dim=-1) * 0.1

    users = torch.randint(0, 500, (256,), device=DEV)
    items = torch.randint(0, 800, (256,), device=DEV)

    def cl_loss(fn, U, I):
        u_idx, i_idx = torch.unique(users), torch.unique(items)
        u1, u2 = views_of(U, noise_u)
        i1, i2 = views_of(I, noise_i)
        return 0.5 * (fn(u1[u_idx], u2[u_idx], 0.2) + fn(i1[i_idx], i2[i_idx], 0.2))

    ours = cl_loss(InfoNCE, U, I)
    gU, gI = torch.autograd.grad(ours, (U, I))
    ref = cl_loss(lambda a, b, t: formula(a.double(), b.double(), t, True), U, I)
    rU, rI = torch.autograd.grad(ref, (U, I))
    assert abs(ours.item() - ref.item()) <= 1e-5 * abs(ref.item())
    for got, want in ((gU, rU), (gI, rI)):
        assert (got.double() - want).abs().max().item() <= 1e-4 * want.abs().max().item()
    opt = torch.optim.Adam([U, I], lr=1e-2)
    first = None
    for _ in range(5):
        loss = cl_loss(InfoNCE, U, I)
        first = loss.item() if first is None else first
        opt.zero_grad()
        loss.backward()
        opt.step()
    assert cl_loss(InfoNCE, U, I).item() < first
