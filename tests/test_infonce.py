"""CPU-only checks of crh_infonce_f32 (include/coldrec_hip.h): argument errors without a GPU, the workspace formula, and a
float64 restatement of InfoNCE's loss and closed-form gradients that reproduces G18(i), the reference's own autograd numbers.
The restatement pins the math the kernel implements (P - I, F.normalize's clamped backward) to the reference; the GPU tests
check the kernel against G18(i) directly and against float64 torch autograd of the formula.  tests/infonce_restate.py restates
the same loss in the form that does not cancel where P_ii ~ 1 (the reference of tests/test_infonce_edges_gpu.py and of the
fuzzer): it is pinned here to G18(i), to float64 autograd, and -- in float32 -- shown to hold the row-by-row bar that plain
float32 autograd misses."""
import numpy as np
import pytest
import torch

from coldrec_amd import _lib, ops
from tests import infonce_restate
from tests.conftest import load_golden


def infonce64(v1, v2, tau, b_cos):
    """Loss and both input gradients of util/utils.py:61-76 in float64, without autograd: P = softmax_rows(S),
    dZ1 = (P - I) Z2 / (N tau), dZ2 = (P - I)^T Z1 / (N tau), then F.normalize's backward (norm clamped at 1e-12; below the
    clamp the norm gets no gradient)."""
    v1, v2 = np.asarray(v1, np.float64), np.asarray(v2, np.float64)
    n = v1.shape[0]

    def fwd(v):
        nr = np.sqrt((v * v).sum(1))
        den = np.maximum(nr, 1e-12)
        return v / den[:, None], nr, den

    def bwd(v, g, nr, den):
        live = (nr >= 1e-12)[:, None]
        dot = (g * v).sum(1, keepdims=True)
        corr = np.where(live, v * dot / (den * den)[:, None] / np.where(nr > 0, nr, 1.0)[:, None], 0.0)
        return g / den[:, None] - corr

    if b_cos:
        z1, n1, d1 = fwd(v1)
        z2, n2, d2 = fwd(v2)
    else:
        z1, z2 = v1, v2
    s = z1 @ z2.T / tau
    m = s.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(s - m).sum(1))
    loss = float(np.mean(lse - np.diag(s)))
    p = np.exp(s - lse[:, None]) - np.eye(n)
    g1, g2 = p @ z2 / (n * tau), p.T @ z1 / (n * tau)
    if b_cos:
        g1, g2 = bwd(v1, g1, n1, d1), bwd(v2, g2, n2, d2)
    return loss, g1, g2


def test_float64_restatement_reproduces_the_references_infonce_g18():
    g = load_golden("g18_infonce.npz")
    for name in g["cases"]:
        name = str(name)
        loss, g1, g2 = infonce64(g[f"{name}_v1"], g[f"{name}_v2"], float(g[f"{name}_tau"]), bool(g[f"{name}_bcos"]))
        want = float(g[f"{name}_loss"])
        assert abs(loss - want) <= 1e-12 * max(1.0, abs(want)), name
        for v, got, ref in ((g[f"{name}_v1"], g1, g[f"{name}_g1"]), (g[f"{name}_v2"], g2, g[f"{name}_g2"])):
            # a zero row's gradient is grad / 1e-12 under b_cos: it and the other rows are held to bars of their own
            zero = (np.abs(v).sum(1) == 0) & bool(g[f"{name}_bcos"])
            for sel in (zero, ~zero):
                if sel.any():
                    assert np.abs(got[sel] - ref[sel]).max() <= 1e-10 * max(np.abs(ref[sel]).max(), 1e-30), name


def test_cancellation_free_restatement_reproduces_g18():
    """tests/infonce_restate.py in float64 against the reference's own numbers, to the bars infonce64 is held to above."""
    g = load_golden("g18_infonce.npz")
    for name in g["cases"]:
        name = str(name)
        b_cos = bool(g[f"{name}_bcos"])
        term, loss, g1, g2 = infonce_restate.infonce(g[f"{name}_v1"], g[f"{name}_v2"], float(g[f"{name}_tau"]), b_cos)
        want = float(g[f"{name}_loss"])
        assert abs(float(loss) - want) <= 1e-12 * max(1.0, abs(want)), name
        assert term.shape == (g[f"{name}_v1"].shape[0],)
        for v, got, ref in ((g[f"{name}_v1"], g1.numpy(), g[f"{name}_g1"]), (g[f"{name}_v2"], g2.numpy(), g[f"{name}_g2"])):
            zero = (np.abs(v).sum(1) == 0) & b_cos
            for sel in (zero, ~zero):
                if sel.any():
                    assert np.abs(got[sel] - ref[sel]).max() <= 1e-10 * max(np.abs(ref[sel]).max(), 1e-30), name


def _plain_views(n, d, seed, scale):
    g = torch.Generator().manual_seed(seed)
    v1 = torch.randn(n, d, generator=g) * scale
    return v1, v1 + torch.randn(n, d, generator=g) * (scale * 0.7)


def test_cancellation_free_restatement_agrees_with_float64_autograd():
    """Row by row, to 1e-8 of each row's own maximum, wherever float64 autograd of the formula is itself good: inputs whose
    smallest 1 - P_ii is >= 1e-7 (asserted).  Closer to 1 autograd's (P - I) cancels in float64 too -- 6e-10 at 7e-8 on
    mixed-256x64, about 3e-7 at 1e-10 -- and stops being a reference; the restatement does not cancel there."""
    cases = {k: v[:3] + (True,) for k, v in infonce_restate.peaked_cases().items() if k in ("mixed-130x132", "peaked-64x32",
                                                                                          "anti-64x32")}
    for tau in (0.05, 0.2, 1.0):
        for b_cos in (True, False):
            cases[f"plain-{tau}-{int(b_cos)}"] = _plain_views(97, 36, 11, 0.3 if b_cos else 0.08) + (tau, b_cos)
    worst = 0.0
    for name, (v1, v2, tau, b_cos) in cases.items():
        assert infonce_restate.one_minus_pii(v1, v2, tau, b_cos).min() >= 1e-7, name
        _, loss, g1, g2 = infonce_restate.infonce(v1, v2, tau, b_cos)
        l64, a64, b64 = infonce_restate.autograd(v1, v2, tau, b_cos)
        assert abs(float(loss) - float(l64)) <= 1e-12 * max(1.0, abs(float(l64))), name
        rho = max(infonce_restate.row_rho(g1, a64), infonce_restate.row_rho(g2, b64))
        worst = max(worst, rho)
        assert rho <= 1e-8, (name, rho)
    print(f"restatement vs float64 autograd, worst row-relative distance: {worst:.1e}")


def test_peaked_cases_tell_the_stable_float32_form_from_the_naive_one():
    """The teeth of tests/test_infonce_edges_gpu.py's row-by-row bars, on the CPU.  On every peaked case the float32
    restatement lies within 1e-4 / 8 of the float64 one, row by row (so the GPU bar max(8 x that, 1e-4) is 1e-4 and a
    correct float32 evaluation meets it), and within 1e-5 / 8 on the loss; plain float32 autograd of the formula is off by
    >= 1e-3 on g1 of every case with peaked rows (so a kernel that fell back to the naive diagonal could not pass).
    Measured: restatement 3.7e-6 .. 8.3e-6 (gradients), 5e-9 .. 6.5e-7 (loss); plain autograd 5.6e-3 .. 1.3e-1 on g1."""
    for name, (v1, v2, tau, peaked) in infonce_restate.peaked_cases().items():
        _, l64, a64, b64 = infonce_restate.infonce(v1, v2, tau)
        _, l32, a32, b32 = infonce_restate.infonce(v1, v2, tau, dtype=torch.float32)
        _, an, _ = infonce_restate.autograd(v1, v2, tau, dtype=torch.float32)
        rho = max(infonce_restate.row_rho(a32, a64), infonce_restate.row_rho(b32, b64))
        rel = abs(float(l32) - float(l64)) / abs(float(l64))
        naive = infonce_restate.row_rho(an, a64)
        print(f"{name}: float32 restatement rho {rho:.2e} loss {rel:.2e}; plain float32 autograd rho(g1) {naive:.2e}")
        assert rho <= 1e-4 / 8, (name, rho)
        assert rel <= 1e-5 / 8, (name, rel)
        if peaked.any():
            assert infonce_restate.one_minus_pii(v1, v2, tau)[peaked.numpy()].max() <= 1e-3, name
            assert naive >= 1e-3, (name, naive)
    anti = infonce_restate.peaked_cases()["anti-64x32"]
    assert (infonce_restate.diag_binades_under_max(*anti[:3]) > 100).sum() >= 8


def test_g18_covers_the_cases_the_issue_names():
    g = load_golden("g18_infonce.npz")
    names = [str(n) for n in g["cases"]]
    taus = {float(g[f"{n}_tau"]) for n in names}
    assert taus == {0.05, 0.2, 1.0}
    assert {int(g[f"{n}_bcos"]) for n in names} == {0, 1}
    zero_rows = [n for n in names if (np.abs(g[f"{n}_v1"]).sum(1) == 0).any()]
    dup_rows = [n for n in names if len(np.unique(g[f"{n}_v1"], axis=0)) < g[f"{n}_v1"].shape[0]]
    assert zero_rows and dup_rows
    assert {g[f"{n}_v1"].shape[1] for n in names} >= {4, 8, 50, 64, 128}


def _splits(n_max):
    return _lib.lib().crh_infonce_splits(n_max)


@pytest.mark.parametrize("n_max,d", [(1, 4), (31, 50 + 2), (4096, 64), (4096, 128), (32768, 64), (5000, 256)])
def test_infonce_workspace_formula(n_max, d):
    L = _lib.lib()
    pad = lambda x: (x + 31) // 32 * 32
    r256 = lambda b: (b + 255) // 256 * 256
    n_pad, dp, s = pad(n_max), pad(d), _splits(n_max)
    want = 2 * r256(n_pad * dp * 4) + 5 * r256(n_pad * 4) + 2 * r256(s * n_pad * 4) + r256(s * n_pad * dp * 4)
    assert L.crh_infonce_workspace_bytes(n_max, d) == want
    assert 1 <= s <= 32
    # the splits fill the chip with ~2048 waves (4 per workgroup) and never exceed the tile count
    tiles = n_pad // 32
    assert s <= tiles and (s == tiles or s == 32 or s * ((tiles + 3) // 4) * 4 >= 2048)
    # the N^2 logits of the formula would need n_max^2 * 4 bytes; the workspace is O(n_max * d)
    assert L.crh_infonce_workspace_bytes(n_max, d) <= (2 + s) * n_pad * dp * 4 + (5 + 2 * s) * n_pad * 4 + 10 * 256


def test_infonce_argument_errors_without_gpu():
    L = _lib.lib()
    f = L.crh_infonce_f32
    fake = 1 << 20      # never dereferenced: every check fails before a launch
    assert f(None, None, fake, None, None, 4, 8, 0.2, 1, 1.0, 0, fake, fake, None, fake, 1 << 20, None) == -1
    assert b"NULL" in L.crh_last_error()
    assert f(fake, None, fake, None, None, 4, 6, 0.2, 1, 1.0, 0, fake, fake, None, fake, 1 << 20, None) == -1
    assert b"multiple of 4" in L.crh_last_error()
    assert f(fake, None, fake, None, None, 4, 260, 0.2, 1, 1.0, 0, fake, fake, None, fake, 1 << 20, None) == -1
    assert f(fake, None, fake, None, None, 0, 8, 0.2, 1, 1.0, 0, fake, fake, None, fake, 1 << 20, None) == -1
    assert b"n_max" in L.crh_last_error()
    assert f(fake, None, fake, None, None, 4, 8, 0.0, 1, 1.0, 0, fake, fake, None, fake, 1 << 20, None) == -1
    assert b"tau" in L.crh_last_error()
    assert f(fake, None, fake, None, None, 4, 8, 0.2, 1, 1.0, 0, fake, fake, None, fake, 16, None) == -3
    assert b"workspace" in L.crh_last_error()
    with pytest.raises(RuntimeError, match="workspace"):
        _lib.check(-3, "crh_infonce_f32")
    assert L.crh_infonce_workspace_bytes(0, 8) == 0 and L.crh_infonce_splits(0) == -1
    # gradients are optional (a NULL grad2 skips the column pass), but a call must compute something
    assert f(fake, None, fake, None, None, 4, 8, 0.2, 1, 1.0, 0, None, None, None, fake, 1 << 20, None) == -1
    assert b"nothing to compute" in L.crh_last_error()


def test_contrastive_ops_refuse_cpu_tensors():
    from coldrec_amd.util.utils import InfoNCE
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.infonce(torch.zeros(4, 8), torch.zeros(4, 8), 0.2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        InfoNCE(torch.zeros(4, 8), torch.zeros(4, 8), 0.2)
