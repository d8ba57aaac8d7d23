"""GPU: crh_table_nce_f32 (csrc/table_nce.hip, ops.table_nce) against the float64 restatement tests/ncl_restate.py
(tests/test_ncl.py pins that restatement to the reference's own numbers, G23).  Bars, those of tests/test_infonce_gpu.py:
loss within 1e-5 relative, each gradient within 1e-4 of the float64 gradient's maximum (rows below F.normalize's clamp, whose
gradient is g / 1e-12, get that bar over themselves).  The peaked case is held row by row: 1e-4 of the ROW's maximum (fp32's
6e-8 times the ~10^2 products of a row's sums, with room for their mixed signs) plus 1e-6 of the gradient's maximum."""
import numpy as np
import pytest
import torch

from coldrec_amd import _lib, ops
from tests import ncl_restate
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def inputs(b, n, d, seed, scale=0.3, ids="random"):
    g = torch.Generator().manual_seed(seed)
    table = torch.randn(n, d, generator=g) * scale
    ctx = table * 0.5 + torch.randn(n, d, generator=g) * (scale * 0.6)
    if ids == "equal":
        idx = torch.full((b,), n // 2, dtype=torch.int32)
    else:
        idx = torch.randint(0, n, (b,), generator=g, dtype=torch.int32)
        idx[b // 2] = n - 1                                           # the last row is always a positive
    return ctx.to(DEV).contiguous(), table.to(DEV).contiguous(), idx.to(DEV)


def assert_close(got, ref, label, rel=1e-4):
    got, ref = got.double().cpu(), ref.double()
    big = ref.abs().max().item()
    err = (got - ref).abs().max().item()
    assert err <= rel * big + 1e-30, (label, err, big)


def check(ctx, table, idx, tau, out, label, alias=False):
    loss, g_ctx, g_table = out
    _, l64, c64, t64 = ncl_restate.table_nce(ctx, table, idx, tau)
    assert torch.isfinite(loss).all(), label
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item()) + 1e-6, (label, loss.item(), l64.item())
    if alias:
        assert_close(g_ctx, c64 + t64, label)
        return
    if g_ctx is not None:
        assert_close(g_ctx, c64, (label, "ctx"))
    if g_table is not None:
        assert_close(g_table, t64, (label, "table"))


@pytest.mark.parametrize("d", [36, 132])
@pytest.mark.parametrize("n", [1, 31, 33, 129, 1025])
@pytest.mark.parametrize("b", [1, 31, 32, 33, 129])
def test_matches_float64_over_batch_table_and_width(b, n, d):
    """Every (B, N) pair includes repeated ids once B > 1 and N is small, B > N (129 vs 1 .. 33), N not a multiple of 32
    (padded rows must stay out of l: the loss bar sees one exp(0) in 33) and the last table row as a positive."""
    ctx, table, idx = inputs(b, n, d, seed=b * 10000 + n * 10 + d)
    check(ctx, table, idx, 0.2, ops.table_nce(ctx, table, idx, 0.2), (b, n, d))


@pytest.mark.parametrize("d", [4, 8, 32, 60, 64, 96, 100, 128, 160, 192, 196, 224, 252, 256])
def test_every_width_instantiation(d):
    ctx, table, idx = inputs(33, 129, d, seed=d)
    check(ctx, table, idx, 0.2, ops.table_nce(ctx, table, idx, 0.2), d)


def test_all_ids_equal():
    ctx, table, idx = inputs(70, 129, 36, seed=5, ids="equal")
    loss, g_ctx, g_table = ops.table_nce(ctx, table, idx, 0.2)
    check(ctx, table, idx, 0.2, (loss, g_ctx, g_table), "equal ids")
    other = torch.ones(129, dtype=torch.bool, device=DEV)
    other[129 // 2] = False
    assert (g_ctx[other] == 0).all()


def test_padded_table_rows_do_not_count():
    """N = 33: the table copy has 31 zero rows behind it.  Counted in l, they would move the loss by B log(64 / 33)-ish --
    the restatement with those rows appended shows the size of what the bar has to catch."""
    ctx, table, idx = inputs(40, 33, 36, seed=9)
    loss, _, _ = ops.table_nce(ctx, table, idx, 0.2)
    _, l64, _, _ = ncl_restate.table_nce(ctx, table, idx, 0.2)
    pad = torch.zeros(31, 36, device=DEV)
    _, lpad, _, _ = ncl_restate.table_nce(torch.cat([ctx, pad]), torch.cat([table, pad]), idx, 0.2)
    assert abs(lpad.item() - l64.item()) > 1e-2 * abs(l64.item())
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item())


def split_tiles(y_rows_max, y_rows, splits):
    """Tiles per split of a pass, as csrc/table_nce.hip cuts them: per = ceil(tiles_all / splits), t_begin = cs * per,
    t_end clamped to the tiles that hold rows."""
    tiles_all, n_tiles = (y_rows_max + 31) // 32, (y_rows + 31) // 32
    per = (tiles_all + splits - 1) // splits
    return [max(0, min(cs * per + per, n_tiles) - cs * per) for cs in range(splits)]


def test_column_splits_with_no_tile_and_with_one():
    """Row pass: B = 33 is one workgroup, so the table's 257 tiles are cut into the maximum of 256 splits, two tiles each:
    split 128 holds exactly one, splits 129.. none.  Column pass: batch_max = 160 against n_dev = 70 leaves two of the five
    batch splits without a tile and gives the others one each."""
    L = _lib.lib()
    b, n = 33, 257 * 32
    rs = L.crh_table_nce_splits(b, n, 0)
    got = split_tiles(n, n, rs)
    assert 0 in got and 1 in got and sum(got) == 257, f"crh_table_nce_splits changed: {rs} splits -> {got}"
    ctx, table, idx = inputs(b, n, 36, seed=3)
    check(ctx, table, idx, 0.2, ops.table_nce(ctx, table, idx, 0.2), "row splits")

    b_max, nb, n = 160, 70, 33
    cs = L.crh_table_nce_splits(b_max, n, 1)
    got = split_tiles(b_max, nb, cs)
    assert 0 in got and 1 in got, f"crh_table_nce_splits changed: {cs} splits -> {got}"
    ctx, table, idx = inputs(b_max, n, 36, seed=4)
    n_dev = torch.tensor([nb], dtype=torch.int32, device=DEV)
    out = ops.table_nce(ctx, table, idx, 0.2, n_dev=n_dev)
    check(ctx, table, idx[:nb], 0.2, out, "batch splits")


def test_zero_rows_are_finite_and_match_torch():
    """A zero row in the table (a column with S = 0 and a gradient of g / 1e-12) and a zero row in the batch."""
    ctx, table, idx = inputs(40, 45, 36, seed=6)
    table[7] = 0.0
    ctx[11] = 0.0
    idx[3] = 11
    idx[4] = 7
    loss, g_ctx, g_table = ops.table_nce(ctx, table, idx, 0.2)
    assert torch.isfinite(loss).all() and torch.isfinite(g_ctx).all() and torch.isfinite(g_table).all()
    lt, ct, tt = ncl_restate.table_nce_autograd(ctx, table, idx, 0.2)
    assert abs(loss.item() - lt.item()) <= 1e-5 * abs(lt.item())
    for got, ref, zero in ((g_ctx, ct, 11), (g_table, tt, 7)):
        sel = torch.zeros(45, dtype=torch.bool)
        sel[zero] = True
        assert ref[sel].abs().max() > 1e6 * ref[~sel].abs().max()      # the clamp's g / 1e-12
        assert_close(got.cpu()[sel], ref[sel], "zero row")
        assert_close(got.cpu()[~sel], ref[~sel], "other rows")


def test_peaked_softmax_row_by_row():
    """tau = 0.05 and every batch row a multiple of its own table row: P_pos is within ~1e-4 of 1 and the gradient rows are
    small differences of products.  Unique ids, so grad_ctx's rows are the records."""
    n, d = 129, 64
    g = torch.Generator().manual_seed(8)
    table = (torch.randn(n, d, generator=g) * 0.3).to(DEV)
    ctx = (table * 1.7).contiguous()
    idx = torch.randperm(n, generator=g)[:100].int().to(DEV)
    loss, g_ctx, g_table = ops.table_nce(ctx, table, idx, 0.05)
    term, l64, c64, t64 = ncl_restate.table_nce(ctx, table, idx, 0.05)
    assert term.max().item() < 1e-2                                   # peaked: every P_pos > 0.99
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item())
    for got, ref in ((g_ctx, c64), (g_table, t64)):
        err = (got.double().cpu() - ref).abs().max(1).values
        bar = 1e-4 * ref.abs().max(1).values + 1e-6 * ref.abs().max()
        assert (err <= bar).all(), (err / bar).max().item()


def test_scale_and_accumulate_bitwise():
    ctx, table, idx = inputs(70, 129, 36, seed=12)
    loss, g_ctx, g_table = ops.table_nce(ctx, table, idx, 0.2)
    gc = torch.randn(129, 36, device=DEV)
    gt = torch.randn(129, 36, device=DEV)
    pc, pt = gc.clone(), gt.clone()
    loss2, _, _ = ops.table_nce(ctx, table, idx, 0.2, scale=0.5, accumulate=True, grad_ctx=gc, grad_table=gt)
    assert torch.equal(loss2, loss)                                   # the loss is unscaled
    hit = torch.zeros(129, dtype=torch.bool, device=DEV)
    hit[idx.long()] = True
    assert torch.equal(gc[hit], pc[hit] + 0.5 * g_ctx[hit]) and torch.equal(gc[~hit], pc[~hit])
    assert torch.equal(gt, pt + 0.5 * g_table)
    # overwrite mode writes the batch's rows of grad_ctx only, and every row of grad_table
    hc = torch.full((129, 36), 7.0, device=DEV)
    ht = torch.full((129, 36), 7.0, device=DEV)
    ops.table_nce(ctx, table, idx, 0.2, grad_ctx=hc, grad_table=ht)
    assert torch.equal(hc[hit], g_ctx[hit]) and (hc[~hit] == 7.0).all() and torch.equal(ht, g_table)


def test_each_gradient_null_in_turn_keeps_the_other_outputs_bits():
    ctx, table, idx = inputs(70, 129, 36, seed=13)
    loss, g_ctx, g_table = ops.table_nce(ctx, table, idx, 0.2)
    l1, c1, t1 = ops.table_nce(ctx, table, idx, 0.2, want_grad_table=False)
    assert t1 is None and torch.equal(l1, loss) and torch.equal(c1, g_ctx)
    l2, c2, t2 = ops.table_nce(ctx, table, idx, 0.2, want_grad_ctx=False)
    assert c2 is None and torch.equal(l2, loss) and torch.equal(t2, g_table)
    l3, c3, t3 = ops.table_nce(ctx, table, idx, 0.2, want_grad_ctx=False, want_grad_table=False)
    assert c3 is None and t3 is None and torch.equal(l3, loss)


@pytest.mark.parametrize("n", [-3, 0, 1, 33, 40])
def test_device_batch_size(n):
    b_max, rows, d = 40, 45, 36
    ctx, table, idx = inputs(b_max, rows, d, seed=14)
    n_dev = torch.tensor([n], dtype=torch.int32, device=DEV)
    gc = torch.full((rows, d), 3.0, device=DEV)
    gt = torch.full((rows, d), 3.0, device=DEV)
    loss, _, _ = ops.table_nce(ctx, table, idx, 0.2, n_dev=n_dev, grad_ctx=gc, grad_table=gt)
    nb = min(max(n, 0), b_max)
    hit = torch.zeros(rows, dtype=torch.bool, device=DEV)
    hit[idx[:nb].long()] = True
    assert (gc[~hit] == 3.0).all()                                    # untouched rows keep their bits
    if nb == 0:
        assert loss.item() == 0.0 and (gt == 3.0).all()
        return
    _, l64, c64, t64 = ncl_restate.table_nce(ctx, table, idx[:nb], 0.2)
    assert abs(loss.item() - l64.item()) <= 1e-5 * abs(l64.item()) + 1e-6
    assert_close(gc[hit], c64[hit.cpu()], "ctx")
    assert_close(gt, t64, "table")


def test_ctx_aliasing_the_table():
    _, table, idx = inputs(40, 45, 36, seed=15)
    g = torch.zeros_like(table)
    loss, _, _ = ops.table_nce(table, table, idx, 0.2, accumulate=True, grad_ctx=g, grad_table=g)
    check(table, table, idx, 0.2, (loss, g, g), "alias", alias=True)
    lt, ga, _ = ncl_restate.table_nce_autograd(table, table, idx, 0.2, alias=True)
    assert abs(loss.item() - lt.item()) <= 1e-5 * abs(lt.item())
    assert_close(g, ga, "alias vs autograd")


def test_dirty_oversized_workspace_and_repeat_calls_change_no_bit():
    ctx, table, idx = inputs(70, 129, 36, seed=16)
    a = ops.table_nce(ctx, table, idx, 0.2)
    b = ops.table_nce(ctx, table, idx, 0.2)
    need = ops.table_nce_workspace_bytes(70, 129, 36)
    ws = torch.full((need + 4096,), 0xFF, dtype=torch.uint8, device=DEV)      # NaN bit patterns everywhere
    c = ops.table_nce(ctx, table, idx, 0.2, workspace=ws)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_caller_buffers_are_checked():
    ctx, table, idx = inputs(8, 16, 8, seed=17)
    with pytest.raises(RuntimeError, match="gradient buffers"):
        ops.table_nce(ctx, table, idx, 0.2, grad_table=torch.zeros(16, 8, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.table_nce(ctx, table, idx, 0.2, grad_ctx=torch.zeros(16, 8))
    with pytest.raises(RuntimeError, match="row ids"):
        ops.table_nce(ctx, table, idx.long(), 0.2)
    with pytest.raises(RuntimeError, match="n_dev"):
        ops.table_nce(ctx, table, idx, 0.2, n_dev=torch.tensor([3], device=DEV))
    with pytest.raises(RuntimeError, match="differ in shape"):
        ops.table_nce(ctx[:8].contiguous(), table, idx, 0.2)


def test_the_references_g23_ssl_cases():
    """The reference's own ssl_layer_loss and autograd gradients (tests/golden/make_golden_g23.py): both sides of each case
    through ops.table_nce with the reference's weights, summed as the reference sums them."""
    g = load_golden("g23_ssl.npz")
    for name in g["cases"]:
        name = str(name)
        U, tau = int(g[f"{name}_U"]), float(g[f"{name}_tau"])
        ssl_reg, alpha = float(g[f"{name}_ssl_reg"]), float(g[f"{name}_alpha"])
        init = torch.from_numpy(g[f"{name}_initial"]).to(DEV)
        alias = bool(g[f"{name}_alias"])
        ctx = init if alias else torch.from_numpy(g[f"{name}_context"]).to(DEV)
        user = torch.from_numpy(g[f"{name}_user"]).int().to(DEV)
        item = torch.from_numpy(g[f"{name}_item"]).int().to(DEV)
        g_ctx, g_init = torch.zeros_like(init), torch.zeros_like(init)
        lu, _, _ = ops.table_nce(ctx[:U], init[:U], user, tau, scale=ssl_reg, accumulate=True, grad_ctx=g_ctx[:U],
                                 grad_table=g_init[:U])
        li, _, _ = ops.table_nce(ctx[U:], init[U:], item, tau, scale=ssl_reg * alpha, accumulate=True, grad_ctx=g_ctx[U:],
                                 grad_table=g_init[U:])
        want = float(g[f"{name}_loss"])
        got = ssl_reg * (lu.item() + alpha * li.item())
        assert abs(got - want) <= 1e-5 * abs(want), (name, got, want)
        if alias:
            assert_close(g_ctx + g_init, torch.from_numpy(g[f"{name}_g_initial"]), name)
        else:
            assert_close(g_ctx, torch.from_numpy(g[f"{name}_g_context"]), (name, "context"))
            assert_close(g_init, torch.from_numpy(g[f"{name}_g_initial"]), (name, "initial"))
