"""CPU-only: the sizes and the surface of the screened route's prepared item state (no GPU call is made)."""
import inspect

from coldrec_amd import _lib, ops
from coldrec_amd.eval import ShardedTopK, UserShardedTopK


def test_items_bytes_is_monotonic_and_holds_the_copy_and_the_map():
    L = _lib.lib()
    for has_bitmap in (0, 1):
        sizes = [L.crh_score_screen_items_bytes(n, has_bitmap) for n in (1, 31, 32, 33, 5_000, 65_535, 65_536, 70_001, 10_000_000)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
        assert sizes[0] > 0
    assert L.crh_score_screen_items_bytes(0, 1) == 0
    # the headline: the packed fp16 copy (whole 32-row tiles of 256-byte rows) plus, under a bitmap, one id per row of the main range
    n, prefix = 10_000_000, 8192
    copy = (n + 31) // 32 * 32 * 128 * 2
    with_map, without = L.crh_score_screen_items_bytes(n, 1), L.crh_score_screen_items_bytes(n, 0)
    assert without >= copy and with_map >= copy + (n - prefix) * 4
    assert with_map >= without
    # ... and nothing like a second workspace: the exact route's holds the fp32 copy and the partial lists
    assert with_map <= copy + n * 4 + n // 8 + (1 << 20)
    assert 2 * with_map < L.crh_score_topk_workspace_bytes(131072, n, 128, 20)


def test_entry_points_exist():
    L = _lib.lib()
    for name in ("crh_score_screen_items_bytes", "crh_score_screen_items_prepare", "crh_score_screen_items_destroy",
                 "crh_score_topk_f32_prepared", "crh_score_topk_screen_item_preps"):
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert L.crh_score_topk_screen_item_preps() >= 0
    assert L.crh_score_screen_items_destroy(None) == 0
    rc = L.crh_score_screen_items_prepare(None, 10, 128, None, 0, 4, None, 0, None, 0, None, None)
    assert rc == -1 and b"NULL" in L.crh_last_error()
    assert callable(ops.prepare_items) and "prepared" in inspect.signature(ops.score_topk).parameters
    assert list(inspect.signature(ops.prepare_items).parameters) == ["item_emb", "cand_bitmap", "item_base"]


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_engines_keep_their_signatures():
    E = inspect.Parameter.empty
    assert _params(ShardedTopK.__init__) == [("self", E), ("item_shard", E), ("item_base", E), ("n_items_global", E), ("k", E),
                                             ("world", 1), ("rank", 0), ("group", None)]
    assert _params(ShardedTopK.topk) == [("self", E), ("user_emb", E), ("users", E), ("rated_rowptr", None), ("rated_col", None),
                                         ("cand_bitmap", None), ("n_splits", 0), ("kernel_events", None)]
    assert _params(UserShardedTopK.__init__) == [("self", E), ("items", E), ("k", E), ("world", 1), ("rank", 0), ("group", None)]
    assert _params(UserShardedTopK.topk) == [("self", E), ("user_emb", E), ("users", E), ("rated_rowptr", None), ("rated_col", None),
                                             ("cand_bitmap", None)]
    for eng in (ShardedTopK, UserShardedTopK):
        assert _params(eng.refresh) == [("self", E)]
    assert "refresh()" in ShardedTopK.__doc__ and "_version" in ShardedTopK.__doc__
