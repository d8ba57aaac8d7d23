"""Which screened calls stream their live rows by descending norm (no GPU needed): the library's own predicate, with the workspace
`ops.score_topk` passes -- so these also check that crh_score_topk_workspace_bytes covers the ordered layout."""
import pytest

from coldrec_amd import ops


@pytest.fixture(autouse=True)
def _screen_everywhere(monkeypatch):
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    monkeypatch.delenv("CRH_SCORE_SCREEN_ORDER", raising=False)
    monkeypatch.delenv("CRH_SCORE_SCREEN_COMPACT", raising=False)


@pytest.mark.parametrize("n_users,n_items", [(131072, 10_000_000), (130_700, 70_001), (300, 5_000)])
def test_one_cut_shapes_are_ordered(n_users, n_items):
    plan = ops.score_topk_screen_plan(n_users, n_items, 128, 20)
    assert plan == {"cuts": 1, "compact": True}
    assert ops.score_topk_screen_ordered(n_users, n_items, 128, 20)
    assert ops.score_topk_screen_ordered(n_users, n_items, 128, 1)


@pytest.mark.parametrize("n_users,n_items", [(130, 300_000), (300, 70_001)])
def test_cut_shapes_stay_ascending(n_users, n_items):
    assert ops.score_topk_screen_plan(n_users, n_items, 128, 20)["cuts"] > 1
    assert not ops.score_topk_screen_ordered(n_users, n_items, 128, 20)


def test_switches(monkeypatch):
    shape = (131072, 10_000_000, 128, 20)
    assert not ops.score_topk_screen_ordered(*shape, has_bitmap=False)       # no bitmap, no map
    monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", "0")
    assert not ops.score_topk_screen_ordered(*shape)
    monkeypatch.setenv("CRH_SCORE_SCREEN_ORDER", "1")
    assert ops.score_topk_screen_ordered(*shape)
    monkeypatch.setenv("CRH_SCORE_SCREEN_COMPACT", "0")
    assert not ops.score_topk_screen_ordered(*shape)
