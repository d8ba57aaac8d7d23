"""CPU-only: which calls the library screens (crh_score_topk_screened under CRH_SCORE_SCREEN), and that the screened route lives
inside the workspace the exact route asks for."""
import pytest

from coldrec_amd import _lib, ops


def test_screen_default_gate(monkeypatch):
    monkeypatch.delenv("CRH_SCORE_SCREEN", raising=False)
    head = ops.score_topk_route(131072, 10_000_000, 128, 20)
    # the exact route it replaces is still reported as such (the shard pin `code | 32` holds)
    assert head["screened"] and head["route"] == "fused-dma" and head["dma_form"] == "barrier" and head["prefix_items"] == 8192
    assert not ops.score_topk_route(131072, 1_250_000, 128, 20)["screened"]           # flag form: not screened
    assert not ops.score_topk_route(131072, 10_000_000, 128, 21)["screened"]          # k > 20
    assert not ops.score_topk_route(131072, 10_000_000, 64, 20)["screened"]           # fp32 d=64
    assert not ops.score_topk_route(131072, 10_000_000, 128, 20, half=True)["screened"]
    assert not ops.score_topk_route(131072, 10_000_000, 128, 20, n_splits=1)["screened"]
    assert not ops.score_topk_route(131072, 10_000_000, 128, 20, pack=False)["screened"]   # workspace too small
    assert not ops.score_topk_route(8192, 262144, 128, 20)["screened"]


@pytest.mark.parametrize("mode,small,head", [("0", False, False), ("1", False, True), ("2", True, True), ("3", True, True)])
def test_screen_switch(monkeypatch, mode, small, head):
    monkeypatch.setenv("CRH_SCORE_SCREEN", mode)
    assert ops.score_topk_route(3000, 100_000, 128, 20)["screened"] == small
    assert ops.score_topk_route(700, 48, 128, 20)["screened"] == small
    assert ops.score_topk_route(131072, 10_000_000, 128, 20)["screened"] == head
    assert not ops.score_topk_route(3000, 100_000, 64, 20)["screened"]


def test_screen_workspace_unchanged(monkeypatch):
    L = _lib.lib()
    ws = L.crh_score_topk_workspace_bytes(131072, 10_000_000, 128, 20)
    for mode in ("0", "1", "2", "3"):
        monkeypatch.setenv("CRH_SCORE_SCREEN", mode)
        assert L.crh_score_topk_workspace_bytes(131072, 10_000_000, 128, 20) == ws
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    assert L.crh_score_topk_screened(4, 131072, 10_000_000, 128, 20, ws, 1, 0) == 1
    assert L.crh_score_topk_screened(4, 131072, 10_000_000, 128, 20, ws // 2, 1, 0) == 0      # too little workspace
    assert L.crh_score_topk_screened(2, 131072, 10_000_000, 128, 20, ws, 1, 0) == 0
