"""The screened route with a prepared item half of its stage 0 (run with -m gpu on an MI355X).

``ops.prepare_items`` runs the item half once -- the table's scale and norm keys, the live-row map and its sort, the packed fp16
copy with R, N, N^, the tile bits -- into a buffer of its own, and ``ops.score_topk(..., prepared=)`` then runs the user half only.
The prepared state is what the call would have built, so every case runs CRH_SCORE_SCREEN=2 (or 3) and asserts that scores and
ids with a prepared state equal, bit for bit, (a) those of the same call with CRH_SCORE_SCREEN_PREPARED=0 and (b) the exact
route's (CRH_SCORE_SCREEN=0), and (c) that the uncertified count is the same with and without the state.  Reuse is observed
through the library's host counter of item-half runs.

Shapes: those of tests/test_screen_order_gpu.py, for the reasons given there.  300 x 5 000: no prefix, one cut, ordered;
130 700 x 70 001: prefix of 8 192, ragged last tile, one cut, ordered; 300 x 70 001: 30 cuts, compacted but ascending.  Each with a
bitmap and without one (uncompacted, no map).  Every case has an off-grid item base, rated lists and a ``users`` vector with
repeats; one more runs base 0 with users = None."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from coldrec_amd import ops
from coldrec_amd.eval import ShardedTopK

pytestmark = pytest.mark.gpu

K = 20
BASE = 1_000_003
SHAPES = [(300, 5_000), (130_700, 70_001), (300, 70_001)]
# (cuts, compact, ordered) under a bitmap
PLAN = {(300, 5_000): (1, True, True), (130_700, 70_001): (1, True, True), (300, 70_001): (30, True, False)}


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def _bitmap(n_global, ids, dev):
    words = np.zeros((n_global + 31) // 32 + 1, dtype=np.uint32)
    ids = np.asarray(ids, dtype=np.int64)
    np.bitwise_or.at(words, ids >> 5, np.uint32(1) << (ids & 31).astype(np.uint32))
    return torch.from_numpy(words.view(np.int32)).to(dev)


def _rated(rng, n_users, lo, hi, max_len=40):
    lens = rng.integers(0, max_len, n_users)
    owner = np.repeat(np.arange(n_users, dtype=np.int64), lens)
    ids = rng.integers(lo, hi, owner.shape[0], dtype=np.int64)
    key = np.unique((owner << 32) | ids)
    rowptr = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(key >> 32, minlength=n_users), out=rowptr[1:])
    return rowptr, (key & 0xFFFFFFFF).astype(np.int32)


class Case:
    """Tables, masks and user blocks on the device.  ``users`` draws from a table of fewer rows than the block has slots, so it
    repeats rows."""

    def __init__(self, n_users, n_items, bitmap, base=BASE, seed=51, users_vector=True, n_blocks=1):
        dev = _dev()
        rng = np.random.default_rng(seed)
        self.n_users, self.n_items, self.base = n_users, n_items, base
        n_rows = max(64, n_users // 3) if users_vector else n_users
        self.U = torch.from_numpy(rng.standard_normal((n_rows, 128), dtype=np.float32) * np.float32(0.1)).to(dev)
        self.V = torch.from_numpy(rng.standard_normal((n_items, 128), dtype=np.float32) * np.float32(0.1)).to(dev)
        self.bm = _bitmap(base + n_items + 5000, base + np.where(rng.random(n_items) < 0.2)[0], dev) if bitmap else None
        self.blocks = []
        for _ in range(n_blocks):
            users = torch.from_numpy(rng.integers(0, n_rows, n_users).astype(np.int32)).to(dev) if users_vector else None
            rp, rc = _rated(rng, n_users, max(base - 50, 0), base + n_items + 50)     # (ids outside the shard as well)
            self.blocks.append((users, torch.from_numpy(rp).to(dev), torch.from_numpy(rc).to(dev)))

    def call(self, monkeypatch, mode, block=0, prepared=None, switch=1, V=None, bm="own", base=None):
        """One ``score_topk`` call -> (scores, ids, uncertified count or None, item-half runs during the call)."""
        monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
        monkeypatch.setenv("CRH_SCORE_SCREEN_PREPARED", str(switch))
        users, rp, rc = self.blocks[block]
        bm = self.bm if isinstance(bm, str) else bm
        before = ops.screen_item_preps()
        s, i = ops.score_topk(self.U, users, self.V if V is None else V, K, rp, rc, bm,
                              item_base=self.base if base is None else base, prepared=prepared)
        torch.cuda.synchronize()
        unc = ops.score_topk_uncertified() if mode else None
        return s.cpu().numpy(), i.cpu().numpy(), unc, ops.screen_item_preps() - before


def _same(a, b):
    assert np.array_equal(a[1], b[1]), np.argwhere((a[1] != b[1]).any(1))[:5]
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))


def _check(monkeypatch, case, mode=2):
    """(a), (b), (c) of the module's docstring for block 0 of the case; returns the uncertified count."""
    exact = case.call(monkeypatch, 0)
    assert exact[3] == 0                                 # the exact route has no stage 0
    monkeypatch.setenv("CRH_SCORE_SCREEN", str(mode))
    assert ops.score_topk_route(case.n_users, case.n_items, 128, K, has_bitmap=case.bm is not None)["screened"]
    before = ops.screen_item_preps()
    prep = ops.prepare_items(case.V, case.bm, case.base).build(case.n_users, K)
    assert ops.screen_item_preps() == before + 1
    with_state = case.call(monkeypatch, mode, prepared=prep)
    assert with_state[3] == 0                            # the call ran the user half only
    without = case.call(monkeypatch, mode, prepared=prep, switch=0)
    assert without[3] == 1
    _same(with_state, without)
    _same(with_state, exact)
    print("uncertified users: prepared %d, per call %d of %d" % (with_state[2], without[2], case.n_users))
    assert with_state[2] == without[2]
    return with_state[2]


@pytest.mark.parametrize("bitmap", [True, False])
@pytest.mark.parametrize("n_users,n_items", SHAPES)
def test_prepared_equals_per_call_and_exact(monkeypatch, n_users, n_items, bitmap):
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    plan = ops.score_topk_screen_plan(n_users, n_items, 128, K, has_bitmap=bitmap)
    ordered = ops.score_topk_screen_ordered(n_users, n_items, 128, K, has_bitmap=bitmap)
    want = PLAN[(n_users, n_items)] if bitmap else (PLAN[(n_users, n_items)][0], False, False)
    assert (plan["cuts"], plan["compact"], ordered) == want
    assert (BASE + (8192 if n_items >= 65536 else 0)) % 32 != 0 and (BASE + n_items) % 32 != 0
    unc = _check(monkeypatch, Case(n_users, n_items, bitmap))
    assert unc == 0          # gaussian tables: the K' = 28 margin certifies every user


@pytest.mark.parametrize("bitmap", [True, False])
def test_prepared_base_zero_all_rows(monkeypatch, bitmap):
    _check(monkeypatch, Case(300, 5_000, bitmap, base=0, users_vector=False, seed=52))


def test_prepared_no_user_certified(monkeypatch):
    """CRH_SCORE_SCREEN=3: every user goes through the exact fallback, which reads the table and the bitmap, not the state."""
    case = Case(300, 5_000, True, seed=53)
    assert _check(monkeypatch, case, mode=3) == case.n_users


@pytest.mark.parametrize("n_users,n_items", [(130_700, 70_001), (300, 70_001)])
def test_prepared_reuse_across_blocks(monkeypatch, n_users, n_items):
    """Three user blocks on one state, the shared scratch overwritten in between by calls of other ops and shapes: one item-half run
    in all, three with the switch off."""
    case = Case(n_users, n_items, True, seed=54, n_blocks=3)
    other = Case(64, 3_000, True, seed=55)
    dense = torch.randn(50, 4_000, device=_dev())
    exact = [case.call(monkeypatch, 0, block=b) for b in range(3)]
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    before = ops.screen_item_preps()
    prep = ops.prepare_items(case.V, case.bm, case.base)           # (built by the first call that uses it)
    got = []
    for b in range(3):
        got.append(case.call(monkeypatch, 2, block=b, prepared=prep))
        mid = ops.screen_item_preps()
        ops.mask_topk(dense, K, write_back=False)
        other.call(monkeypatch, 2 if b else 0)                     # an exact call, then screened calls of another shape
        scribbled = ops.screen_item_preps() - mid
        assert scribbled == (1 if b else 0)
        before += scribbled
    assert ops.screen_item_preps() - before == 1
    for b in range(3):
        _same(got[b], exact[b])
        assert got[b][2] == 0
    off = [case.call(monkeypatch, 2, block=b, prepared=prep, switch=0) for b in range(3)]
    assert [o[3] for o in off] == [1, 1, 1]
    for b in range(3):
        _same(off[b], exact[b])


@pytest.mark.parametrize("force_fits", [False, True])
def test_prepared_mismatch_falls_back(monkeypatch, force_fits):
    """A state made for something else is ignored: the call builds its own item half (the counter rises) and stays right.
    force_fits: the Python-side comparison is switched off, so the handle reaches the library and its own comparison decides."""
    case = Case(300, 70_001, True, seed=56)
    exact = case.call(monkeypatch, 0)
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    exact_nobm = case.call(monkeypatch, 0, bm=None)
    half = case.n_items // 2
    states = {
        "other bitmap tensor": ops.prepare_items(case.V, case.bm.clone(), case.base).build(case.n_users, K),
        "no bitmap": ops.prepare_items(case.V, None, case.base).build(case.n_users, K),
        "other item_base": ops.prepare_items(case.V, case.bm, case.base + 32).build(case.n_users, K),
        "row slice": ops.prepare_items(case.V[:half], case.bm, case.base).build(case.n_users, K),
        # 130 700 users: one cut, ordered; the call has 300 users: 30 cuts, ascending (the library's comparison in both runs)
        "other plan": ops.prepare_items(case.V, case.bm, case.base).build(130_700, K),
    }
    if force_fits:
        monkeypatch.setattr(ops.PreparedItems, "fits", lambda self, *a, **kw: True)
    for name, prep in states.items():
        got = case.call(monkeypatch, 2, prepared=prep)
        assert got[3] == 1, name
        _same(got, exact)
        assert got[2] == 0, name
    # ... and a state made WITH a bitmap handed to a call without one
    got = case.call(monkeypatch, 2, prepared=states["other plan"], bm=None)
    assert got[3] == 1
    _same(got, exact_nobm)
    # the matching state, last: the same calls do reuse it
    prep = ops.prepare_items(case.V, case.bm, case.base).build(case.n_users, K)
    got = case.call(monkeypatch, 2, prepared=prep)
    assert got[3] == 0
    _same(got, exact)


def test_sharded_topk_prepares_once(monkeypatch):
    case = Case(300, 5_000, True, seed=57, n_blocks=2)
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    monkeypatch.setenv("CRH_SCORE_SCREEN_PREPARED", "1")
    eng = ShardedTopK(case.V, case.base, case.base + case.n_items + 5000, K)

    def topk(block):
        users, rp, rc = case.blocks[block]
        before = ops.screen_item_preps()
        s, i = eng.topk(case.U, users, rp, rc, case.bm)
        torch.cuda.synchronize()
        return s.cpu().numpy(), i.cpu().numpy(), None, ops.screen_item_preps() - before

    first, second = topk(0), topk(1)
    assert (first[3], second[3]) == (1, 0)
    _same(first, case.call(monkeypatch, 0, block=0))
    _same(second, case.call(monkeypatch, 0, block=1))
    # an in-place edit moves the table's _version: the next call prepares again, for the new table
    case.V.mul_(2.0)
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    third, fourth = topk(0), topk(1)
    assert (third[3], fourth[3]) == (1, 0)
    _same(third, case.call(monkeypatch, 0, block=0))
    _same(fourth, case.call(monkeypatch, 0, block=1))
    assert not np.array_equal(third[0], first[0])
    monkeypatch.setenv("CRH_SCORE_SCREEN", "2")
    eng.refresh()
    fifth = topk(0)
    assert fifth[3] == 1
    _same(fifth, third)
    # another bitmap tensor of the same words: a new state
    case.bm = case.bm.clone()
    assert topk(0)[3] == 1 and topk(1)[3] == 0


def test_sharded_topk_merge_path_with_prepared_items(tmp_path):
    """world = 1 with CRH_FORCE_COLLECTIVE=1: the all-gather and the canonical merge behind a screened, prepared call (a one-rank
    process group, so in a process of its own)."""
    script = tmp_path / "prepared_merge_worker.py"
    script.write_text(r'''
import os, sys
sys.path.insert(0, os.environ["CR_ROOT"])
import torch, torch.distributed as dist
torch.cuda.set_device(0)
dev = torch.device("cuda", 0)
dist.init_process_group("nccl", device_id=dev)
from coldrec_amd import ops
from coldrec_amd.eval import ShardedTopK
g = torch.Generator(device=dev).manual_seed(3)
U = torch.randn(300, 128, generator=g, device=dev) * 0.1
V = torch.randn(5000, 128, generator=g, device=dev) * 0.1
os.environ["CRH_SCORE_SCREEN"] = "0"
want = ops.score_topk(U, None, V, 20, item_base=1000003)
os.environ["CRH_SCORE_SCREEN"] = "2"
os.environ["CRH_FORCE_COLLECTIVE"] = "1"
eng = ShardedTopK(V, 1000003, 1000003 + 5000, 20, world=1, rank=0)
before = ops.screen_item_preps()
for _ in range(2):
    got = eng.topk(U, None)
    torch.cuda.synchronize()
    assert torch.equal(got[1], want[1]) and torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
assert ops.screen_item_preps() == before + 1
dist.barrier(); dist.destroy_process_group()
print("PREPARED_MERGE_OK")
''')
    env = dict(os.environ, CR_ROOT=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
               MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "PREPARED_MERGE_OK" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])
