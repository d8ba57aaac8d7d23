"""CPU-only: every decision of the scoring dispatcher against a recorded table.

tests/golden/score_plan_table.json holds, for a grid of shapes, k, flags, environment switches and workspace sizes, what the
library answers without touching a GPU: the full workspace size, the exact route (crh_score_topk_route: code, prefix, cuts),
whether the call is screened, and the screened plan (cuts, compact, ordered, rated tiles), plus the bytes of a prepared item
state.  The workspace sizes include, per answer of the screened plan, the smallest size at which the answer turns true and that
size less one byte (bisected when the table was recorded), so the table pins the workspace layouts to the byte.

The table is a record of the library at one commit (its "recorded_at"); a change that is meant to leave every decision alone
passes against it unchanged.  `python tests/test_score_plan_table.py` records it anew from the library in the tree."""
import contextlib
import ctypes
import itertools
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from coldrec_amd import _lib  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_plan_table.json")

# (element bytes, users, items, d)
SHAPES = [(4, 131072, 10_000_000, 128), (4, 131072, 6_000_000, 128), (4, 8192, 10_000_000, 128), (4, 512, 10_000_000, 128),
          (4, 131072, 1_250_000, 128), (4, 3000, 100_000, 128), (4, 4096, 65_536, 128), (4, 4096, 65_535, 128),
          (4, 700, 48, 128), (4, 1, 33, 128), (4, 131072, 10_000_000, 64), (2, 131072, 10_000_000, 256)]
KS = (1, 20, 21)
FLAGS = tuple(itertools.product((0, 1), (0, 1)))            # (candidate bitmap, rated lists)
ENVS = [{}, {"CRH_SCORE_SCREEN": "0"}, {"CRH_SCORE_SCREEN": "2"},
        {"CRH_SCORE_SCREEN": "2", "CRH_SCORE_SCREEN_COMPACT": "0"}, {"CRH_SCORE_SCREEN": "2", "CRH_SCORE_SCREEN_ORDER": "0"},
        {"CRH_SCORE_SCREEN": "2", "CRH_SCORE_SCREEN_RATED_TILES": "0"}, {"CRH_SCORE_SEED": "0"}, {"CRH_SCORE_SEED": "2"}]
# every switch the recorded decisions read per call: cleared, then the environment of the row set
SWITCHES = ("CRH_SCORE_SCREEN", "CRH_SCORE_SCREEN_COMPACT", "CRH_SCORE_SCREEN_ORDER", "CRH_SCORE_SCREEN_RATED_TILES",
            "CRH_SCORE_SCREEN_PREPARED", "CRH_SCORE_SCREEN_MARGIN", "CRH_SCORE_SEED", "CRH_SCORE_SEED_MAX_ITEMS", "CRH_SCORE_WG",
            "CRH_SCORE_DMA", "CRH_SCORE_DENSE_BLOCK_MB")
SCREENED, COMPACT, ORDERED, RATED_TILES = 1, 2, 4, 8       # bits of a row's last word
SEEDED = 16                                                # bit of the route code


def set_env(env):
    for name in SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(env)


@contextlib.contextmanager
def saved_switches():
    saved = {name: os.environ[name] for name in SWITCHES if name in os.environ}
    try:
        yield
    finally:
        set_env(saved)


def full_bytes(L, esz, n_users, n_items, d, k):
    return int((L.crh_score_topk_f16_workspace_bytes if esz == 2 else L.crh_score_topk_workspace_bytes)(n_users, n_items, d, k))


def screen_bits(L, esz, n_users, n_items, d, k, ws, bitmap, rated):
    """(cuts of the fp16 pass, SCREENED | COMPACT | ORDERED | RATED_TILES) of a call with `ws` bytes of workspace."""
    cuts, compact = ctypes.c_int32(0), ctypes.c_int32(0)
    rc = L.crh_score_topk_screen_plan(n_users, n_items, ws, bitmap, ctypes.byref(cuts), ctypes.byref(compact))
    assert rc == 0
    bits = SCREENED * int(L.crh_score_topk_screened(esz, n_users, n_items, d, k, ws, bitmap, 0))
    bits |= COMPACT * int(compact.value != 0)
    bits |= ORDERED * int(L.crh_score_topk_screen_ordered(n_users, n_items, ws, bitmap))
    bits |= RATED_TILES * int(L.crh_score_topk_screen_rated_tiles(n_users, n_items, ws, bitmap, rated))
    return int(cuts.value), bits


def row(L, esz, n_users, n_items, d, k, ws, bitmap, rated):
    """[workspace bytes, route code, prefix, cuts of the exact route, cuts of the screen's fp16 pass, screen bits]"""
    prefix, splits = ctypes.c_int64(0), ctypes.c_int(0)
    code = L.crh_score_topk_route(esz, n_users, n_items, d, k, ws, bitmap, 0, ctypes.byref(prefix), ctypes.byref(splits))
    assert code > 0, code
    cuts, bits = screen_bits(L, esz, n_users, n_items, d, k, ws, bitmap, rated)
    return [ws, int(code), int(prefix.value), int(splits.value), cuts, bits]


def turning_points(L, esz, n_users, n_items, d, bitmap, rated, top):
    """Under CRH_SCORE_SCREEN=2 and k=20 (the sizes do not depend on k): for each screen bit that is set with `top` bytes, the
    smallest workspace at which it is set and one byte less.  The rated-tile bit is not monotonic -- the order, once the workspace
    holds it, moves the flags further back -- so it is bisected below and from the order's turning point as well."""
    def bit(ws, b):
        return screen_bits(L, esz, n_users, n_items, d, 20, ws, bitmap, rated)[1] & b

    def first_set(lo, hi, b):         # bit clear at lo, set at hi
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if bit(mid, b) else (mid, hi)
        return hi

    out, spans = set(), [(b, 0, top) for b in (SCREENED, COMPACT, ORDERED, RATED_TILES)]
    if bit(top, ORDERED) and not bit(0, ORDERED):
        t = first_set(0, top, ORDERED)
        spans += [(RATED_TILES, 0, t - 1), (RATED_TILES, t, top)]
    for b, lo, hi in spans:
        if hi > lo and bit(hi, b) and not bit(lo, b):
            t = first_set(lo, hi, b)
            out |= {t, t - 1}
    return out


def record(L):
    groups = []
    for (esz, n_users, n_items, d), (bitmap, rated) in itertools.product(SHAPES, FLAGS):
        set_env({"CRH_SCORE_SCREEN": "2"})
        top = max(full_bytes(L, esz, n_users, n_items, d, k) for k in KS)
        turns = turning_points(L, esz, n_users, n_items, d, bitmap, rated, top)
        for k, (e, env) in itertools.product(KS, enumerate(ENVS)):
            set_env(env)
            full = full_bytes(L, esz, n_users, n_items, d, k)
            sizes = sorted({full, full // 2, 0} | turns)
            groups.append({"shape": [esz, n_users, n_items, d], "k": k, "bitmap": bitmap, "rated": rated, "env": e, "full": full,
                           "items_bytes": int(L.crh_score_screen_items_bytes(n_items, bitmap)),
                           "rows": [row(L, esz, n_users, n_items, d, k, ws, bitmap, rated) for ws in sizes]})
    return groups


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_grid(table):
    assert table["envs"] == ENVS
    seen = {(tuple(g["shape"]), g["k"], g["bitmap"], g["rated"], g["env"]) for g in table["groups"]}
    want = {(s, k, b, r, e) for s, k, (b, r), e in itertools.product(SHAPES, KS, FLAGS, range(len(ENVS)))}
    assert seen == want and len(table["groups"]) == len(want)
    for g in table["groups"]:
        sizes = [r[0] for r in g["rows"]]
        assert {g["full"], g["full"] // 2, 0} <= set(sizes)
    # under the default switches and under CRH_SCORE_SCREEN=2 every answer takes both values somewhere
    for e in (0, 2):
        rows = [r for g in table["groups"] if g["env"] == e for r in g["rows"]]
        for name, values in (("screened", {r[5] & SCREENED for r in rows}), ("compact", {r[5] & COMPACT for r in rows}),
                             ("ordered", {r[5] & ORDERED for r in rows}), ("rated tiles", {r[5] & RATED_TILES for r in rows}),
                             ("seeded", {r[1] & SEEDED for r in rows}), ("cuts > 1", {r[4] > 1 for r in rows})):
            assert len(values) == 2, (ENVS[e], name, values)


def test_every_decision_matches_the_table(table):
    L = _lib.lib()
    wrong = []
    with saved_switches():
        for e, env in enumerate(ENVS):
            set_env(env)
            for g in table["groups"]:
                if g["env"] != e:
                    continue
                (esz, n_users, n_items, d), k, bitmap, rated = g["shape"], g["k"], g["bitmap"], g["rated"]
                got = {"full": full_bytes(L, esz, n_users, n_items, d, k),
                       "items_bytes": int(L.crh_score_screen_items_bytes(n_items, bitmap)),
                       "rows": [row(L, esz, n_users, n_items, d, k, r[0], bitmap, rated) for r in g["rows"]]}
                for key, val in got.items():
                    if val != g[key]:
                        wrong.append((g["shape"], k, bitmap, rated, env, key, g[key], val))
    assert not wrong, "%d of %d groups differ; the first: %r" % (len(wrong), len(table["groups"]), wrong[0])


if __name__ == "__main__":
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    commit = subprocess.run(["git", "-C", root, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    commit = os.environ.get("CRH_TABLE_COMMIT", commit)         # (a library built from another checkout: name its commit)
    with saved_switches():
        groups = record(_lib.lib())
    with open(GOLDEN, "w") as f:
        f.write('{"recorded_at": %s,\n "row": ["workspace_bytes", "route_code", "prefix_items", "route_cuts", "screen_cuts", '
                '"screened|compact<<1|ordered<<2|rated_tiles<<3"],\n "envs": %s,\n "groups": [\n' % (json.dumps(commit), json.dumps(ENVS)))
        f.write(",\n".join("  " + json.dumps(g, separators=(",", ":")) for g in groups))
        f.write("\n ]\n}\n")
    print("recorded %d groups, %d rows at %s -> %s" % (len(groups), sum(len(g["rows"]) for g in groups), commit, GOLDEN))
