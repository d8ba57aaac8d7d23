"""The two rates behind the rated-tile flags of the screened route, from tools/screen_order_sim.py on
the bench's own rated lists and cold rows: about one unrated candidate in five hits its user's 192-bit membership filter, and a
wave's 128 users rated a row in about one tile in fifty of the live stream."""
import numpy as np

from bench_legs.common import rated_lists
from tools import screen_order_sim as sim

N_USERS, N_ITEMS, PREFIX = 131072, 10_000_000, 8192


def _bench_inputs():
    rowptr, col = rated_lists(N_USERS, N_ITEMS, 50, seed=4)
    cold = np.where(np.random.default_rng(5).random(N_ITEMS) < 0.2)[0]
    return rowptr, col, cold


def test_hash_matches_the_kernel():
    # rated_hash192 of score_topk_dma.hip on a few ids, worked out by hand: ((id * 2654435761 mod 2^32) >> 16) * 192 >> 16
    for gi in (0, 1, 12345, 9_999_999, 2**31 - 2):
        h = (gi * 2654435761) % 2**32
        assert sim.hash192([gi])[0] == ((h >> 16) * 192) >> 16
    assert sim.hash192(np.arange(100000)).max() < 192


def test_filter_fill_and_flagged_tiles_of_the_bench():
    rowptr, col, cold = _bench_inputs()
    lens = np.diff(rowptr)
    assert abs(lens.mean() - 49.4) < 0.5 and np.median(lens) == 27 and lens.max() == 2000 and abs(rowptr[-1] - 6.47e6) < 0.05e6
    # filter fill over the first 8 192 users: 19.3 %.  A user's fill is 1 - e^(-len/192) on average; the mean over 8 192 users of a
    # quantity between 0 and 1 with standard deviation below 0.25 has a standard error below 0.003: four of them (and half a unit of
    # the last digit the figures are quoted to, here and below)
    fill = sim.filter_fill(rowptr, col, np.arange(8192), PREFIX, N_ITEMS)
    print("mean filter fill %.4f (std %.3f)" % (fill.mean(), fill.std()))
    assert fill.std() < 0.25
    assert abs(fill.mean() - 0.193) < 4 * fill.std() / np.sqrt(len(fill)) + 0.0005
    # tiles of the live stream (cold rows and the prefix removed, id order) that hold a row a wave's 128 users rated: 2.0 % mean
    # over 64 waves, 3.4 % at the most; the standard error of the mean comes from the 64 values themselves
    live = np.ones(N_ITEMS, bool)
    live[cold] = False
    live[:PREFIX] = False
    row_of = np.where(live, np.cumsum(live) - 1, -1)
    n_rows = int(live.sum())
    per_wave = sim.flagged_tiles(rowptr, col, row_of, n_rows, 64)
    print("flagged tiles per wave: mean %.4f, max %.4f" % (per_wave.mean(), per_wave.max()))
    assert abs(per_wave.mean() - 0.020) < 4 * per_wave.std() / 8 + 0.0005
    assert per_wave.max() < 0.04
    per_wg = sim.flagged_tiles(rowptr, col, row_of, n_rows, 16, group=512)
    print("flagged tiles per workgroup: mean %.4f" % per_wg.mean())
    assert abs(per_wg.mean() - 0.079) < 4 * per_wg.std() / 4 + 0.001


def test_stream_counts_on_a_small_table():
    """stream() with rated lists: every candidate is counted once, a candidate in a flagged tile is one whose tile the wave rated,
    and rating EVERY row makes every candidate both a filter hit and flagged."""
    rng = np.random.default_rng(1)
    U = rng.standard_normal((256, 128)).astype(np.float32)
    V = rng.standard_normal((sim.SEED + 4096, 128)).astype(np.float32)
    order = np.arange(sim.SEED, len(V))
    rowptr, col = rated_lists(256, len(V), 50, seed=4)
    base = sim.stream(U, V, order)
    res = sim.stream(U, V, order, rated=(rowptr, col.astype(np.int64)))
    assert res[:3] == base and 0 <= res[4] <= res[3] and 0 <= res[5] <= res[3] and res[3] > 0
    full = (np.arange(257, dtype=np.int64) * len(V), np.tile(np.arange(len(V), dtype=np.int64), 256))
    res = sim.stream(U, V, order, rated=full)
    assert res[4] == res[3] == res[5]
