"""CPU-only: ``ops._owner_chunks``, the grouping behind the plans of the fused CLCRec and CCFCRec losses, against a
brute-force NumPy grouping.  Plain torch, so it runs on CPU tensors."""
import numpy as np
import torch

from coldrec_amd import ops

CHUNK = 4
# id -> group size: exactly one chunk (4), one row over (5), two chunks plus one row (9), and the small groups 1 and 3
SIZES = {7: 1, 40: 3, 2: 4, 11: 5, 5: 9}
CHUNKS = {1: 1, 3: 1, 4: 1, 5: 2, 9: 3}


def _shuffled_ids():
    ids = np.repeat(np.array(list(SIZES.keys()), np.int64), list(SIZES.values()))
    return ids[np.random.RandomState(5).permutation(ids.shape[0])]


def test_owner_chunks_match_a_brute_force_grouping():
    ids = _shuffled_ids()
    assert sorted(np.bincount(ids)[np.bincount(ids) > 0].tolist()) == [1, 3, 4, 5, 9]
    assert any(ids[p] > ids[p + 1] for p in range(len(ids) - 1))          # shuffled: the grouping has something to do
    uniq, order, ptr, chunk_ptr, chunk_own, inv = (t.numpy() for t in ops._owner_chunks(torch.from_numpy(ids), CHUNK))

    want_uniq = sorted(SIZES)
    groups = [[p for p in range(len(ids)) if ids[p] == u] for u in want_uniq]    # positions ascending inside an id
    assert uniq.tolist() == want_uniq and all(a < b for a, b in zip(uniq[:-1], uniq[1:]))
    assert order.tolist() == [p for g in groups for p in g]
    assert ptr.tolist() == np.concatenate([[0], np.cumsum([len(g) for g in groups])]).tolist()
    for j in range(len(groups)):                                          # the stable sort
        mine = order[ptr[j]:ptr[j + 1]]
        assert (ids[mine] == uniq[j]).all() and all(a < b for a, b in zip(mine[:-1], mine[1:]))

    n_chunks = [CHUNKS[SIZES[u]] for u in want_uniq]
    assert n_chunks == [-(-len(g) // CHUNK) for g in groups]
    assert chunk_ptr.tolist() == np.concatenate([[0], np.cumsum(n_chunks)]).tolist()
    assert chunk_own.tolist() == [j for j, n in enumerate(n_chunks) for _ in range(n)]
    for ch, j in enumerate(chunk_own):                                    # chunk ch covers rows of its owner only
        begin = ptr[j] + (ch - chunk_ptr[j]) * CHUNK
        assert ptr[j] <= begin < ptr[j + 1]

    assert inv.tolist() == [want_uniq.index(i) for i in ids.tolist()]
    assert (uniq[inv] == ids).all()
