"""The batches that pin loss_common.h's owner pass (tests/test_owner_pass_gpu.py runs them on the GPU, tests/test_gar.py and
tests/test_owner_model.py measure and check them on the CPU): one owner-size profile that meets every window and chunk
edge of ``lg_owner_chunk_kernel``, the widths of all seven lane-group instantiations, and GAR batches in which the
regulariser's part -- the part that needs the per-owner count of positives -- decides the gradient.

SIZES: 1, 2 (a window of one or two lanes); 63, 64, 65 (a short window, a full one, one occurrence into the second); 127,
129, 255 (ragged second, third and fourth windows); 256, 257 (a full chunk, one occurrence into the second chunk); 320 (a
second chunk of one full window); 513 (three chunks).
WIDTHS: every LPR = pow2(d / 4) from 1 to 64 at a width that fills its lanes (4, 8, 16, 32, 64, 128, 256) and at one that
leaves lanes without a column (12, 20, 36, 68, 132, 252).
"""
import numpy as np
import torch

from tests import gar_restate
from tests import mtpr_restate
from tests import vbpr_restate

CHUNK = 256                                    # LG_CHUNK; the GPU file asserts that the library's is this
SIZES = (1, 2, 63, 64, 65, 127, 129, 255, 256, 257, 320, 513)
WIDTHS = (4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 252, 256)
MTPR_WIDTHS = tuple(d for d in WIDTHS if d <= 128)      # MTPR's d <= 128; its tables are d and 2 d wide
NU, NI = 40, 60
B = sum(SIZES)                                 # 2052 records: the users hold the profile once, the items twice over 2 B


def _deal(ids, sizes, g):
    """Every id ``sizes[k]`` times, shuffled."""
    run = torch.repeat_interleave(ids, torch.tensor(sizes))
    return run[torch.randperm(run.shape[0], generator=g)]


def profile_ids(seed=0):
    """(users, pos, neg), each (B,): 12 of the NU users own SIZES of the B records, 24 of the NI items own SIZES twice
    over the 2 B occurrences; the ids are drawn from the tables' rows in no order."""
    g = torch.Generator().manual_seed(2700 + seed)
    users = _deal(torch.randperm(NU, generator=g)[:len(SIZES)], SIZES, g)
    occ = _deal(torch.randperm(NI, generator=g)[:2 * len(SIZES)], SIZES + SIZES, g)
    return users, occ[:B].clone(), occ[B:].clone()


def owner_sizes(plan, side):
    return torch.diff(plan[f"{side}_ptr"]).tolist()


def vbpr_inputs(d, cold_user, adv=False, wide=False):
    """tests/vbpr_restate.py's inputs at the profile.  ``wide``: tables scaled so that the scores x spread over tens of
    units at every width (a row's length is constant in d, so the scale grows as d^(1/4))."""
    scale = 1.6 * d ** 0.25 if wide else 1.0
    inp = vbpr_restate.inputs((B, d, NU, NI), cold_user, adv, chunk=CHUNK, seed=11, scale=scale)
    return inp[:5] + profile_ids()


def vbpr_scores(inp, cold_user):
    """x per record in float64."""
    P, Q, A, h = (t.double() for t in inp[:4])
    users, pos, neg = inp[5:]
    base = (P[users] * (Q[pos] - Q[neg])).sum(1)
    n = users.shape[0]
    return base + ((h * (A[pos] - A[neg])).sum(1) if cold_user else (A[users] * (h[:n] - h[n:])).sum(1))


def mtpr_inputs(d, cold_user):
    """tests/mtpr_restate.py's inputs at the profile."""
    return mtpr_restate.inputs((B, d, NU, NI), cold_user, chunk=CHUNK, seed=11)[:5] + profile_ids()


# ---- GAR: the count of positives made visible ------------------------------------------------------------------------
# (occurrences, of them positives) per item.  A plan lists an owner's positives first, so n_first marks a position in the
# owner's run: 0, 1, 63, 64, 65, 255, 256, 257, n - 1 and n, on owners of one, two and three chunks.
GAR_ITEM_OWNERS = (
    (1, 1), (1, 0), (2, 1), (63, 0), (64, 63), (64, 64), (65, 64), (65, 65), (127, 65), (129, 63), (255, 255), (256, 255),
    (200, 1),                                                                                    # one chunk
    (257, 256), (257, 257), (320, 257), (320, 64), (300, 65), (258, 1), (257, 0),                # two chunks
    (513, 512), (513, 1), (513, 257), (513, 0))                                                  # three chunks
GAR_HEAVY = (13, 20)                           # (257, 256) and (513, 512): their rows of V are scaled by GAR_HEAVY_SCALE
GAR_HEAVY_SCALE = 4.0
GAR_MISCOUNTED = 20                            # the three-chunk owner whose count the "one miscounted" mutation moves
GAR_ALPHA, GAR_BETA = 0.05, 0.1


def gar_owners():
    """(item owners with the filler that balances positives and negatives, user sizes): the items' positives and their
    negatives both sum to B; the users hold SIZES and one owner for the rest."""
    own = list(GAR_ITEM_OWNERS)
    n, first = sum(o[0] for o in own), sum(o[1] for o in own)
    spare = 2 * first - n                      # positives over negatives
    if spare:
        own.append((abs(spare), 0 if spare > 0 else abs(spare)))
    n, first = sum(o[0] for o in own), sum(o[1] for o in own)
    assert n == 2 * first
    users = list(SIZES) + [first - sum(SIZES)]
    assert users[-1] > 0
    return own, users


def gar_count_ids(seed=0):
    """(users, pos, neg, item ids in GAR_ITEM_OWNERS' order)."""
    own, user_sizes = gar_owners()
    batch = sum(user_sizes)
    g = torch.Generator().manual_seed(2800 + seed)
    items = torch.randperm(NI, generator=g)[:len(own)]
    pos = _deal(items, [o[1] for o in own], g)
    neg = _deal(items, [o[0] - o[1] for o in own], g)
    users = _deal(torch.randperm(NU, generator=g)[:len(user_sizes)], user_sizes, g)
    assert pos.shape[0] == neg.shape[0] == users.shape[0] == batch
    return users, pos, neg, items


def gar_count_inputs(d):
    """((U, V, users, pos, neg, G), (alpha, beta, reg)) with reg = B; tests/test_gar_gpu.py's tables (randn * 0.3) with the
    rows of the two positive-heavy items scaled by 4, so that the positive block's norm is over twice the negative's."""
    users, pos, neg, items = gar_count_ids()
    g = torch.Generator().manual_seed(2900 + d)
    U, V = torch.randn(NU, d, generator=g) * 0.3, torch.randn(NI, d, generator=g) * 0.3
    V[items[list(GAR_HEAVY)]] *= GAR_HEAVY_SCALE
    G = torch.tanh(torch.randn(users.shape[0], d, generator=g) * 0.3)
    return (U, V, users, pos, neg, G), (GAR_ALPHA, GAR_BETA, float(users.shape[0]))


def gar_mutations(inp, coef, cold_user):
    """The float64 restatement and four mutated ones.  R's part of a table's gradient is written out: factor x count x
    row, factor = reg / (B |block|_F); the rest is the restatement at reg = 0.  Returns (true, {name: mutated}, written),
    each a (terms, d U, d V, d G) tuple of numpy float64; ``written`` is the unmutated sum of the two parts, which must
    equal ``true``."""
    U, V, users, pos, neg, G = inp
    alpha, beta, reg = coef
    true = gar_restate.step(*inp, alpha, beta, reg, cold_user)
    rest = gar_restate.step(*inp, alpha, beta, 0.0, cold_user)
    n = users.shape[0]
    U64, V64 = U.double().numpy(), V.double().numpy()
    f_u, f_p, f_n = (reg / (n * np.linalg.norm(t)) for t in (U64[users.numpy()], V64[pos.numpy()], V64[neg.numpy()]))
    c_u = np.bincount(users.numpy(), minlength=U.shape[0]).astype(np.float64)
    c_p = np.bincount(pos.numpy(), minlength=V.shape[0]).astype(np.float64)
    c_n = np.bincount(neg.numpy(), minlength=V.shape[0]).astype(np.float64)

    def build(cp, cn, fp=f_p, fn=f_n, user_part=True):
        du = rest[1] + (f_u * c_u)[:, None] * U64 if user_part else rest[1]
        return true[0], du, rest[2] + (fp * cp + fn * cn)[:, None] * V64, true[3]

    one = c_p.copy()
    _, _, _, items = gar_count_ids()
    one[int(items[GAR_MISCOUNTED])] -= 1.0
    other = c_n.copy()
    other[int(items[GAR_MISCOUNTED])] += 1.0
    mutated = {"counts swapped": build(c_n, c_p), "all counted as positives": build(c_p + c_n, 0 * c_n),
               "one occurrence miscounted": build(one, other), "R dropped on the user side": build(c_p, c_n, user_part=False)}
    return true, mutated, build(c_p, c_n)
