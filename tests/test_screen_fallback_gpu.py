"""The screened route's exact fallback at the sizes where its slicing changes (run with -m gpu on an MI355X).

The fallback splits each uncertified user's item range into slices chosen on the device from the count of uncertified users:
thousands of them get a few slices each and one merge level, a handful get hundreds to thousands of slices each and a second
merge level.  Every case asserts that the screened call equals the exact route (CRH_SCORE_SCREEN=0) for every user, bit for bit,
and the C oracle on sampled users (the helpers of test_score_screen_gpu)."""
import numpy as np
import pytest

from tests.test_score_screen_gpu import _check, _rated, _tables

pytestmark = pytest.mark.gpu


def test_fallback_every_user_thousands_by_millions(monkeypatch):
    """CRH_SCORE_SCREEN=3 (inside _check) sends all 3 000 users through the fallback over 2 M items: a few slices per user,
    one merge level.  Off-grid shard base, rated lists that straddle the shard, a 20 % bitmap, users through `users`."""
    rng = np.random.default_rng(21)
    n_rows, n_items, base = 5000, 2_000_003, 777_777
    U, V = _tables(rng, n_rows, n_items)
    users = rng.integers(0, n_rows, 3000).astype(np.int32)
    rated = _rated(rng, 3000, base - 100, base + n_items + 100)
    cold = base + np.where(rng.random(n_items) < 0.2)[0]
    unc = _check(monkeypatch, U, V, users=users, rated=rated, bitmap_ids=cold, item_base=base, n_sample=8)
    assert unc <= 3            # gaussian tables: the screen certifies (almost) every user


@pytest.mark.parametrize("n_zero", [1, 5, 40])
def test_fallback_few_users_two_merge_levels(monkeypatch, n_zero):
    """Zero user rows tie every item at 0, so exactly those users stay uncertified under CRH_SCORE_SCREEN=2; with few of them
    each gets hundreds of slices and the merge runs its second level.  Their answer is the lowest unmasked ids."""
    rng = np.random.default_rng(22 + n_zero)
    n_users, n_items = 2000, 1_500_017
    U, V = _tables(rng, n_users, n_items)
    zero = rng.choice(n_users, n_zero, replace=False)
    U[zero] = 0.0
    rated = _rated(rng, n_users, 0, n_items)
    for j in zero[: n_zero // 2 + 1]:            # some of them have rated the lowest ids: those must stay out
        rated[j] = np.union1d(rated[j], np.arange(0, 30, 2))
    cold = np.where(rng.random(n_items) < 0.2)[0]
    unc = _check(monkeypatch, U, V, rated=rated, bitmap_ids=cold, n_sample=6)
    assert n_zero <= unc <= n_zero + 3
