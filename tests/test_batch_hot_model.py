"""The sweep's hot block restated in numpy (bfs_batch.hip: make_hot, batch_hot_copy): which vertices are hubs, how the
CSC indices and the hint are renamed, and what the tail of a word array holds after a refresh.  No GPU: the GPU suite
(test_gpu_batch_hot.py) compares the library's answer with hub_rule() below.

The rule: with a cap, t is the smallest threshold such that at most cap vertices have out-degree >= t; the hubs are exactly
those vertices in ascending id, slot j the j-th.  Ties at the threshold are all in or all out."""
import numpy as np
import pytest


def hub_rule(deg, cap):
    """(t, hubs) by the definition: try every threshold from 0 up"""
    deg = np.asarray(deg, dtype=np.int64)
    t = 0
    while np.count_nonzero(deg >= t) > cap:
        t += 1
    return t, np.nonzero(deg >= t)[0]


def hub_rule_select(deg, cap):
    """the same by selection, as the library finds it: one more than the (cap + 1)-th largest degree, digit by digit"""
    deg = np.asarray(deg, dtype=np.int64)
    if cap >= deg.size:
        return 0, np.arange(deg.size)
    mask, value, rank = 0, 0, cap
    for shift in (22, 11, 0):
        d = deg[(deg & mask) == value]
        bins = np.bincount((d >> shift) & 2047, minlength=2048)
        digit = 2047
        while digit > 0 and rank >= bins[digit]:
            rank -= bins[digit]
            digit -= 1
        assert rank < bins[digit]
        value |= digit << shift
        mask |= 2047 << shift
    t = value + 1
    hubs = np.nonzero(deg >= t)[0]
    assert hubs.size == cap - rank
    return t, hubs


def rename(ind, n, hubs):
    """every entry that names hub j becomes n + j; an entry that names no vertex (-1) stays"""
    name = np.arange(n, dtype=np.int64)
    name[hubs] = n + np.arange(hubs.size)
    ind = np.asarray(ind, dtype=np.int64)
    return np.where((ind >= 0) & (ind < n), name[np.clip(ind, 0, n - 1)], ind)


def refresh(words, hubs, stride):
    """a word array with its tail: n words, the hubs' words behind them, padding up to the stride"""
    ext = np.zeros(stride, dtype=np.uint64)
    ext[:words.size] = words
    ext[words.size:words.size + hubs.size] = words[hubs]
    return ext


def stride_of(n, H):
    return (n + H + 31) // 32 * 32 if H else n


@pytest.mark.parametrize("seed", range(6))
def test_threshold_and_hubs_on_random_degrees(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    deg = (rng.pareto(1.2, n) * 3).astype(np.int64) if seed % 2 else rng.integers(0, 12, n)
    for cap in [0, 1, 2, 7, n // 3, n - 1, n, n + 5]:
        t, hubs = hub_rule(deg, cap)
        t2, hubs2 = hub_rule_select(deg, cap)
        assert (t, hubs.tolist()) == (t2, hubs2.tolist()), (seed, cap)
        assert hubs.size <= cap and np.all(np.diff(hubs) > 0)
        assert np.all(deg[hubs] >= t) and hubs.size == np.count_nonzero(deg >= t)
        if t > 0:                                                   # the smallest such threshold: one lower is over the cap
            assert np.count_nonzero(deg >= t - 1) > cap


def test_ties_at_the_threshold_stay_out_together():
    deg = np.array([5, 9, 7, 7, 7, 3, 9, 1])
    t, hubs = hub_rule(deg, 2)
    assert (t, hubs.tolist()) == (8, [1, 6])
    for cap in (2, 3, 4):                                           # the three sevens do not fit until cap = 5
        t, hubs = hub_rule_select(deg, cap)
        assert (t, hubs.tolist()) == (8, [1, 6])
    t, hubs = hub_rule_select(deg, 5)
    assert (t, hubs.tolist()) == (6, [1, 2, 3, 4, 6])               # the smallest threshold: one above the sixth largest degree
    t, hubs = hub_rule_select(deg, 1)                               # the two nines tie at the top: nobody is a hub
    assert (t, hubs.size) == (10, 0)


def test_cap_zero_cap_over_n_and_equal_degrees():
    deg = np.array([4, 0, 6, 2])
    for rule in (hub_rule, hub_rule_select):
        assert rule(deg, 0)[0] == 7 and rule(deg, 0)[1].size == 0
        assert rule(deg, 4)[0] == 0 and rule(deg, 4)[1].tolist() == [0, 1, 2, 3]
        assert rule(deg, 9)[1].size == 4
        flat = np.full(50, 4)                                       # a grid, a ring: all in or all out
        for cap in (0, 1, 49):
            t, hubs = rule(flat, cap)
            assert (t, hubs.size) == (5, 0)
        assert rule(flat, 50)[1].size == 50
    t, hubs = hub_rule_select(np.array([1 << 30, 3, (1 << 30) + 1]), 1)   # every digit of the selection in use
    assert (t, hubs.tolist()) == ((1 << 30) + 1, [2])


@pytest.mark.parametrize("seed", range(4))
def test_gathers_through_renamed_indices_read_the_same_words(seed):
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(40, 300))
    nvals = int(rng.integers(n, 8 * n))
    # a skewed index array: most entries name few vertices
    ind = np.minimum((rng.pareto(0.8, nvals)).astype(np.int64), n - 1)
    ind = rng.permutation(n)[ind]
    deg = np.bincount(ind, minlength=n)                             # the occurrences of c ARE c's out-degree
    hint = np.where(rng.random(n) < 0.1, -1, rng.integers(0, n, n))
    for cap in (0, 1, 5, 64, n):
        t, hubs = hub_rule_select(deg, cap)
        H = hubs.size
        stride = stride_of(n, H)
        assert stride % 32 == 0 or H == 0
        ind_hot, hint_hot = rename(ind, n, hubs), rename(hint, n, hubs)
        assert ind_hot.max() < n + H and np.array_equal(hint_hot == -1, hint == -1)
        assert np.array_equal(ind_hot >= n, np.isin(ind, hubs))
        for _ in range(3):
            words = rng.integers(0, 1 << 63, n, dtype=np.uint64)
            ext = refresh(words, hubs, stride)
            assert np.array_equal(ext[ind_hot], words[ind])
            has = hint >= 0
            assert np.array_equal(ext[hint_hot[has]], words[hint[has]])
            assert np.array_equal(ext[:n], words)                   # the kernels that walk [0, n) see what they saw
        if cap == n:
            assert H == n and np.array_equal(ind_hot, ind + n)


def test_a_stale_tail_is_what_the_refresh_prevents():
    rng = np.random.default_rng(7)
    n, hubs = 64, np.array([3, 17, 40])
    ind_hot = rename(np.array([3, 5, 17, 40, 63]), n, hubs)
    old = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    ext = refresh(old, hubs, stride_of(n, hubs.size))
    new = old.copy()
    new[17] ^= np.uint64(1)
    ext[:n] = new                                                   # a level wrote its words; nobody copied
    assert not np.array_equal(ext[ind_hot], new[[3, 5, 17, 40, 63]])
    ext[n:n + hubs.size] = ext[hubs]                                # tail[j] = words[hub[j]]
    assert np.array_equal(ext[ind_hot], new[[3, 5, 17, 40, 63]])
