"""tests/sample_model.py, the host restatement of grb_random_walk and grb_sample_neighbors, against hand-worked cases, and the
spread of the draw it defines: every outcome within 5 % of its expectation for the seeds 0, 1, 12345 and 0xffffffff.  The
spread is a condition on the definition (include/grb_hip.h), not a device measurement.  No GPU."""
import numpy as np
import pytest

import sample_model as sm

I, F = np.int32, np.float32
SEEDS = (0, 1, 12345, 0xffffffff)


def _csr(n, edges, w=None):
    e = sorted(zip(*edges)) if w is None else sorted(zip(edges[0], edges[1], w))
    r = np.array([x[0] for x in e], np.int64)
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    return ptr, np.array([x[1] for x in e], np.int64), np.array([x[2] for x in e] if w is not None else np.ones(len(e)), np.int64)


# ---- the draw ------------------------------------------------------------------------------------------------------------
def test_mix_is_the_murmur3_finaliser():
    assert sm.mix(0) == 0 and sm.mix(1) == 0x514e28b7
    x = np.array([0, 1, 2, 0xffffffff, 0x9e3779b9], np.uint64)
    assert sm.mix(x).tolist() == [sm.mix(int(v)) for v in x]


def test_scalar_and_array_draws_agree_and_wrap():
    for seed in SEEDS:
        a = np.array([0, 1, 77, 2 ** 31 - 1, 2 ** 32 - 1], np.int64)
        b = np.array([0, 5, 2 ** 32 - 1, 3, 10 ** 6], np.int64)
        assert sm.draw(seed, a, b).tolist() == [sm.draw(seed, int(x), int(y)) for x, y in zip(a, b)]
        assert sm.draw(seed, 3, b).tolist() == [sm.draw(seed, 3, int(y)) for y in b]
    assert sm.pick(0xffffffff, 7) == 6 and sm.pick(0, 7) == 0 and sm.pick(0x80000000, 2 ** 31 - 1) == 2 ** 30 - 1
    assert sm.pick(np.array([0xffffffff, 0], np.uint32), np.array([2 ** 31 - 1, 5])).tolist() == [2 ** 31 - 2, 0]


@pytest.mark.parametrize("seed", SEEDS)
def test_draw_is_a_bijection_of_b(seed):
    """200 000 consecutive b give 200 000 distinct values: the keys of one row are distinct, no tie rule is needed"""
    for a in (0, 9):
        assert np.unique(sm.draw(seed, a, np.arange(200000))).size == 200000


def _within(counts, expect, what):
    counts = np.asarray(counts, np.float64)
    dev = np.abs(counts - expect) / expect
    print(what, counts.min(), counts.max(), "worst %.2f %%" % (100 * dev.max()))
    assert (dev <= 0.05).all(), (what, counts)


@pytest.mark.parametrize("seed", SEEDS)
def test_spread_over_seven_outcomes(seed):
    """70 000 draws (7 000 walkers, 10 steps) over 7 outcomes"""
    w, t = np.meshgrid(np.arange(7000), np.arange(10), indexing="ij")
    c = np.bincount(sm.pick(sm.draw(seed, w.ravel(), t.ravel()), 7), minlength=7)
    _within(c, 10000, ("seven", seed))


@pytest.mark.parametrize("seed", SEEDS)
def test_spread_of_pairs(seed):
    """consecutive steps of one walker, and one step of adjacent walkers, over 3 x 3 outcomes: 90 000 draws each"""
    w, t = np.meshgrid(np.arange(9000), np.arange(10), indexing="ij")
    w, t = w.ravel(), t.ravel()
    here = sm.pick(sm.draw(seed, w, t), 3)
    _within(np.bincount(3 * here + sm.pick(sm.draw(seed, w, t + 1), 3), minlength=9), 10000, ("steps", seed))
    _within(np.bincount(3 * here + sm.pick(sm.draw(seed, w + 1, t), 3), minlength=9), 10000, ("walkers", seed))


@pytest.mark.parametrize("seed", SEEDS)
def test_spread_of_weights(seed):
    """weights 1, 2, 3, 4 over 100 000 draws, by the walk itself: one weighted step from vertex 0 for 100 000 walkers"""
    ptr, ind, val = _csr(5, ([0, 0, 0, 0], [1, 2, 3, 4]), [1, 2, 3, 4])
    r = sm.walk(ptr, ind, val, np.zeros(100000, np.int64), 1, sm.WEIGHTED, seed)
    c = np.bincount(r.walks.reshape(-1, 2)[:, 1], minlength=5)[1:]
    _within(c / np.array([1, 2, 3, 4]), 10000, ("weights", seed))


# ---- the walk ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", (sm.UNIFORM, sm.WEIGHTED))
def test_directed_path_is_forced_then_dead(mode):
    ptr, ind, val = _csr(4, ([0, 1, 2], [1, 2, 3]))
    r = sm.walk(ptr, ind, val, [0, 2, 3], 5, mode, 7)
    assert r.walks.reshape(3, 6).tolist() == [[0, 1, 2, 3, -1, -1], [2, 3, -1, -1, -1, -1], [3, -1, -1, -1, -1, -1]]
    assert (r.walkers, r.steps, r.dead_ends) == (3, 4, 3)
    r = sm.walk(ptr, ind, val, [0], 3, mode, 7)                      # ends ON the dead end: it did not stop early
    assert r.walks.tolist() == [0, 1, 2, 3] and (r.steps, r.dead_ends) == (3, 0)
    r = sm.walk(ptr, ind, val, None, 0, mode, 7)                     # length 0, every vertex
    assert r.walks.tolist() == [0, 1, 2, 3] and (r.walkers, r.steps, r.dead_ends) == (4, 0, 0)


def test_cycle_and_loop():
    ptr, ind, val = _csr(3, ([0, 1, 2], [1, 2, 0]))
    r = sm.walk(ptr, ind, val, [1, 1], 7, sm.UNIFORM, 99)
    assert r.walks.reshape(2, 8).tolist() == [[1, 2, 0, 1, 2, 0, 1, 2]] * 2 and (r.steps, r.dead_ends) == (14, 0)
    ptr, ind, val = _csr(2, ([0], [0]))                               # a diagonal entry is an ordinary step
    assert sm.walk(ptr, ind, val, [0], 3, sm.UNIFORM, 1).walks.tolist() == [0, 0, 0, 0]


def test_one_positive_weight_among_zeros():
    ptr, ind, val = _csr(6, ([0] * 5 + [3], [1, 2, 3, 4, 5, 0]), [0, 0, 9, 0, 0, 1])
    for seed in SEEDS:
        r = sm.walk(ptr, ind, val, [0] * 50, 2, sm.WEIGHTED, seed)
        assert (r.walks.reshape(50, 3) == [0, 3, 0]).all()
    z = np.zeros(6, np.int64)                                        # an all-zero row is a dead end in weighted mode only
    assert sm.walk(ptr, ind, z, [0], 2, sm.WEIGHTED, 1).walks.tolist() == [0, -1, -1]
    assert sm.walk(ptr, ind, z, [0], 2, sm.UNIFORM, 1).walks[1] in (1, 2, 3, 4, 5)


def test_uniform_step_is_pick_of_the_stored_order():
    ptr, ind, val = _csr(8, ([0] * 7, [1, 2, 3, 4, 5, 6, 7]))
    r = sm.walk(ptr, ind, val, [0, 0, 0], 1, sm.UNIFORM, 12345)
    for w in range(3):
        assert r.walks[2 * w + 1] == 1 + (sm.draw(12345, w, 0) * 7 >> 32)


def test_weight_rule():
    ptr, ind, _ = _csr(2, ([0, 0], [0, 1]))
    ok = lambda v: sm.walk(ptr, ind, v, [0], 1, sm.WEIGHTED, 0) is not None
    assert ok(np.array([2.0 ** 24, -0.0], F)) and ok(np.array([0, 5], I))
    for bad in (np.array([-1, 1], I), np.array([0.5, 1], F), np.array([np.nan, 1], F), np.array([np.inf, 1], F), np.array([-3, 1], F),
                np.array([2.0 ** 24 + 2, 1], F)):
        assert not ok(bad)
        assert sm.walk(ptr, ind, bad, [0], 1, sm.UNIFORM, 0) is not None       # the values are never read
    assert ok(np.array([2 ** 31 - 2, 1], I)) and not ok(np.array([2 ** 31 - 1, 1], I))


# ---- the sample ----------------------------------------------------------------------------------------------------------
def test_fanout_at_least_d_copies_the_row():
    ptr, ind, _ = _csr(4, ([0, 0, 0, 2], [1, 2, 3, 0]))
    val = np.array([1.5, -0.0, np.nan, 0.0], F)
    for fanout in (3, 4, 100):
        r = sm.sample(ptr, ind, val, [2, 0, 1, 0], fanout, 5)
        assert r.ptr.tolist() == [0, 1, 4, 4, 7] and r.ind.tolist() == [0, 1, 2, 3, 1, 2, 3]
        assert r.val.view(np.uint32).tolist() == val[[3, 0, 1, 2, 0, 1, 2]].view(np.uint32).tolist()
        assert (r.rows, r.entries, r.full_rows) == (4, 7, 4)


def test_smallest_keys_in_stored_order():
    ptr, ind, val = _csr(12, ([0] * 10, list(range(2, 12))))
    for seed in SEEDS:
        for k_at, fanout in ((0, 1), (1, 3), (2, 9)):
            seeds = [1] * k_at + [0]                                  # the key takes the list position
            r = sm.sample(ptr, ind, val, seeds, fanout, seed)
            keys = [sm.draw(seed, k_at, p) for p in range(10)]
            want = sorted(sorted(range(10), key=lambda p: keys[p])[:fanout])
            assert r.ind[r.ptr[k_at]:].tolist() == [2 + p for p in want] and r.full_rows == k_at
    assert sm.sample(ptr, ind, val, [], 3, 1).ptr.tolist() == [0]
