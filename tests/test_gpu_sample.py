"""Random walks and neighbour sampling on the device (csrc/sample.hip: grb_random_walk, grb_sample_neighbors) against
tests/sample_model.py, the host restatement of the definitions in include/grb_hip.h.  Every comparison is EXACT: every element
of walks, every pointer, column and value bit of C, and walkers / steps / dead_ends, rows / entries / full_rows.  The graphs
are made here with numpy.  Walks: forced graphs, a grid, a star whose hub row is longer than every class, loops, isolated
starts, length 0, one long walk, many short ones, duplicated starts, a null list, two seeds; weighted: every row class of the
prefix pass at its bounds with zeros mixed in, an all-zero row, i32 = f32, -0.0, the row-sum bound, every bad weight, NaN under
uniform mode.  Sampling: every row class at its bounds with fanouts around d, a row of 5 000, empty rows, seeds out of order and
repeated, a rectangular A, value bits, ns = 0, fanout >= the longest row against grb_matrix_extract, the CSC read back, C = A.
Both: the CSR-only format, a product result, caller-owned storage, determinism (also on four CUs in a child process), every
error code with the output unchanged, and the C++ frontend."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import sample_model as sm
from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
PRE_LANE_LEN, PRE_WAVE_LEN = 8, 2048            # kSmLaneLen, kSmWaveLen: the prefix pass (a lane, a wave, the workgroup)
SMP_LANE_LEN, SMP_WAVE_LEN = 8, 512             # kSnLaneLen, kSnWaveLen: sampling
U, W = sm.UNIFORM, sm.WEIGHTED
INT32_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs ------------------------------------------------------------------------------------------------------------
class Csr:
    """nrows x ncols; the entries (r, c, v) in CSR order (columns ascending in a row)"""

    def __init__(self, nrows, ncols, r, c, v=None):
        r, c = np.asarray(r, np.int64).ravel(), np.asarray(c, np.int64).ravel()
        v = np.ones(r.size, np.int64) if v is None else np.asarray(v).ravel()
        assert r.size == c.size == v.size and np.unique(r * max(ncols, 1) + c).size == r.size
        o = np.lexsort((c, r))
        self.nrows, self.ncols, self.rows, self.ind, self.val = nrows, ncols, r[o], c[o], v[o]
        self.ptr = np.zeros(nrows + 1, np.int64)
        if r.size:
            np.cumsum(np.bincount(r, minlength=nrows), out=self.ptr[1:])

    def with_values(self, v):
        return Csr(self.nrows, self.ncols, self.rows, self.ind, np.asarray(v))


def _matrix(g, a, dt=I, csr_only=False, monkeypatch=None):
    if csr_only:
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(a.nrows, a.ncols, dt)
    if csr_only:
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(a.ptr.astype(I), a.ind.astype(I), a.val.astype(dt)) == 0
    return A


def _walk(hb, A, a, starts, length, mode, seed, walks=None, name="", want=None):
    g = hb.g
    want = sm.walk(a.ptr, a.ind, a.val, starts, length, mode, seed) if want is None else want
    ns = a.nrows if starts is None else len(starts)
    if walks is None:
        walks = g.Vector(ns * (length + 1), I)
    info, res = g.random_walk(walks, A, starts, length, mode, seed, None)
    assert info == 0, (name, info)
    print(name, res)
    if ns:
        assert walks.getStorage() == g.GrB_DENSE and walks.nvals() == ns * (length + 1)
        got = walks.extractTuples()[1]
        assert got.dtype == I
        bad = np.flatnonzero(got != want.walks)
        assert bad.size == 0, (name, "walks", bad[:10], got[bad[:10]], want.walks[bad[:10]])
    else:
        got = np.zeros(0, I)
    assert (res["walkers"], res["steps"], res["dead_ends"]) == (want.walkers, want.steps, want.dead_ends), (name, res, want.steps, want.dead_ends)
    assert res["loop_ms"] >= 0 and res["launches"] == (0 if ns == 0 else 2 if mode == W and a.ind.size else 1)
    return got, res


def _csc_of(ptr, ind, val, ncols):
    rows = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    o = np.lexsort((rows, ind))
    cp = np.zeros(ncols + 1, np.int64)
    if ind.size:
        np.cumsum(np.bincount(ind, minlength=ncols), out=cp[1:])
    return cp, rows[o], val[o]


def _same_csr(name, got, want_ptr, want_ind, want_val):
    ptr, ind, val = got
    assert np.array_equal(ptr, want_ptr), (name, "ptr", ptr[:20], want_ptr[:20])
    assert np.array_equal(ind, want_ind), (name, "ind", np.flatnonzero(ind != want_ind)[:10])
    assert np.array_equal(val.view(np.uint32), np.asarray(want_val).view(np.uint32)), (name, "value bits")


def _sample(hb, A, a, seeds, fanout, seed, dt=I, C=None, name="", csc=True):
    g = hb.g
    want = sm.sample(a.ptr, a.ind, a.val.astype(dt), seeds, fanout, seed)
    if C is None:
        C = g.Matrix(len(seeds), a.ncols, dt)
    info, res = g.sample_neighbors(C, A, seeds, fanout, seed, None)
    assert info == 0, (name, info)
    assert (res["rows"], res["entries"], res["full_rows"]) == (want.rows, want.entries, want.full_rows), (name, res)
    assert C.nvals() == want.entries and res["loop_ms"] >= 0
    _same_csr(name, C.host_csr(), want.ptr, want.ind, want.val)
    if csc:                                                # the other orientation, read back
        cp, ci, cv = _csc_of(want.ptr.astype(np.int64), want.ind.astype(np.int64), want.val, a.ncols)
        _same_csr((name, "csc"), C.host_csc(), cp, ci, cv)
    return C, res, want


def _grid(h, w):
    idx = np.arange(h * w).reshape(h, w)
    u = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    v = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    return Csr(h * w, h * w, np.concatenate([u, v]), np.concatenate([v, u]))


# ---- walks, uniform ------------------------------------------------------------------------------------------------------
def test_forced_walks(hb):
    path = Csr(4, 4, [0, 1, 2], [1, 2, 3])
    got, res = _walk(hb, _matrix(hb.g, path), path, [0, 2, 3], 5, U, 7, name="path")
    assert got.reshape(3, 6).tolist() == [[0, 1, 2, 3, -1, -1], [2, 3, -1, -1, -1, -1], [3, -1, -1, -1, -1, -1]]
    assert (res["steps"], res["dead_ends"]) == (4, 3)
    got, res = _walk(hb, _matrix(hb.g, path, F), path, [0], 3, W, 7, name="path, ends on the dead end")
    assert got.tolist() == [0, 1, 2, 3] and res["dead_ends"] == 0
    cyc = Csr(3, 3, [0, 1, 2], [1, 2, 0])
    got, _ = _walk(hb, _matrix(hb.g, cyc), cyc, [1, 1], 7, U, 99, name="cycle")
    assert got.reshape(2, 8).tolist() == [[1, 2, 0, 1, 2, 0, 1, 2]] * 2


def test_grid_loops_isolated_starts_and_length_zero(hb):
    gr = _grid(20, 21)
    n = gr.nrows
    # loops on every third vertex, and ten isolated vertices behind the grid
    loops = np.arange(0, n, 3)
    a = Csr(n + 10, n + 10, np.concatenate([gr.rows, loops]), np.concatenate([gr.ind, loops]))
    A = _matrix(hb.g, a)
    _walk(hb, A, a, None, 12, U, 1, name="grid, every vertex")
    got, res = _walk(hb, A, a, [n, n + 9, 5, n + 3], 4, U, 1, name="isolated starts")
    assert res["dead_ends"] == 3 and (got.reshape(4, 5)[[0, 1, 3], 1:] == -1).all()
    got, res = _walk(hb, A, a, [3, 3, n + 1], 0, U, 1, name="length 0")
    assert got.tolist() == [3, 3, n + 1] and (res["steps"], res["dead_ends"]) == (0, 0)
    assert (_walk(hb, A, a, [7], 50, U, 1)[0] != _walk(hb, A, a, [7], 50, U, 2)[0]).any()       # two seeds
    for seed in (0, 0xffffffff):
        _walk(hb, A, a, None, 3, U, seed, name=("seed", seed))


def test_star_from_the_hub_and_from_the_leaves(hb):
    leaves = PRE_WAVE_LEN + 60                               # the hub row is longer than every class of either pass
    a = Csr(leaves + 1, leaves + 1, np.concatenate([np.zeros(leaves, np.int64), 1 + np.arange(leaves)]),
            np.concatenate([1 + np.arange(leaves), np.zeros(leaves, np.int64)]))
    A = _matrix(hb.g, a)
    got, _ = _walk(hb, A, a, [0] * 3000, 3, U, 5, name="from the hub")
    assert np.unique(got.reshape(3000, 4)[:, 1]).size > 1000
    _walk(hb, A, a, 1 + np.arange(leaves), 4, U, 5, name="from the leaves")
    _walk(hb, A, a, None, 2, W, 5, name="weighted, the hub's prefix by the workgroup")


def test_one_long_walk_many_short_ones_and_duplicates(hb):
    a = _grid(30, 30)
    A = _matrix(hb.g, a)
    got, res = _walk(hb, A, a, [17], 10000, U, 3, name="one walker, 10 000 steps")
    assert res["steps"] == 10000 and np.unique(got).size > 100
    rng = np.random.default_rng(1)
    _walk(hb, A, a, rng.integers(0, a.nrows, 50000), 3, U, 4, name="50 000 walkers")
    got, _ = _walk(hb, A, a, [40] * 8, 20, U, 4, name="duplicated starts")
    rows = got.reshape(8, 21)
    assert all((rows[i] != rows[j]).any() for i in range(8) for j in range(i))


# ---- walks, weighted -----------------------------------------------------------------------------------------------------
def _class_graph(rng):
    """hubs 0 .. 5 with rows of PRE_LANE_LEN - 1 .. PRE_WAVE_LEN + 1 entries (columns 0 .. len - 1: the hubs reach each other
    and themselves), every other vertex with two or three entries back to the hubs; weights 0 .. 5, zeros mixed in; the last
    vertex's row is all zeros: a dead end in weighted mode only"""
    lens = [PRE_LANE_LEN - 1, PRE_LANE_LEN, PRE_LANE_LEN + 1, PRE_WAVE_LEN - 1, PRE_WAVE_LEN, PRE_WAVE_LEN + 1]
    n = PRE_WAVE_LEN + 40
    r = [np.full(d, h) for h, d in enumerate(lens)]
    c = [np.arange(d) for d in lens]
    rest = np.arange(6, n)
    r += [rest, rest, rest[::2]]
    c += [rest % 6, 6 + (rest * 7) % (n - 6), (rest[::2] + 1) % 6]
    r, c = np.concatenate(r), np.concatenate(c)
    key = np.unique(r * n + c)
    r, c = key // n, key % n
    w = rng.integers(0, 6, r.size)
    w[r == n - 1] = 0
    return Csr(n, n, r, c, w), lens


def test_weighted_every_class_of_the_prefix_pass(hb):
    rng = np.random.default_rng(2)
    a, lens = _class_graph(rng)
    assert np.diff(a.ptr)[:6].tolist() == lens and (a.val == 0).sum() > 100
    got_i, res = _walk(hb, _matrix(hb.g, a, I), a, None, 6, W, 21, name="classes, i32")
    assert res["dead_ends"] > 0 and got_i.reshape(a.nrows, 7)[a.nrows - 1].tolist() == [a.nrows - 1] + [-1] * 6
    hubs = np.bincount(got_i[got_i >= 0], minlength=a.nrows)[:6]
    assert (hubs > 100).all(), hubs                        # every class is searched many times
    fv = a.val.astype(F)
    fv[np.flatnonzero(fv == 0)[::2]] = -0.0                 # -0.0 is +0.0
    af = a.with_values(fv)
    want = sm.walk(a.ptr, a.ind, a.val, None, 6, W, 21)
    got_f, _ = _walk(hb, _matrix(hb.g, af, F), af, None, 6, W, 21, name="classes, f32 with -0.0", want=want)
    assert np.array_equal(got_f, got_i)
    _walk(hb, _matrix(hb.g, a, I), a, [0, 1, 2, 3, 4, 5] * 500, 2, W, 22, name="from the hubs")
    # the same structure under uniform mode takes the zero-weight entries too, and the last vertex is no dead end
    got_u, res_u = _walk(hb, _matrix(hb.g, a, I), a, None, 6, U, 21, name="classes, uniform")
    assert res_u["dead_ends"] == 0 and (got_u != got_i).any()


@pytest.mark.parametrize("d", (3, 100, PRE_WAVE_LEN + 1))
def test_row_sum_bound(hb, d):
    """a row sum of exactly 2^31 - 1 is accepted, 2^31 is refused: by a lane, a wave and the workgroup"""
    g = hb.g
    base = INT32_MAX // d
    w = np.full(d, base, np.int64)
    w[-1] += INT32_MAX - base * d
    assert w.sum() == INT32_MAX
    a = Csr(d + 1, d + 1, np.zeros(d, np.int64), 1 + np.arange(d), w)
    _walk(hb, _matrix(g, a), a, [0] * 200, 1, W, 8, name=("row sum 2^31 - 1", d))
    w[d // 2] += 1
    b = a.with_values(w)
    walks = g.Vector(8, I)
    assert walks.build(np.arange(8, dtype=I) + 50, 8) == 0
    info, _ = g.random_walk(walks, _matrix(g, b), [0] * 4, 1, W, 8, None)
    assert info == g.GrB_INVALID_VALUE and walks.extractTuples()[1].tolist() == list(range(50, 58))
    _walk(hb, _matrix(g, b), b, [0] * 4, 1, U, 8, name="uniform never reads it")


def test_bad_weights_and_nan_under_uniform_mode(hb):
    g = hb.g
    a = _grid(6, 7)
    before = np.arange(3 * 5, dtype=I) + 9
    walks = g.Vector(15, I)
    assert walks.build(before, 15) == 0
    sv = g.Vector(15, I)                                     # a sparse walks stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0
    for dt, x in ((I, -1), (F, -3.0), (F, 0.5), (F, np.nan), (F, np.inf), (F, 2.0 ** 24 + 2)):
        for at in (0, a.ind.size - 1, 37):
            v = a.val.astype(dt)
            v[at] = x
            M = _matrix(g, a.with_values(v), dt)
            for out in (walks, sv):
                info, _ = g.random_walk(out, M, [0, 5, 41], 4, W, 3, None)
                assert info == g.GrB_INVALID_VALUE, (dt, x, at)
        assert np.array_equal(walks.extractTuples()[1], before) and walks.getStorage() == g.GrB_DENSE
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
    v = a.val.astype(F)
    v[5] = 2.0 ** 24                                        # exactly 2^24 is allowed
    b = a.with_values(v)
    _walk(hb, _matrix(g, b, F), b, None, 5, W, 3, name="2^24")
    nan = a.with_values(np.full(a.ind.size, np.nan, F))
    _walk(hb, _matrix(g, nan, F), nan, None, 9, U, 3, name="uniform on NaN")


# ---- sampling ------------------------------------------------------------------------------------------------------------
def _sample_graph(rng, dt):
    """a rectangular A: rows at the bounds of every class, a row of 5 000, empty rows, a few short ones"""
    lens = [SMP_LANE_LEN - 1, SMP_LANE_LEN, SMP_LANE_LEN + 1, 0, SMP_WAVE_LEN - 1, SMP_WAVE_LEN, SMP_WAVE_LEN + 1, 5000, 0, 1, 2, 30, 64, 65]
    ncols = 7000
    r = np.concatenate([np.full(d, k) for k, d in enumerate(lens)])
    c = np.concatenate([np.sort(rng.choice(ncols, d, replace=False)) for d in lens])
    if dt is F:
        v = rng.standard_normal(r.size).astype(F)
        v[::5] = 0.0
        v[1::7] = -0.0
        v[2::11] = np.nan
        v[3::13] = np.float32(np.uint32(0x7fc00123).view(F))        # a NaN with a payload
    else:
        v = rng.integers(-5, 6, r.size)
    return Csr(len(lens), ncols, r, c, v), lens


@pytest.mark.parametrize("dt", (F, I))
def test_sample_every_class_and_fanout(hb, dt):
    rng = np.random.default_rng(3)
    a, lens = _sample_graph(rng, dt)
    A = _matrix(hb.g, a, dt)
    seeds = np.arange(a.nrows)
    fanouts = sorted({f for d in lens if d > 2 for f in (1, 2, d - 1, d, d + 1)} | {10})
    assert {1, 2, 10, 4999, 5000, 5001, SMP_WAVE_LEN, SMP_LANE_LEN} <= set(fanouts)
    for fanout in fanouts:
        _, res, want = _sample(hb, A, a, seeds, fanout, 17, dt, name=("classes", fanout))
        assert np.array_equal(np.diff(want.ptr), np.minimum(lens, fanout))
        assert all(np.all(np.diff(want.ind[want.ptr[k]:want.ptr[k + 1]]) > 0) for k in range(a.nrows))
    assert res["launches"] == 5


def test_seeds_out_of_order_and_repeated(hb):
    rng = np.random.default_rng(4)
    a, lens = _sample_graph(rng, I)
    A = _matrix(hb.g, a)
    seeds = [7, 0, 7, 5, 3, 5, 11, 7, 2, 11, 10, 2, 13, 13, 10]
    differ = {7: False, 5: False, 2: False, 13: False}
    for seed in (1, 2, 3, 4, 5):
        C, _, want = _sample(hb, A, a, seeds, 6, seed, name=("repeats", seed))
        for row in differ:
            first, second = [k for k, s in enumerate(seeds) if s == row][:2]
            differ[row] |= want.ind[want.ptr[first]:want.ptr[first + 1]].tolist() != want.ind[want.ptr[second]:want.ptr[second + 1]].tolist()
        assert want.ind[want.ptr[10]:want.ptr[11]].tolist() == want.ind[want.ptr[14]:want.ptr[15]].tolist()   # row 10: d = 2 <= fanout
    assert all(differ.values()), differ


def test_ns_zero_and_all_rows_empty(hb):
    g = hb.g
    rng = np.random.default_rng(5)
    a, _ = _sample_graph(rng, F)
    A = _matrix(g, a, F)
    C, res, _ = _sample(hb, A, a, [], 4, 1, F, name="ns = 0")
    assert (C.nrows(), C.ncols(), C.nvals(), res["rows"]) == (0, a.ncols, 0, 0)
    C, res, _ = _sample(hb, A, a, [3, 8, 3], 4, 1, F, name="empty rows only")
    assert res["entries"] == 0 and res["full_rows"] == 3


def test_fanout_at_least_the_longest_row_is_extract(hb):
    g = hb.g
    rng = np.random.default_rng(6)
    a, lens = _sample_graph(rng, F)
    A = _matrix(g, a, F)
    seeds = [13, 7, 0, 7, 4, 3, 12]
    C, res, _ = _sample(hb, A, a, seeds, max(lens), 9, F, name="whole rows")
    assert res["full_rows"] == len(seeds)
    X = g.Matrix(len(seeds), a.ncols, F)
    assert g.extract(X, None, None, A, seeds, None, hb.descriptor()) == 0
    _same_csr("extract", C.host_csr(), *X.host_csr())
    _same_csr("extract, csc", C.host_csc(), *X.host_csc())


def test_c_is_a(hb):
    g = hb.g
    rng = np.random.default_rng(7)
    n = 700
    lens = rng.integers(0, 40, n)
    lens[[5, 77]] = [600, SMP_WAVE_LEN + 1]
    r = np.concatenate([np.full(d, k) for k, d in enumerate(lens)])
    c = np.concatenate([np.sort(rng.choice(n, d, replace=False)) for d in lens])
    a = Csr(n, n, r, c, rng.integers(1, 100, r.size))
    A = _matrix(g, a)
    seeds = rng.permutation(n)
    _sample(hb, A, a, seeds, 5, 31, C=A, name="C = A")
    assert A.nrows() == n and A.nvals() == int(np.minimum(lens, 5).sum())


# ---- both: formats, storage, determinism -----------------------------------------------------------------------------------
def test_csr_only_product_and_adopted(hb, monkeypatch):
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(8)
    a, _ = _class_graph(rng)
    n = a.nrows
    seeds = [3, 0, 5, 4, 100, 3, n - 1]
    for dt in (I, F):
        A1 = _matrix(g, a, dt, csr_only=True, monkeypatch=monkeypatch)
        _walk(hb, A1, a, None, 4, W, 5, name=("CSR only", dt))
        _walk(hb, A1, a, None, 4, U, 5, name=("CSR only, uniform", dt))
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
        C1 = g.Matrix(len(seeds), n, dt)
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
        _sample(hb, A1, a, seeds, 7, 5, dt, C=C1, name=("CSR only", dt), csc=False)
        _sample(hb, A1, a, seeds, 7, 5, dt, name=("CSR-only A, a C with both", dt))
    # a product result: S * S of a 0/1 structure has small integer values; no CSC of its own
    s = _grid(12, 13)
    S = _matrix(g, s, F)
    P = g.Matrix(s.nrows, s.nrows, F)
    assert g.mxm(P, None, None, "PlusMultiplies", S, S, hb.descriptor()) == 0
    pp, pi, pv = P.host_csr()
    p = Csr(s.nrows, s.nrows, np.repeat(np.arange(s.nrows), np.diff(pp)), pi, pv.astype(np.int64))
    assert p.ind.size > s.ind.size and (pv == np.round(pv)).all() and pv.max() > 1
    _walk(hb, P, p, None, 8, W, 6, name="product result")
    _walk(hb, P, p, None, 8, U, 6, name="product result, uniform")
    _sample(hb, P, p, np.arange(s.nrows)[::-1], 3, 6, F, name="product result")
    # caller-owned storage: A's arrays and walks at every 4-byte offset past a 16-byte boundary (the quads of the prefix pass)
    ptr, ind, val = a.ptr.astype(I), a.ind.astype(I), a.val.astype(I)
    want = sm.walk(a.ptr, a.ind, a.val, None, 3, W, 9)
    for k in ad.KS:
        ks = (k, (k + 1) % 4, (k + 2) % 4)
        Aad, checks = ad.adopt_csr(g, (n, n), I, ptr, ind, val, ks)
        out, t, check = ad.adopt_dense(g, np.full(n * 4, 77, I), (k + 3) % 4)
        got, _ = _walk(hb, Aad, a, None, 3, W, 9, walks=out, name=("adopted", k), want=want)
        assert np.array_equal(ad.payload(t, (k + 3) % 4, n * 4, I), got)
        check(("walks", k))
        _sample(hb, Aad, a, seeds, 7, 5, name=("adopted", k))
        for c in checks:
            c(("A", k))


CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import graphblast_amd as g
d = np.load(sys.argv[2])
ptr, ind, val, seeds = d["ptr"], d["ind"], d["val"], d["seeds"]
n = ptr.size - 1
A = g.Matrix(n, n, val.dtype.type)
assert A.build_csr(ptr, ind, val) == 0
out = {}
for mode in (0, 1):
    w = g.Vector(n * 6, np.int32)
    info, res = g.random_walk(w, A, None, 5, mode, 77, None)
    assert info == 0, (info, res)
    out["walks%d" % mode] = w.extractTuples()[1]
    out["rec%d" % mode] = np.array([res["walkers"], res["steps"], res["dead_ends"]], np.int64)
C = g.Matrix(seeds.size, n, val.dtype.type)
info, res = g.sample_neighbors(C, A, seeds, 6, 77, None)
assert info == 0, (info, res)
out["cptr"], out["cind"], out["cval"] = C.host_csr()
out["crec"] = np.array([res["rows"], res["entries"], res["full_rows"]], np.int64)
np.savez(sys.argv[3], **out)
"""


def test_two_runs_and_a_child_on_four_cus_give_the_same_bits(hb, tmp_path):
    g = hb.g
    rng = np.random.default_rng(9)
    a, _ = _class_graph(rng)
    n = a.nrows
    A = _matrix(g, a)
    seeds = rng.integers(0, n, 300)
    seeds[:6] = np.arange(6)
    runs = []
    for _ in range(2):
        out = {}
        for mode in (U, W):
            got, res = _walk(hb, A, a, None, 5, mode, 77, name="determinism")
            out["walks%d" % mode] = got.tobytes()
            out["rec%d" % mode] = [res["walkers"], res["steps"], res["dead_ends"]]
        C, res, _ = _sample(hb, A, a, seeds, 6, 77, name="determinism")
        cp, ci, cv = C.host_csr()
        out.update(cptr=cp.tobytes(), cind=ci.tobytes(), cval=cv.tobytes(), crec=[res["rows"], res["entries"], res["full_rows"]])
        runs.append(out)
    assert runs[0] == runs[1]
    np.savez(tmp_path / "in.npz", ptr=a.ptr.astype(I), ind=a.ind.astype(I), val=a.val.astype(I), seeds=seeds.astype(I))
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                       env=dict(os.environ, GRB_NUM_CU="4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    for key, want in runs[0].items():
        assert (out[key].tolist() if key.endswith(("rec0", "rec1", "crec")) else out[key].tobytes()) == want, key


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_walk_errors_leave_walks_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    a = _grid(5, 6)
    n = a.nrows
    A = _matrix(g, a)
    ptr, ind, val = a.ptr.astype(I), a.ind.astype(I), a.val.astype(I)
    before = (np.arange(12) + 100).astype(I)
    walks = g.Vector(12, I)
    assert walks.build(before, 12) == 0
    starts = np.array([0, 5, 29], I)

    def call(w_, a_, s_=starts, ns=3, length=3, mode=0):
        return lib.grb_random_walk(w_, a_, None if s_ is None else s_.ctypes.data, ns, length, mode, 1, None, None)

    assert call(walks._h, A._h) == 0                                                   # the call itself is fine
    assert walks.build(before, 12) == 0
    assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT
    assert call(walks._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(walks._h, g.Matrix(n, n, I)._h) == g.GrB_UNINITIALIZED_OBJECT          # an unbuilt A
    R = g.Matrix(n, n + 1, I)                                                          # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(walks._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Vector(13, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH                  # size(walks) != ns * (length + 1)
    assert call(walks._h, A._h, length=2) == g.GrB_DIMENSION_MISMATCH
    assert call(walks._h, A._h, s_=None, ns=3) == g.GrB_DIMENSION_MISMATCH             # a null list: ns is ignored, n walkers
    for bad in (-1, n, 2 ** 31 - 1):
        assert call(walks._h, A._h, s_=np.array([0, bad, 1], I)) == g.GrB_INVALID_INDEX, bad
    assert call(walks._h, A._h, ns=-1) == g.GrB_INVALID_VALUE
    assert call(walks._h, A._h, length=-1) == g.GrB_INVALID_VALUE
    for mode in (2, -1):
        assert call(walks._h, A._h, mode=mode) == g.GrB_INVALID_VALUE
    assert call(walks._h, A._h, s_=None, length=2 ** 27) == g.GrB_INVALID_VALUE       # ns * (length + 1) > INT32_MAX
    assert call(walks._h, A._h, length=INT32_MAX) == g.GrB_INVALID_VALUE
    fv = g.Vector(12, F)                                                               # walks not i32
    fbefore = np.arange(12).astype(F) + 2
    assert fv.build(fbefore, 12) == 0
    assert call(fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(fv.extractTuples()[1], fbefore)
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                           # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(walks._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    assert walks.getStorage() == g.GrB_DENSE and np.array_equal(walks.extractTuples()[1], before)
    # ns = 0 is a success; a descriptor and a null descriptor give the same walks; the record is optional
    info, res = g.random_walk(g.Vector(0, I), A, [], 3, U, 1, None)
    assert info == 0 and (res["walkers"], res["steps"], res["dead_ends"]) == (0, 0, 0)
    w1, w2 = g.Vector(12, I), g.Vector(12, I)
    assert g.random_walk(w1, A, starts, 3, U, 1, hb.descriptor())[0] == 0 and call(w2._h, A._h) == 0
    assert np.array_equal(w1.extractTuples()[1], w2.extractTuples()[1])


def test_sample_errors_leave_c_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(10)
    a, lens = _sample_graph(rng, I)
    A = _matrix(g, a)
    ptr, ind, val = a.ptr.astype(I), a.ind.astype(I), a.val.astype(I)
    seeds = np.array([7, 0, 2], I)
    C, _, _ = _sample(hb, A, a, seeds, 4, 1, name="before")
    before = C.host_csr(), C.host_csc()

    def call(c_, a_, s_=seeds, ns=3, fanout=4):
        return lib.grb_sample_neighbors(c_, a_, None if s_ is None else s_.ctypes.data, ns, fanout, 1, None, None)

    assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT
    assert call(C._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(C._h, g.Matrix(a.nrows, a.ncols, I)._h) == g.GrB_UNINITIALIZED_OBJECT
    assert call(C._h, A._h, s_=None) == g.GrB_NULL_POINTER                             # a null list with ns > 0
    assert call(g.Matrix(4, a.ncols, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Matrix(3, a.ncols + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert call(C._h, A._h, ns=2) == g.GrB_DIMENSION_MISMATCH
    for bad in (-1, a.nrows, 2 ** 31 - 1):
        assert call(C._h, A._h, s_=np.array([0, bad, 1], I)) == g.GrB_INDEX_OUT_OF_BOUNDS, bad
    for fanout in (0, -3):
        assert call(C._h, A._h, fanout=fanout) == g.GrB_INVALID_VALUE
    assert call(C._h, A._h, ns=-1) == g.GrB_INVALID_VALUE
    assert call(g.Matrix(3, a.ncols, F)._h, A._h) == g.GrB_NOT_IMPLEMENTED             # C of another type
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, a.nrows, a.ncols) == 0               # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(C._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    # more than INT32_MAX entries: 430 000 times the row of 5 000, whole
    many = np.full(430000, 7, I)
    big = g.Matrix(many.size, a.ncols, I)
    assert call(big._h, A._h, s_=many, ns=many.size, fanout=5000) == g.GrB_OUT_OF_MEMORY
    for got, want in zip((C.host_csr(), C.host_csc()), before):
        _same_csr("unchanged", got, *want)
    # a descriptor and a null descriptor give the same C
    C2 = g.Matrix(3, a.ncols, I)
    assert g.sample_neighbors(C2, A, seeds, 4, 1, hb.descriptor())[0] == 0
    _same_csr("descriptor", C2.host_csr(), *before[0])


# ---- the C++ frontend ------------------------------------------------------------------------------------------------------
def _read_pattern_mtx(path):
    with open(path) as f:
        lines = [ln for ln in f if not ln.startswith("%")]
    n = int(lines[0].split()[0])
    e = np.array([[int(x) for x in ln.split()[:2]] for ln in lines[1:] if ln.strip()], np.int64) - 1
    return n, e[:, 0], e[:, 1]


def test_cpp_frontend(tmp_path):
    """tests/tools/sample.cpp on chesapeake.mtx: the walks, C's tuples and the records"""
    exe = str(tmp_path / "sample")
    subprocess.run(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "sample.cpp"),
                    "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip", "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe],
                   check=True, timeout=300)
    path = os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    n, u, v = _read_pattern_mtx(path)
    keep = u != v
    key = np.unique(np.concatenate([u[keep] * n + v[keep], v[keep] * n + u[keep]]))
    rr, cc = key // n, key % n
    a = Csr(n, n, rr, cc, 1 + (rr + cc) % 3)
    assert lines[-1] == "ok"
    uw = sm.walk(a.ptr, a.ind, a.val, None, 6, U, 11)
    ww = sm.walk(a.ptr, a.ind, a.val, [n - 1, 0, 0, 3], 9, W, 12)
    for tag, want in (("uniform", uw), ("weighted", ww)):
        assert ("%s walkers %d steps %d dead %d | " % (tag, want.walkers, want.steps, want.dead_ends)) + " ".join(map(str, want.walks.tolist())) in lines
    s = sm.sample(a.ptr, a.ind, a.val, [n - 1, 0, 0, 5, 2], 3, 13)
    assert "sample rows %d entries %d full %d | %s | %s | %s" % (s.rows, s.entries, s.full_rows, " ".join(map(str, s.ptr.tolist())),
                                                                  " ".join(map(str, s.ind.tolist())), " ".join(map(str, s.val.tolist()))) in lines
