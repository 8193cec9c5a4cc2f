"""Community detection by label propagation on the device (csrc/cdlp.hip) against a numpy restatement of the definition in
include/grb_hip.h: the (vertex, neighbour's label) pairs of the multiset N(v), np.unique with counts, a lexsort by (vertex,
-count, label) whose first entry per vertex is the new label, and the changed mask carried along for `evaluated`.  Every
comparison is exact: the labels (i32, dense, all n stored), iterations, changed, evaluated and communities, with the
skipping of unchanged neighbourhoods on and off.  Random undirected and directed graphs in both element types with values
that must not matter, reciprocal edges, oscillation, an early stop, rows around every size threshold of the evaluation
kernels under crafted labels, more long rows than count arrays, degenerate shapes, a product result, the CSR-only format,
every error code with the labels unchanged, determinism and the C++ frontend."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
# csrc/cdlp.hip: a vertex's list is its CSR row (directed: followed by its CSC column), the diagonal included in the length
TINY_LEN = 8         # kCdTinyLen: a list of up to this many entries is evaluated by eight lanes, a longer one by a wave
WAVE_LEN = 64        # kCdWaveLen: ... by a wave, a longer one by a workgroup with the LDS hash table
SMALL_LEN = 512      # kCdSmallLen: ... by one wave with an LDS hash table of 1024 (label, count) pairs, a longer one by four waves
BLOCK_LEN = 2048     # kCdBlockLen: ... with the large LDS table, a longer one by a count array of n words in global memory
SLOTS = 4096         # kCdSlots: (label, count) pairs of the large LDS table
POOL = 256           # kCdPoolMax: the most count arrays, i.e. long lists evaluated at the same time (a small n gets them all)
TILE = 2048          # kCdTile: vertices one workgroup of the work lists' compaction takes


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs and the reference ------------------------------------------------------------------------------------------
def _pattern(n, r, c):
    """the 0 / 1 pattern of the entries (r, c), duplicates merged, columns ascending; the diagonal stays if given"""
    S = sp.csr_matrix((np.ones(len(r), np.int64), (np.asarray(r, np.int64), np.asarray(c, np.int64))), shape=(n, n))
    S.data[:] = 1
    S.sort_indices()
    return S


def _sym(n, r, c, diag=None):
    """the undirected graph of the draws: loops dropped, both directions; diag: rows that also store their diagonal"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    r, c = r[keep], c[keep]
    d = np.zeros(0, np.int64) if diag is None else np.asarray(diag, np.int64)
    return _pattern(n, np.concatenate([r, c, d]), np.concatenate([c, r, d]))


def _pairs(S, directed):
    """(v, u) for every u of the multiset N(v)"""
    n = S.shape[0]
    v = np.repeat(np.arange(n, dtype=np.int64), np.diff(S.indptr))
    u = S.indices.astype(np.int64)
    if directed:
        T = sp.csc_matrix(S)
        T.sort_indices()
        v = np.concatenate([v, np.repeat(np.arange(n, dtype=np.int64), np.diff(T.indptr))])
        u = np.concatenate([u, T.indices.astype(np.int64)])
    keep = v != u
    return v[keep], u[keep]


def _ref(S, directed=False, init=None, max_iter=10):
    """-> labels, dict(iterations, changed, evaluated, communities), the vertices with a non-empty N(v), changed per iteration"""
    n = S.shape[0]
    v, u = _pairs(S, directed)
    lab = np.arange(n, dtype=np.int64) if init is None else np.asarray(init, np.int64).copy()
    some = np.zeros(n, bool)
    some[v] = True
    changed = np.ones(n, bool)
    evaluated, history = 0, []
    it = 0
    while it < max_iter:
        it += 1
        if it == 1:
            evaluated += int(some.sum())
        else:
            ev = np.zeros(n, bool)
            ev[v[changed[u]]] = True
            evaluated += int(ev.sum())
        new = lab.copy()
        if v.size:
            key, cnt = np.unique(v * n + lab[u], return_counts=True)
            row, label = key // n, key % n
            order = np.lexsort((label, -cnt, row))
            row, label = row[order], label[order]
            first = np.concatenate([[True], row[1:] != row[:-1]])
            new[row[first]] = label[first]
        changed = new != lab
        lab = new
        history.append(int(changed.sum()))
        if not changed.any():
            break
    rec = dict(iterations=it, changed=history[-1], evaluated=evaluated, communities=int(np.unique(lab).size))
    return lab.astype(I), rec, int(some.sum()), history


def _matrix(g, S, dt=F, rng=None):
    """A with S's structure; values that must not matter (zeros and negatives among them)"""
    n = S.shape[0]
    vals = np.ones(S.nnz, dt) if rng is None else rng.integers(-3, 4, S.nnz).astype(dt)
    A = g.Matrix(n, n, dt)
    assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), vals) == 0
    return A


def _vector(g, n, values, sparse=False):
    v = g.Vector(n, I)
    if sparse:
        assert v.build(np.arange(n, dtype=I), np.asarray(values, I), n, None) == 0
    else:
        assert v.build(np.asarray(values, I), n) == 0
    return v


def _labels(g, v, n):
    assert v.getStorage() == g.GrB_DENSE and v.nvals() == n and v.np_dtype == I
    info, vals = v.extractTuples()
    assert info == 0 and vals.dtype == I
    return vals


def _check(hb, S, A=None, directed=False, init=None, max_iter=10, name="", sparse_init=False, want=None):
    """cdlp on S's graph against the reference, with the skipping on and then off; -> (labels, the record, the reference's
    changed counts)"""
    g = hb.g
    n = S.shape[0]
    if A is None:
        A = _matrix(g, S)
    lab, rec, some, history = _ref(S, directed, init, max_iter) if want is None else want
    was = g.cdlp_set_skip(1)
    try:
        out = None
        for skip in (1, 0):
            assert g.cdlp_set_skip(skip) == (was if skip == 1 else 1)
            v = g.Vector(n, I)
            iv = None if init is None else _vector(g, n, init, sparse_init)
            info, res = g.cdlp(v, A, None, iv, directed, max_iter)
            assert info == 0, (name, skip, info)
            got = _labels(g, v, n)
            print(name, "skip", skip, {k: res[k] for k in ("iterations", "changed", "evaluated", "communities")}, rec, some)
            assert np.array_equal(got, lab), (name, skip, np.flatnonzero(got != lab)[:10], got[got != lab][:10], lab[got != lab][:10])
            for k in ("iterations", "changed", "communities"):
                assert res[k] == rec[k], (name, skip, k, res, rec)
            assert res["evaluated"] == (rec["evaluated"] if skip else rec["iterations"] * some), (name, skip, res, rec, some)
            assert res["loop_ms"] >= 0
            if skip:
                out = (got, res, history)
        return out
    finally:
        g.cdlp_set_skip(was)


# ---- random graphs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("n, draws", [(2000, 8000), (20000, 200000)])
def test_random_undirected(hb, dt, n, draws):
    """values with zeros and negatives, a tenth of the rows store their diagonal; the changed counts fall from (nearly) n to
    0: dense and nearly empty work lists"""
    rng = np.random.default_rng(7)
    diag = np.sort(rng.choice(n, n // 10, replace=False))
    S = _sym(n, rng.integers(0, n, draws), rng.integers(0, n, draws), diag)
    _, res, history = _check(hb, S, _matrix(hb.g, S, dt, rng), max_iter=30, name=("random", n, dt.__name__))
    assert 3 <= res["iterations"] < 30 and res["changed"] == 0, res
    assert history[0] > n // 2 and 0 < min(h for h in history if h) < n // 100, history


def test_random_directed(hb):
    """directed = 1 against the reference on CSR + CSC, directed = 0 on the same A against its rows only; the two differ"""
    rng = np.random.default_rng(8)
    n, draws = 3000, 20000
    r, c = rng.integers(0, n, draws), rng.integers(0, n, draws)
    S = _pattern(n, r, c)                                  # (some draws are diagonal entries)
    assert (S != S.T).nnz > 0
    A = _matrix(hb.g, S, F, rng)
    both, _, _ = _check(hb, S, A, directed=True, max_iter=30, name="directed")
    rows, _, _ = _check(hb, S, A, directed=False, max_iter=30, name="rows only")
    assert not np.array_equal(both, rows)
    # ... and from labels of the caller's, in either storage
    init = rng.integers(0, n, n)
    for sparse in (False, True):
        _check(hb, S, A, directed=True, init=init, max_iter=4, name=("directed, init", sparse), sparse_init=sparse)


def test_reciprocal_edges_count_twice(hb):
    S = _pattern(4, [0, 0, 3], [1, 3, 0])
    A = _matrix(hb.g, S, I)
    got, _, _ = _check(hb, S, A, directed=True, max_iter=1, name="reciprocal")
    assert got.tolist() == [3, 0, 2, 0]
    got, _, _ = _check(hb, S, A, directed=False, max_iter=1, name="reciprocal, rows")
    assert got.tolist() == [1, 1, 2, 0]


# ---- oscillation and the early stop ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter, want", [(4, [0, 1]), (5, [1, 0])])
def test_single_edge_oscillates(hb, max_iter, want):
    S = _sym(2, [0], [1])
    got, res, _ = _check(hb, S, max_iter=max_iter, name=("edge", max_iter))
    assert got.tolist() == want and res["iterations"] == max_iter and res["changed"] == 2


def test_path_never_settles(hb):
    n = 3000
    S = _sym(n, np.arange(n - 1), np.arange(1, n))
    _, res, history = _check(hb, S, max_iter=50, name="path")
    assert res["iterations"] == 50 and res["changed"] > 0 and min(history) > 0, (res, history[-5:])


@pytest.fixture(scope="module")
def planted():
    """64 blocks of 64 vertices, complete inside, 300 random edges across"""
    rng = np.random.default_rng(9)
    b, m = 64, 64
    x, y = np.triu_indices(m, 1)
    r = np.concatenate([k * m + x for k in range(b)] + [rng.integers(0, b * m, 300)])
    c = np.concatenate([k * m + y for k in range(b)] + [rng.integers(0, b * m, 300)])
    S = _sym(b * m, r, c)
    return S, _ref(S, False, None, 30)


def test_early_stop(hb, planted):
    S, want = planted
    g = hb.g
    n = S.shape[0]
    lab, rec, _, history = want
    assert 3 <= rec["iterations"] < 30 and rec["changed"] == 0 and rec["communities"] <= 64 + 8, rec
    A = _matrix(g, S)
    got, res, _ = _check(hb, S, A, max_iter=30, name="planted", want=want)
    assert res["iterations"] == rec["iterations"] and res["changed"] == 0
    _, res, _ = _check(hb, S, A, max_iter=rec["iterations"] - 1, name="planted, one less")
    assert res["changed"] == history[-2] > 0
    # from the result: one iteration that changes nothing
    again, res, _ = _check(hb, S, A, init=lab, max_iter=1, name="planted, again")
    assert np.array_equal(again, lab) and res["changed"] == 0 and res["iterations"] == 1
    # labels aliasing init, from labels that are not yet settled, in either storage of init
    start, _, _, _ = _ref(S, False, None, 1)
    sep, _, _ = _check(hb, S, A, init=start, max_iter=30, name="planted, from iteration 1")
    assert np.array_equal(sep, lab)
    for sparse in (False, True):
        v = _vector(g, n, start, sparse)
        info, res = g.cdlp(v, A, None, v, False, 30)
        assert info == 0 and res["iterations"] == rec["iterations"] - 1
        assert _labels(g, v, n).tobytes() == sep.tobytes()


# ---- crafted rows ------------------------------------------------------------------------------------------------------
LENGTHS = [1, 2, TINY_LEN - 1, TINY_LEN, TINY_LEN + 1, WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1, SMALL_LEN - 1, SMALL_LEN,
           SMALL_LEN + 1, BLOCK_LEN - 1, BLOCK_LEN, BLOCK_LEN + 1, 2 * SLOTS + 5]


def _crafted_inits(n, hub, leaves):
    """label patterns over the hub's list (the leaves in ascending order, as the row stores them) -> {name: (init, the hub's
    new label or None where only the reference says)}"""
    L = leaves.size
    base = np.arange(n, dtype=np.int64)
    out = {"distinct": (base.copy(), int(leaves.min()))}
    eq = base.copy()
    eq[leaves] = n - 2 if n > 2 else 0
    out["equal"] = (eq, int(eq[leaves[0]]))
    k = min(3, L // 2)
    if k >= 1:
        # the smaller label only in the last k entries, the larger only in the first k, everything between once
        small, large = 1, n - 1
        others = np.setdiff1d(base, [small, large])[: L - 2 * k]
        tie = base.copy()
        tie[leaves[:k]] = large
        tie[leaves[L - k:]] = small
        tie[leaves[k:L - k]] = others
        out["tie"] = (tie, small)
        if L >= 2 * k + 1:
            more = tie.copy()
            more[leaves[k]] = large                        # one more of the larger
            out["tie, one more of the larger"] = (more, large)
    if L >= 5:
        ends = base.copy()
        ends[leaves] = np.resize(np.setdiff1d(base, [0, n - 1]), L)   # (a label twice at the most)
        ends[leaves[[1, L - 1]]] = 0
        ends[leaves[[0, 2, L - 2]]] = n - 1
        out["0 twice, n - 1 three times"] = (ends, n - 1)
        ends = ends.copy()
        ends[leaves[L // 2 if L // 2 not in (0, 1, 2, L - 2, L - 1) else 3]] = 0
        if L >= 6:
            out["0 three times, n - 1 three times"] = (ends, 0)
    if L >= 10:
        heavy = base.copy()
        heavy[leaves] = np.setdiff1d(base, [7])[:L]
        rng = np.random.default_rng(L)
        heavy[rng.choice(leaves, (9 * L) // 10, replace=False)] = 7
        out["one label on 90 %"] = (heavy, 7)
    return out


@pytest.mark.parametrize("length", LENGTHS)
def test_crafted_rows(hb, length):
    """a star: the hub sits at a middle vertex id, its list has exactly `length` entries, the leaves carry the labels"""
    n = length + 1
    hub = n // 2
    leaves = np.setdiff1d(np.arange(n), [hub])
    S = _sym(n, np.full(length, hub), leaves)
    assert S.indptr[hub + 1] - S.indptr[hub] == length
    A = _matrix(hb.g, S)
    for name, (init, want) in _crafted_inits(n, hub, leaves).items():
        got, res, _ = _check(hb, S, A, init=init, max_iter=1, name=(length, name))
        assert want is None or got[hub] == want, (length, name, got[hub], want)
        assert np.all(got[leaves] == init[hub])


@pytest.mark.parametrize("length", [TINY_LEN, TINY_LEN + 1, WAVE_LEN, WAVE_LEN + 1, SMALL_LEN, SMALL_LEN + 1, BLOCK_LEN,
                                    BLOCK_LEN + 1, 2 * SLOTS + 5])
def test_crafted_rows_directed(hb, length):
    """the hub's row and column together have exactly `length` entries: a third of the leaves hang on out-edges, the rest on
    in-edges, the hub stores its diagonal (it counts in the length, not in the multiset); and the undirected reading of
    the same matrix, where the marks go along the columns"""
    n = length - 1                                          # the diagonal is in the row and in the column
    hub = n // 2
    leaves = np.setdiff1d(np.arange(n), [hub])
    nout = leaves.size // 3
    r = np.concatenate([np.full(nout, hub), leaves[nout:], [hub]])
    c = np.concatenate([leaves[:nout], np.full(leaves.size - nout, hub), [hub]])
    S = _pattern(n, r, c)
    assert (S.indptr[hub + 1] - S.indptr[hub]) + (sp.csc_matrix(S).indptr[hub + 1] - sp.csc_matrix(S).indptr[hub]) == length
    A = _matrix(hb.g, S)
    for name, (init, want) in _crafted_inits(n, hub, leaves).items():
        got, _, _ = _check(hb, S, A, directed=True, init=init, max_iter=2, name=("directed", length, name))
        _check(hb, S, A, directed=False, init=init, max_iter=3, name=("rows of directed", length, name))


def test_more_long_rows_than_count_arrays(hb):
    """POOL + 8 hubs, all adjacent to the same BLOCK_LEN + 1 leaves: more long lists than count arrays, every hub the same label"""
    hubs, L = POOL + 8, BLOCK_LEN + 1
    n = hubs + L
    leaves = np.arange(hubs, n)
    S = _sym(n, np.repeat(np.arange(hubs), L), np.tile(leaves, hubs))
    A = _matrix(hb.g, S)
    rng = np.random.default_rng(10)
    init = np.arange(n, dtype=np.int64)
    init[leaves] = rng.permutation(np.setdiff1d(np.arange(n), [5, n - 1]))[:L]   # every other label once at the most
    init[leaves[:3]] = n - 1                                # the larger in the first three entries,
    init[leaves[-3:]] = 5                                   # the smaller in the last three: 5
    init[:hubs] = np.where(np.arange(hubs) % 2 == 0, 9, 3)  # the leaves see as many 9 as 3: 3
    got, _, _ = _check(hb, S, A, init=init, max_iter=1, name="hubs")
    assert np.all(got[:hubs] == 5) and np.all(got[leaves] == 3)
    _check(hb, S, A, init=init, max_iter=6, name="hubs, on")


# ---- degenerate shapes -------------------------------------------------------------------------------------------------
def test_degenerate(hb):
    g = hb.g
    for n, S in ((1, _sym(1, [], [])), (1, _sym(1, [], [], [0])), (50, _sym(50, [], [])), (50, _sym(50, [], [], np.arange(0, 50, 3))),
                 (TILE + 70, _sym(TILE + 70, [3, TILE - 1], [TILE + 60, TILE]))):
        for directed in (False, True):
            got, res, _ = _check(hb, S, directed=directed, max_iter=3, name=("degenerate", n, directed))
            if S.nnz == 0 or n <= 50:
                assert np.array_equal(got, np.arange(n)) and res["iterations"] == 1 and res["changed"] == 0 and res["evaluated"] == 0
                assert res["communities"] == n
    # isolated vertices keep the label they were given
    n = 300
    rng = np.random.default_rng(11)
    S = _sym(n, rng.integers(0, 100, 400), rng.integers(0, 100, 400))
    init = rng.integers(0, n, n)
    got, _, _ = _check(hb, S, init=init, max_iter=20, name="isolated")
    assert np.array_equal(got[100:], init[100:])


def test_product_result_and_csr_only_format(hb, monkeypatch):
    """directed = 0 reads only the CSR: it works on C = A A from the unmasked mxm (no CSC of its own) and on a matrix of the
    CSR-only format; directed = 1 is GrB_INVALID_OBJECT on both"""
    g = hb.g
    rng = np.random.default_rng(12)
    n = 500
    S = _pattern(n, rng.integers(0, n, 1500), rng.integers(0, n, 1500))
    One = _matrix(g, S, F)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", One, One, hb.descriptor()) == 0
    pp, pi, _ = P.host_csr()
    SP = sp.csr_matrix((np.ones(pi.size, np.int64), pi, pp), shape=(n, n))
    assert (SP != SP.T).nnz > 0
    _check(hb, SP, P, max_iter=12, name="product")
    v = g.Vector(n, I)
    assert g.cdlp(v, P, None, None, True, 5)[0] == g.GrB_INVALID_OBJECT
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Q = _matrix(g, S, I)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    _check(hb, S, Q, max_iter=12, name="CSR only")
    assert g.cdlp(v, Q, None, None, True, 5)[0] == g.GrB_INVALID_OBJECT


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_labels_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(13)
    n = 80
    S = _sym(n, rng.integers(0, n, 300), rng.integers(0, n, 300))
    A = _matrix(g, S, F, rng)
    before = rng.integers(-5, 1000, n).astype(I)
    v = _vector(g, n, before)
    good = _vector(g, n, rng.integers(0, n, n))

    def unchanged():
        return v.getStorage() == g.GrB_DENSE and np.array_equal(v.extractTuples()[1], before)

    call = lambda v_, A_, init_=None, directed=0, max_iter=10: lib.grb_cdlp(v_, A_, init_, directed, max_iter, None, None)
    assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                              # null handles
    assert call(v._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(v._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT             # an unbuilt A
    assert unchanged()
    R = g.Matrix(n, n + 1, F)                                                         # A not square
    assert R.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)) == 0
    assert call(v._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH              # size(labels) != n
    assert call(v._h, A._h, _vector(g, n - 1, np.zeros(n - 1))._h) == g.GrB_DIMENSION_MISMATCH   # size(init) != n
    assert unchanged()
    for max_iter in (0, -3):
        assert call(v._h, A._h, max_iter=max_iter) == g.GrB_INVALID_VALUE
    for directed in (2, -1):
        assert call(v._h, A._h, directed=directed) == g.GrB_INVALID_VALUE
    few = g.Vector(n, I)                                                              # nvals(init) != n
    assert few.build(np.arange(n - 1, dtype=I), np.zeros(n - 1, I), n - 1, None) == 0
    assert call(v._h, A._h, few._h) == g.GrB_INVALID_VALUE
    assert call(v._h, A._h, g.Vector(n, I)._h) == g.GrB_INVALID_VALUE                 # (nothing stored at all)
    assert unchanged()
    for where, bad in ((0, n), (n - 1, -1), (n // 2, 2 ** 31 - 1)):                   # an init value outside 0 .. n - 1
        vals = rng.integers(0, n, n)
        vals[where] = bad
        for sparse in (False, True):
            assert call(v._h, A._h, _vector(g, n, vals, sparse)._h) == g.GrB_INVALID_INDEX
    assert unchanged()
    bad_self = _vector(g, n, before)                                                   # ... with labels = init: untouched too
    assert call(bad_self._h, A._h, bad_self._h) == g.GrB_INVALID_INDEX
    assert np.array_equal(bad_self.extractTuples()[1], before)
    fv = g.Vector(n, F)                                                               # types
    assert fv.build(np.zeros(n, F), n) == 0
    assert call(fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert call(v._h, A._h, fv._h) == g.GrB_NOT_IMPLEMENTED
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                          # an A of element type code 2
    hp, hi, hv = S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)
    assert lib.grb_matrix_build_csr(h, hp.ctypes.data, hi.ctypes.data, hv.ctypes.data, S.nnz, None, None, None) == 0
    assert call(v._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    assert unchanged()
    One = _matrix(g, S, F)                                                            # directed on a product result
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", One, One, hb.descriptor()) == 0
    assert call(v._h, P._h, directed=1) == g.GrB_INVALID_OBJECT
    assert unchanged()
    # a descriptor and a null descriptor give the same result; the record is optional; a good call does write
    w = g.Vector(n, I)
    assert lib.grb_cdlp(w._h, A._h, good._h, 0, 10, hb.descriptor()._h, None) == 0
    assert call(v._h, A._h, good._h) == 0
    assert np.array_equal(v.extractTuples()[1], w.extractTuples()[1]) and not unchanged()


def test_determinism(hb):
    from graphblast_amd.graphgen import rmat_edges
    g = hb.g
    s, d, n = rmat_edges(12, 8, seed=5)
    S = _sym(n, np.asarray(s), np.asarray(d))
    assert np.diff(S.indptr).max() > WAVE_LEN
    A = _matrix(g, S, F)
    outs = []
    for _ in range(2):
        v = g.Vector(n, I)
        info, res = g.cdlp(v, A, None, None, False, 10)
        assert info == 0
        outs.append((_labels(g, v, n).tobytes(), [res[k] for k in ("iterations", "changed", "evaluated", "communities")]))
    assert outs[0] == outs[1]
    lab, rec, _, _ = _ref(S, False, None, 10)
    assert outs[0][0] == lab.tobytes() and outs[0][1] == [rec[k] for k in ("iterations", "changed", "evaluated", "communities")]


def test_cpp_frontend(tmp_path):
    """tests/tools/cdlp.cpp: two triangles and a bridge, the reciprocal edges, labels = init"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "cdlp")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "cdlp.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln.split(" ")[0] in ("und", "rec", "dir", "row", "init")]
    S = _sym(7, [0, 0, 1, 3, 3, 4, 2], [1, 2, 2, 4, 5, 5, 3])
    lab, rec, _, _ = _ref(S, False, None, 10)
    assert lab.tolist() == [0, 0, 0, 2, 2, 2, 6] and rec["changed"] == 0, (lab, rec)
    lab2, _, _, _ = _ref(S, False, [6, 0, 0, 3, 3, 6, 1], 10)
    assert lab2.tolist() != [6, 0, 0, 3, 3, 6, 1]

    def line(tag, vals):
        return tag + " " + " ".join(str(int(x)) for x in vals)

    assert lines == [line("und", lab), line("rec", [rec[k] for k in ("iterations", "changed", "evaluated", "communities")]),
                     "dir 3 0 2 0", "row 1 1 2 0", line("init", lab2)], lines
