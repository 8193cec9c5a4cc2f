"""k-truss and edge trussness on the device (csrc/ktruss.hip) against a scipy restatement of the definition in
include/grb_hip.h: repeat S = (A @ A).multiply(A), keep the entries >= k - 2, until nothing changes; the trussness from
running that for k = 3, 4, ...  Every comparison is exact, on ptr, ind and the values of both orientations of C.  Random
graphs in both element types of A and C with values that must not matter, a deep cascade, a triangle strip, a hub and rows
around every size threshold of the support kernel, survivor counts around the filter's tile, closed forms, identities through
the library's own mxm / select / tc, every error code with C unchanged, aliasing, determinism and the C++ frontend."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
# csrc/ktruss.hip
WAVE_LEN = 64        # kKtWaveLen: a row of up to this many entries is one wave's task, a longer one workgroup tasks
LANE_LEN = 32        # kKtLaneLen: a partner of up to this many entries is walked by a lane, a longer one by the wave
BITS = 4096          # kKtBits: a column window of up to this many columns is a bitmap, a wider one a hash table
HASH_LEN = 4096      # kKtHashLen: the most entries of one hash table; a longer list is taken in slices
TASK = 256           # kKtTask: partners of one workgroup task
T = 2048             # kKtTile: the entries one workgroup of the filter compacts


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs and the reference ------------------------------------------------------------------------------------------
def _sym(n, r, c):
    """the simple undirected graph of the draws (r, c): loops dropped, both directions, no duplicates; int64 ones"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    r, c = r[keep], c[keep]
    S = sp.csr_matrix((np.ones(2 * r.size, np.int64), (np.concatenate([r, c]), np.concatenate([c, r]))), shape=(n, n))
    S.data[:] = 1
    S.sort_indices()
    return S


def _rand(rng, n, draws):
    return _sym(n, rng.integers(0, n, draws), rng.integers(0, n, draws))


def _supports(S):
    """the support of every stored entry of S (a 0 / 1 symmetric pattern), in S's order"""
    D = (S @ S).multiply(S) + S                          # S's structure: the support + 1
    D = sp.csr_matrix(D)
    D.sort_indices()
    assert np.array_equal(D.indptr, S.indptr) and np.array_equal(D.indices, S.indices)
    return D.data - 1


def _ref_ktruss(S, k):
    """-> (ptr, ind, supports) of the k-truss, the rounds it took (the last one changes nothing), the truss as a pattern"""
    n = S.shape[0]
    rounds = 0
    while True:
        rounds += 1
        sup = _supports(S)
        keep = sup >= k - 2
        if keep.all():
            return (S.indptr.astype(I), S.indices.astype(I), sup.astype(np.int64)), rounds, S
        rows = np.repeat(np.arange(n), np.diff(S.indptr))
        S = sp.csr_matrix((np.ones(int(keep.sum()), np.int64), (rows[keep], S.indices[keep])), shape=(n, n))
        S.sort_indices()
        if S.nnz == 0:
            return (S.indptr.astype(I), S.indices.astype(I), np.zeros(0, np.int64)), rounds, S


def _ref_trussness(S):
    """-> (ptr, ind, trussness) on S's structure, kmax"""
    n = S.shape[0]
    Tr = sp.csr_matrix((np.full(S.nnz, 2, np.int64), S.indices.copy(), S.indptr.copy()), shape=(n, n))
    cur, k = S, 2
    while cur.nnz:
        k += 1
        cur = _ref_ktruss(cur, k)[2]
        Tr = Tr + cur                                    # one more for every truss the edge is in
    Tr = sp.csr_matrix(Tr)
    Tr.sort_indices()
    assert np.array_equal(Tr.indices, S.indices)
    return (S.indptr.astype(I), S.indices.astype(I), Tr.data.astype(np.int64)), (k - 1 if S.nnz else 2)


def _matrix(g, S, dt=F, rng=None, diag=None):
    """A with S's structure; values that must not matter (zeros and negatives among them); diag: rows that also store
    their diagonal entry"""
    n = S.shape[0]
    P = S
    if diag is not None:
        P = sp.csr_matrix(S + sp.csr_matrix((np.ones(len(diag), np.int64), (diag, diag)), shape=(n, n)))
        P.sort_indices()
    vals = np.ones(P.nnz, dt) if rng is None else rng.integers(-3, 4, P.nnz).astype(dt)
    A = g.Matrix(n, n, dt)
    assert A.build_csr(P.indptr.astype(I), P.indices.astype(I), vals) == 0
    return A


def _both(C):
    return list(C.host_csr()) + list(C.host_csc())


def _same(C, want, name=""):
    """C's two orientations, exactly: the pointers, the indices, the values in C's type"""
    ptr, ind, val = want
    got = _both(C)
    for o in (0, 3):
        assert np.array_equal(got[o], ptr), (name, "ptr", o)
        assert np.array_equal(got[o + 1], ind), (name, "ind", o)
        assert got[o + 2].dtype == C.np_dtype and np.array_equal(got[o + 2], val.astype(C.np_dtype)), (name, "val", o)
    assert C.nvals() == ind.size


def _check(hb, S, ks, dt=F, ct=I, rng=None, diag=None, name=""):
    """ktruss for every k of ks and the trussness of the graph S, against the reference; -> {k: (result dict, ref rounds)}"""
    g = hb.g
    n = S.shape[0]
    A = _matrix(g, S, dt, rng, diag)
    out = {}
    for k in ks:
        want, rounds, _ = _ref_ktruss(S, k)
        Cm = g.Matrix(n, n, ct)
        info, res = g.ktruss(Cm, A, k, None)
        assert info == 0, (name, k, info)
        _same(Cm, want, (name, k))
        assert res["edges"] == S.nnz // 2 and res["result_edges"] == want[1].size // 2 and res["kmax"] == k
        assert 1 <= res["rounds"] <= rounds or S.nnz == 0, (name, k, res, rounds)
        out[k] = (res, rounds, want)
    return out


def _check_trussness(hb, S, dt=F, ct=I, rng=None, name=""):
    g = hb.g
    n = S.shape[0]
    want, kmax = _ref_trussness(S)
    Cm = g.Matrix(n, n, ct)
    info, res = g.trussness(Cm, _matrix(g, S, dt, rng), None)
    assert info == 0, name
    _same(Cm, want, name)
    assert res["kmax"] == kmax and res["edges"] == res["result_edges"] == S.nnz // 2, (name, res, kmax)
    assert res["supports"] <= res["rounds"]
    return Cm, res


# ---- random graphs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("ct", [F, I])
@pytest.mark.parametrize("n, draws", [(300, 3000), (2000, 30000)])
def test_random_graphs(hb, dt, ct, n, draws):
    """k = 2 .. 6: non-empty trusses after a few rounds for the small k, empty ones for the large; A's values include zeros
    and negatives; a tenth of the rows store their diagonal entry"""
    rng = np.random.default_rng(7)
    S = _rand(rng, n, draws)
    diag = np.sort(rng.choice(n, n // 10, replace=False))
    out = _check(hb, S, range(2, 7), dt, ct, rng, diag, (n, draws))
    sizes = [out[k][2][1].size for k in range(2, 7)]
    assert sizes[0] == S.nnz and any(0 < s < S.nnz for s in sizes) and any(s == 0 for s in sizes), sizes
    assert any(out[k][1] >= 2 and out[k][2][1].size > 0 for k in (3, 4)), [out[k][1] for k in range(2, 7)]
    assert all(out[k][0]["supports"] == out[k][0]["rounds"] or out[k][2][1].size == 0 for k in range(2, 7))


def test_random_trussness(hb):
    rng = np.random.default_rng(7)
    for n, draws, ct in ((300, 3000, I), (2000, 30000, F)):
        _check_trussness(hb, _rand(rng, n, draws), F, ct, rng, (n, draws))


# ---- a deep cascade ----------------------------------------------------------------------------------------------------
def test_deep_cascade(hb):
    """a power-law graph, n = 4096, 60 000 draws with probability ~ rank^-0.9, k = 8: the reference needs at least 8 rounds"""
    rng = np.random.default_rng(7)
    n = 4096
    p = np.arange(1, n + 1, dtype=np.float64) ** -0.9
    p /= p.sum()
    e = rng.choice(n, (60000, 2), p=p)
    S = _sym(n, e[:, 0], e[:, 1])
    assert np.diff(S.indptr).max() > 1000
    res, rounds, want = _check(hb, S, [8], F, I, rng, None, "cascade")[8]
    assert rounds >= 8, rounds
    assert 1 <= res["rounds"] <= rounds, (res, rounds)
    assert want[1].size > 0


def test_triangle_strip(hb):
    """edges (i, i + 1) and (i, i + 2) over 40 vertices, k = 4: two edges of one triangle leave in the same round, and in
    the end all of it goes"""
    n = 40
    r = np.concatenate([np.arange(n - 1), np.arange(n - 2)])
    c = np.concatenate([np.arange(1, n), np.arange(2, n)])
    S = _sym(n, r, c)
    res, rounds, want = _check(hb, S, [4], F, I)[4]
    assert want[1].size == 0 and rounds >= 2
    _check(hb, S, [2, 3], I, F)
    _check_trussness(hb, S, name="strip")


# ---- long rows and thresholds ------------------------------------------------------------------------------------------
def _with_row(rng, n, cols, draws):
    """vertex 0 joined to exactly `cols`, over a sparse random graph on the other vertices"""
    r, c = rng.integers(1, n, draws), rng.integers(1, n, draws)
    S = _sym(n, np.concatenate([r, np.zeros(len(cols), np.int64)]), np.concatenate([c, np.asarray(cols, np.int64)]))
    assert S.indptr[1] == len(cols)
    return S


@pytest.mark.parametrize("every", [1, 2])
def test_hub(hb, every):
    """one hub joined to every other vertex (every = 1: its list is a run of consecutive columns; every = 2: to every second
    one, a list with gaps), over a sparse random graph: its degree is larger than a hash table, a bitmap and a task"""
    rng = np.random.default_rng(11)
    deg = HASH_LEN + 103
    n = every * deg + 1
    S = _with_row(rng, n, np.arange(1, n, every), 3 * n)
    assert S.indptr[1] == deg > max(HASH_LEN, BITS, TASK)
    _check(hb, S, [3, 4], F, I, rng, None, ("hub", every))


@pytest.mark.parametrize("length", [WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1, TASK - 1, TASK, TASK + 1, 2 * TASK, 2 * TASK + 1])
def test_row_lengths_around_the_task_thresholds(hb, length):
    """a row one below, at and one above: a wave's task against workgroup tasks, one task against two, two against three"""
    rng = np.random.default_rng(12)
    n = 1500
    S = _with_row(rng, n, 1 + np.sort(rng.choice(n - 1, length, replace=False)), 8 * n)
    _check(hb, S, [2, 3, 4], F, I, rng, None, length)


@pytest.mark.parametrize("length", [HASH_LEN - 1, HASH_LEN, HASH_LEN + 1])
def test_row_lengths_around_the_hash_table(hb, length):
    """a list with gaps (no bitmap) of one entry less than a hash table takes, exactly that, and one more (two slices)"""
    rng = np.random.default_rng(13)
    n = length + 400
    S = _with_row(rng, n, 1 + np.sort(rng.choice(n - 1, length, replace=False)), 3 * n)
    _check(hb, S, [3], F, I, rng, None, length)


@pytest.mark.parametrize("window", [BITS - 1, BITS, BITS + 1])
def test_column_windows_around_the_bitmap(hb, window):
    """a row of 100 entries (workgroup tasks) and one of 40 (a wave's task) whose columns span exactly `window` columns"""
    rng = np.random.default_rng(14)
    n = BITS + 300
    for length in (100, 40):
        first = 7
        inner = first + 1 + np.sort(rng.choice(window - 2, length - 2, replace=False))
        cols = np.concatenate([[first], inner, [first + window - 1]])
        S = _with_row(rng, n, cols, 8 * n)
        assert S.indices[S.indptr[1] - 1] - S.indices[0] + 1 == window
        _check(hb, S, [2, 3, 4], F, I, rng, None, (window, length))


@pytest.mark.parametrize("length", [LANE_LEN - 1, LANE_LEN, LANE_LEN + 1])
def test_partner_lengths_around_the_lane_walk(hb, length):
    """partners of exactly these lengths under an owner with a longer list: a clique of length + 1 vertices (every list
    has `length` entries) all joined to one vertex of degree 200"""
    m = length + 1
    r, c = np.triu_indices(m, 1)
    n = 400
    hub = m
    hr = np.full(200, hub)
    hc = np.concatenate([np.arange(m), np.arange(m + 1, m + 1 + 200 - m)])
    S = _sym(n, np.concatenate([r, hr]), np.concatenate([c, hc]))
    assert S.indptr[hub + 1] - S.indptr[hub] == 200 and S.indptr[1] == length + 1
    _check(hb, S, [2, 3, length + 2, length + 3], F, I, None, None, length)
    # ... and with lists of exactly `length` entries: the clique without the extra vertex
    _check(hb, _sym(m, r, c), [2, m, m + 1], I, F, None, None, ("clique", length))


# ---- compaction edges --------------------------------------------------------------------------------------------------
def _cliques_with_pendant_triangles(edges):
    """K4s (6 edges, support 2), K5s (10, support 3) and at most one K6 (15, support 4) with exactly `edges` edges between
    them, and a pendant triangle (support 1) on the first vertex of every clique: k = 4 takes the pendant triangles away in
    the first round and nothing in the second"""
    blocks = [6] if edges % 2 else []
    left = edges - (15 if edges % 2 else 0)
    a = next(a for a in range(5) if (left - 6 * a) % 10 == 0 and left - 6 * a >= 0)
    blocks += [4] * a + [5] * ((left - 6 * a) // 10)
    r, c, at = [], [], 0
    for m in blocks:
        x, y = np.triu_indices(m, 1)
        r += [at + x, np.array([at, at, at + m])]
        c += [at + y, np.array([at + m, at + m + 1, at + m + 1])]
        at += m + 2
    return _sym(at, np.concatenate(r), np.concatenate(c)), len(blocks)


@pytest.mark.parametrize("survivors", [T // 2 - 1, T // 2, T // 2 + 1, T - 1, T, T + 1])
def test_survivors_around_the_tile(hb, survivors):
    """2047, 2048 and 2049 surviving EDGES after the first round (4094, 4096 and 4098 entries: the end of the second tile)
    and, since a symmetric matrix without a diagonal holds an even number of entries, 1023, 1024 and 1025 edges for the
    2046, 2048 and 2050 entries around the end of the first tile"""
    S, nblocks = _cliques_with_pendant_triangles(survivors)
    assert S.nnz == 2 * (survivors + 3 * nblocks)
    res, rounds, want = _check(hb, S, [4], F, I, None, None, survivors)[4]
    assert want[1].size == 2 * survivors and rounds == 2 and res["rounds"] == 2 and res["supports"] == 2
    if survivors == T:
        _check_trussness(hb, S, name="cliques")


def test_runs_of_empty_rows(hb):
    """thousands of empty rows before, between and after the populated ones"""
    gap = 5000
    r, c, at = [], [], gap
    for i in range(6):
        a, b = np.triu_indices(6, 1)
        r += [at + a, np.array([at, at, at + 6])]
        c += [at + b, np.array([at + 6, at + 7, at + 7])]
        at += 8 + (gap if i in (1, 4) else 0)
    S = _sym(at + gap, np.concatenate(r), np.concatenate(c))
    out = _check(hb, S, [2, 3, 4, 6, 7], F, I)
    assert out[4][2][1].size == 6 * 30 and out[7][2][1].size == 0
    _check_trussness(hb, S, name="empty rows")


# ---- closed forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [3, 17, 70])
def test_complete_graph(hb, m):
    S = _sym(m, *np.triu_indices(m, 1))
    out = _check(hb, S, [2, 3, m, m + 1], I, I)
    assert np.all(out[m][2][2] == m - 2) and out[m][2][1].size == m * (m - 1) and out[m + 1][2][1].size == 0
    Cm, res = _check_trussness(hb, S, name=m)
    assert res["kmax"] == m and np.all(Cm.host_csr()[2] == m)


def test_two_cliques_joined_by_a_path(hb):
    a, b = np.triu_indices(6, 1)
    c, d = np.triu_indices(9, 1)
    path = np.arange(5, 5 + 4)                           # 5 - 6 - 7 - 8 - 9, the second clique on 9 .. 17
    S = _sym(18, np.concatenate([a, c + 9, path]), np.concatenate([b, d + 9, path + 1]))
    out = _check(hb, S, [2, 3, 6, 7, 9, 10], F, F)
    assert out[3][2][1].size == 30 + 72 and out[7][2][1].size == 72 and out[10][2][1].size == 0
    Cm, res = _check_trussness(hb, S, name="two cliques")
    assert res["kmax"] == 9 and sorted(set(Cm.host_csr()[2].tolist())) == [2, 6, 9]


def test_bipartite(hb):
    rng = np.random.default_rng(15)
    S = _sym(300, rng.integers(0, 150, 2000), rng.integers(150, 300, 2000))
    out = _check(hb, S, [2, 3], F, I)
    assert out[3][2][1].size == 0 and not out[2][2][2].any()
    Cm, res = _check_trussness(hb, S, name="bipartite")
    assert res["kmax"] == 2 and np.all(Cm.host_csr()[2] == 2)


def test_degenerate(hb):
    """n = 1, n = 2, a matrix with no entries, a matrix with only diagonal entries"""
    g = hb.g
    for n, S, diag in ((1, _sym(1, [], []), None), (2, _sym(2, [0], [1]), None), (2, _sym(2, [], []), None),
                       (50, _sym(50, [], []), None), (50, _sym(50, [], []), np.arange(0, 50, 3)), (1, _sym(1, [], []), np.array([0]))):
        out = _check(hb, S, [2, 3], F, I, None, diag, (n, "degenerate"))
        assert out[3][2][1].size == 0
        A = _matrix(g, S, F, None, diag)
        Cm = g.Matrix(n, n, F)
        info, res = g.trussness(Cm, A, None)
        assert info == 0 and Cm.nvals() == S.nnz and res["kmax"] == 2
        _same(Cm, (S.indptr.astype(I), S.indices.astype(I), np.full(S.nnz, 2)))


# ---- identities through the library ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph():
    rng = np.random.default_rng(21)
    return _rand(rng, 600, 9000)


def test_supports_sum_to_six_triangle_counts(hb, graph):
    g = hb.g
    n = graph.shape[0]
    A = _matrix(g, graph, I)
    Cm = g.Matrix(n, n, I)
    assert g.ktruss(Cm, A, 2, None)[0] == 0
    L = g.Matrix(n, n, I)
    assert g.select(L, None, None, "tril", A, -1, hb.descriptor()) == 0
    info, ntri, _ = g.tc(L, g.Matrix(n, n, I), hb.descriptor())
    assert info == 0 and ntri > 0
    assert int(Cm.host_csr()[2].astype(np.int64).sum()) == 6 * ntri


def _op_by_op(hb, S, k):
    """the loop a caller writes today: mxm under the survivors' mask (the graph is symmetric: A A^T read from the CSR),
    select VALUEGE k - 2, the values back to 1"""
    g = hb.g
    n = S.shape[0]
    d = hb.descriptor()
    assert d.toggle(g.GrB_INP1) == 0
    ptr, ind = S.indptr.astype(I), S.indices.astype(I)
    while True:
        cur = g.Matrix(n, n, F)
        assert cur.build_csr(ptr, ind, np.ones(ind.size, F)) == 0
        P, K = g.Matrix(n, n, F), g.Matrix(n, n, F)
        assert g.mxm(P, cur, None, "PlusMultiplies", cur, cur, d) == 0
        assert g.select(K, None, None, "valuege", P, k - 2, hb.descriptor()) == 0
        kp, ki, kv = K.host_csr()
        if ki.size == ind.size or ki.size == 0:
            return kp, ki, kv
        ptr, ind = kp, ki


def test_bit_identical_to_the_op_by_op_loop(hb, graph):
    g = hb.g
    n = graph.shape[0]
    A = _matrix(g, graph, F)
    sizes = []
    for k in (3, 4, 5, 6):
        Cm = g.Matrix(n, n, F)
        assert g.ktruss(Cm, A, k, None)[0] == 0
        kp, ki, kv = _op_by_op(hb, graph, k)
        p, i, v = Cm.host_csr()
        assert np.array_equal(p, kp) and np.array_equal(i, ki) and v.tobytes() == kv.tobytes(), k
        sizes.append(i.size)
    assert sizes[0] > 0


def test_trussness_selected_is_the_ktruss(hb, graph):
    g = hb.g
    n = graph.shape[0]
    A = _matrix(g, graph, F)
    Tm = g.Matrix(n, n, I)
    info, res = g.trussness(Tm, A, None)
    assert info == 0 and res["kmax"] >= 3
    for k in range(2, res["kmax"] + 2):
        Sel, Cm = g.Matrix(n, n, I), g.Matrix(n, n, I)
        assert g.select(Sel, None, None, "valuege", Tm, k, hb.descriptor()) == 0
        assert g.ktruss(Cm, A, k, None)[0] == 0
        for x, y in zip(_both(Sel)[0:2] + _both(Sel)[3:5], _both(Cm)[0:2] + _both(Cm)[3:5]):
            assert np.array_equal(x, y), k
        assert (Cm.nvals() == 0) == (k == res["kmax"] + 1)


def test_idempotent_and_in_place(hb, graph):
    """ktruss of ktruss(k)'s own result is itself (in one round); C may be A, for both drivers"""
    g = hb.g
    n = graph.shape[0]
    A = _matrix(g, graph, F)
    Cm = g.Matrix(n, n, I)
    assert g.ktruss(Cm, A, 4, None)[0] == 0
    first = _both(Cm)
    assert first[1].size > 0
    C2 = g.Matrix(n, n, I)
    info, res = g.ktruss(C2, Cm, 4, None)
    assert info == 0 and res["rounds"] == 1 and res["supports"] == 1
    assert all(np.array_equal(x, y) for x, y in zip(first, _both(C2)))
    info, res = g.ktruss(Cm, Cm, 4, None)                # in place, on a matrix whose values are supports
    assert info == 0 and all(np.array_equal(x, y) for x, y in zip(first, _both(Cm)))
    B = _matrix(g, graph, I, np.random.default_rng(3))
    assert g.ktruss(B, B, 4, None)[0] == 0
    assert all(np.array_equal(x, y) for x, y in zip(first, _both(B)))
    want, _ = _ref_trussness(graph)
    Bt = _matrix(g, graph, F, np.random.default_rng(4))
    assert g.trussness(Bt, Bt, None)[0] == 0
    _same(Bt, want, "trussness in place")


def test_determinism(hb):
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    g = hb.g
    s, dd, n = rmat_edges(10, 8, seed=5)
    S = _sym(n, np.asarray(s), np.asarray(dd))
    A = _matrix(g, S, F)
    outs = []
    for _ in range(2):
        Cm, Tm = g.Matrix(n, n, F), g.Matrix(n, n, I)
        assert g.ktruss(Cm, A, 4, None)[0] == 0 and g.trussness(Tm, A, None)[0] == 0
        outs.append(_both(Cm) + _both(Tm))
    assert outs[0][1].size > 0
    assert all(x.tobytes() == y.tobytes() for x, y in zip(outs[0], outs[1]))


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_c_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(31)
    n = 60
    S = _rand(rng, n, 600)
    A = _matrix(g, S, F, rng)
    Cm = g.Matrix(n, n, I)
    assert g.ktruss(Cm, A, 3, None)[0] == 0
    before = _both(Cm)
    assert before[1].size > 0

    def unchanged():
        return all(np.array_equal(x, y) for x, y in zip(before, _both(Cm)))

    kt = lambda C_, A_, k=3: lib.grb_ktruss(C_, A_, k, None, None)
    tr = lambda C_, A_: lib.grb_trussness(C_, A_, None, None)
    for f in (kt, tr):
        assert f(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                           # null handles
        assert f(Cm._h, None) == g.GrB_UNINITIALIZED_OBJECT
        assert f(Cm._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT          # an unbuilt A
        assert unchanged()
    # A not square, C not n x n
    R = g.Matrix(n, n + 1, F)
    assert R.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)) == 0
    Cr = g.Matrix(n, n + 1, I)
    for f in (kt, tr):
        assert f(Cm._h, R._h) == g.GrB_DIMENSION_MISMATCH
        assert f(Cr._h, R._h) == g.GrB_DIMENSION_MISMATCH
        assert f(g.Matrix(n + 1, n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH
        assert f(g.Matrix(n, n - 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert unchanged()
    for k in (1, 0, -5):                                                           # k < 2
        assert g.ktruss(Cm, A, k, None)[0] == g.GrB_INVALID_VALUE
    assert unchanged()
    # a type outside f32 / i32: a C of element type code 2
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0
    for f in (kt, tr):
        assert f(h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    # A without a CSC of its own: a product result; its transpose under INP0 = TRAN has one
    d = hb.descriptor()
    One = _matrix(g, S, F)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", One, One, d) == 0
    for f in (kt, tr):
        assert f(Cm._h, P._h) == g.GrB_INVALID_OBJECT
    assert unchanged()
    dt = hb.descriptor()
    assert dt.toggle(g.GrB_INP0) == 0
    P2 = g.Matrix(n, n, F)
    assert g.transpose(P2, None, None, P, dt) == 0
    C2 = g.Matrix(n, n, I)
    assert g.ktruss(C2, P2, 3, None)[0] == 0
    pp, pi, _ = P.host_csr()
    S2 = sp.csr_matrix((np.ones(pi.size, np.int64), pi, pp), shape=(n, n))
    S2.setdiag(0)
    S2.eliminate_zeros()
    S2.sort_indices()
    _same(C2, _ref_ktruss(S2, 3)[0], "A A with a CSC")
    # not symmetric: A with one entry taken out
    r = int(np.argmax(np.diff(S.indptr)))
    drop = S.indptr[r]
    ptr = S.indptr.astype(I).copy()
    ptr[r + 1:] -= 1
    N = g.Matrix(n, n, F)
    assert N.build_csr(ptr, np.delete(S.indices.astype(I), drop), np.ones(S.nnz - 1, F)) == 0
    for f in (kt, tr):
        assert f(Cm._h, N._h) == g.GrB_INVALID_VALUE
    assert unchanged()
    # a null descriptor and a descriptor give the same result; the record is optional
    Cd = g.Matrix(n, n, I)
    assert lib.grb_ktruss(Cd._h, A._h, 3, hb.descriptor()._h, None) == 0
    assert all(np.array_equal(x, y) for x, y in zip(before, _both(Cd)))


def test_cpp_frontend(tmp_path):
    """tests/tools/ktruss.cpp: K4 with a pendant triangle and a pendant edge"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ktruss")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "ktruss.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln.split(" ")[0] in ("k4", "k3T", "truss", "rec")]
    edges = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3), (3, 4), (3, 5), (4, 5), (5, 6)]
    S = _sym(7, [a for a, _ in edges], [b for _, b in edges])

    def line(tag, want):
        p, i, v = want
        return "%s 7 7 %d | %s | %s | %s" % (tag, i.size, " ".join(map(str, p)), " ".join(map(str, i)), " ".join(map(str, v)))

    tw, kmax = _ref_trussness(S)
    assert kmax == 4
    assert lines == [line("k4", _ref_ktruss(S, 4)[0]), line("k3T", _ref_ktruss(S, 3)[0]), line("truss", tw),
                     "rec 1 10 10 4"], lines
