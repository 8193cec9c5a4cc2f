"""The local clustering coefficient on the device (csrc/lcc.hip) against a scipy restatement of the definition in
include/grb_hip.h: B = the 0 / 1 off-diagonal pattern of A, S = pattern(B + B^T), num = the row sums of (S B) .* S, d = the row
lengths of S, lcc = num / (d (d - 1)) in float64 rounded to float32 once, triangles = sum((S S) .* S) / 6.  Every comparison
is EXACT: the f32 values bit for bit, and the record's integers.  Random undirected and directed graphs in both element
types with values that must not matter, every size threshold of the kernels straddled, closed-form graphs, the library's
own tc and ktruss as cross-checks, the golden graphs, a product result, the CSR-only format, every error code with lcc
unchanged, degenerate shapes, caller-owned storage, determinism, a relabelling and the C++ frontend."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
# csrc/lcc.hip.  O(v): the neighbours of v that rank above it by (d, id); per edge the end with the longer O is the pivot
MERGE_STEP = 64      # kWave: entries of a CSR row / CSC column that one step of the merge places
WAVE_LEN = 256       # kLcWaveLen: a pivot whose O has up to this many entries is a wave's task, a longer one a workgroup's
KEYS = 2048          # kLcKeys: entries of a pivot's O in the LDS table at a time; a longer O is taken in slices
LANE_LEN = 32        # kLcLaneLen: a partner whose O has up to this many entries is walked by one lane, a longer one by the wave
CHUNK = (256, 1024)  # kLcChunk: partners per task of a wave / of a workgroup
WAVE_GRID = 65536    # the most waves the enumeration of the waves' tasks is launched with: beyond, a wave takes several tasks in turn
BLOCK_GRID = 16384   # ... and the most workgroups for the workgroups' tasks.  A workgroup task needs a pivot with more than
                     # WAVE_LEN entries in its O, so BLOCK_GRID + 1 of them need more than 16 385 x 257 = 4.2 M edges, 8.4 M entries:
                     # test_more_workgroup_tasks_than_workgroups has a closed-form graph of that size


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


def _ref(A):
    """-> lcc (f32), dict(edges, triangles, closed, wedges, max_degree), num, d.  A: any scipy matrix; only its structure counts"""
    n = A.shape[0]
    B = sp.csr_matrix(A, dtype=np.int64, copy=True)
    B.data[:] = 1
    B.setdiag(0)
    B.eliminate_zeros()
    S = sp.csr_matrix(B + B.T)
    S.data[:] = 1
    S.sort_indices()
    d = np.diff(S.indptr).astype(np.int64)
    if n <= 4096 and S.nnz > 200 * n:                        # a dense core: the same products through BLAS, exact in f64
        Sd, Bd = S.toarray().astype(np.float64), B.toarray().astype(np.float64)
        num = np.rint(((Sd @ Bd) * Sd).sum(axis=1)).astype(np.int64)
        six = int(np.rint(((Sd @ Sd) * Sd).sum()))
    else:
        num = np.asarray(((S @ B).multiply(S)).sum(axis=1)).ravel().astype(np.int64)
        six = int(num.sum()) if (B != S).nnz == 0 else int(((S @ S).multiply(S)).sum())   # (B = S: the same product)
    with np.errstate(divide="ignore", invalid="ignore"):
        lcc = np.where(d >= 2, num.astype(np.float64) / (d.astype(np.float64) * (d - 1).astype(np.float64)), 0.0).astype(F)
    assert six % 6 == 0
    rec = dict(edges=int(S.nnz) // 2, triangles=six // 6, closed=int(num.sum()), wedges=int((d * (d - 1)).sum()),
               max_degree=int(d.max()) if n else 0)
    return lcc, rec, num, d


def _matrix(g, S, dt=F, rng=None):
    """A with S's structure; values that must not matter (zeros and negatives among them)"""
    n = S.shape[0]
    vals = np.ones(S.nnz, dt) if rng is None else rng.integers(-3, 4, S.nnz).astype(dt)
    A = g.Matrix(n, n, dt)
    assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), vals) == 0
    return A


def _values(g, v, n):
    assert v.getStorage() == g.GrB_DENSE and v.nvals() == n and v.np_dtype == F
    info, vals = v.extractTuples()
    assert info == 0 and vals.dtype == F and vals.size == n
    return vals


REC = ("edges", "triangles", "closed", "wedges", "max_degree")


def _check(hb, S, A=None, directed=False, name="", want=None, v=None):
    """lcc on S's graph against the reference, bit for bit; -> (values, record)"""
    g = hb.g
    n = S.shape[0]
    if A is None:
        A = _matrix(g, S)
    lcc, rec = (want if want is not None else _ref(S))[:2]
    if v is None:
        v = g.Vector(n, F)
    info, res = g.lcc(v, A, None, directed)
    assert info == 0, (name, info)
    got = _values(g, v, n)
    print(name, {k: res[k] for k in REC}, rec, "loop_ms", res["loop_ms"])
    bad = np.flatnonzero(got.view(np.uint32) != lcc.view(np.uint32))
    assert bad.size == 0, (name, bad.size, bad[:10], got[bad[:10]], lcc[bad[:10]])
    for k in REC:
        assert res[k] == rec[k], (name, k, res, rec)
    assert res["loop_ms"] >= 0
    return got, res


def _one_way(S, rng, frac):
    """S (symmetric) with one direction of about frac of its edges dropped: the same undirected graph, other m"""
    U = sp.triu(S, 1).tocoo()
    drop = rng.random(U.nnz) < frac
    which = rng.random(U.nnz) < 0.5
    r = np.concatenate([U.row[~(drop & which)], U.col[~(drop & ~which)]])
    c = np.concatenate([U.col[~(drop & which)], U.row[~(drop & ~which)]])
    return _pattern(S.shape[0], r, c)


def _complete(m, one_way=False):
    r, c = np.triu_indices(m, 1)
    return _pattern(m, r, c) if one_way else _sym(m, r, c)


def _layered(t, leaves, x):
    """a clique T of t vertices; x vertices joined to all of T (they lift T's degrees above everything else); per entry K of
    `leaves` a middle vertex joined to all of T and to K leaves, each leaf also joined to one vertex of T.  A middle vertex's
    O is T (t entries) and it is the pivot of its K leaves (O of 2 entries) and of the t - 1 vertices of T with a non-empty
    O: K + t - 1 partners.  -> S (symmetric), the middle vertices"""
    assert x > max(leaves) + 1 and t > 2
    r, c = [a for a in np.triu_indices(t, 1)]
    r, c = list(r), list(c)
    nxt = t
    for _ in range(x):
        r += [nxt] * t
        c += list(range(t))
        nxt += 1
    mids = []
    for K in leaves:
        p = nxt
        nxt += 1
        mids.append(p)
        r += [p] * t
        c += list(range(t))
        for k in range(K):
            r += [nxt, nxt]
            c += [p, k % t]
            nxt += 1
    return _sym(nxt, r, c), mids


def _olen(S):
    """|O(v)| of the undirected graph S"""
    d = np.diff(S.indptr)
    v = np.repeat(np.arange(S.shape[0]), d)
    u = S.indices
    above = (d[u] > d[v]) | ((d[u] == d[v]) & (u > v))
    return np.bincount(v[above], minlength=S.shape[0])


# ---- random graphs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("n, draws", [(2000, 8000), (20000, 200000)])
def test_random_undirected(hb, dt, n, draws):
    """isolated vertices, vertices of degree 1, stored diagonals, values that must not matter"""
    rng = np.random.default_rng(1 + n)
    m = n - 60                                               # the draws; then ten pendant vertices, then 50 isolated ones
    S = _sym(n - 50, np.concatenate([rng.integers(0, m, draws), m + np.arange(10)]), np.concatenate([rng.integers(0, m, draws), np.arange(10)]),
             rng.integers(0, n - 50, n // 10))
    S = sp.csr_matrix((S.data, S.indices, np.concatenate([S.indptr, np.full(50, S.indptr[-1])])), shape=(n, n))   # 50 isolated
    d = _ref(S)[3]
    assert (d == 0).sum() >= 50 and (d == 1).any() and S.diagonal().sum() > 0
    _check(hb, S, _matrix(hb.g, S, dt, rng), name=("undirected", dt.__name__, n))


@pytest.mark.parametrize("dt", [F, I])
def test_random_directed(hb, dt):
    """reciprocal and one-way edges mixed, stored diagonals, a hub whose row and column are longer than a step of the merge"""
    rng = np.random.default_rng(3)
    n = 3000
    r = np.concatenate([rng.integers(0, n, 20000), np.full(300, 7), rng.integers(0, n, 200), np.arange(0, n, 9)])
    c = np.concatenate([rng.integers(0, n, 20000), rng.integers(0, n, 300), np.full(200, 7), np.arange(0, n, 9)])
    back = rng.random(r.size) < 0.3                         # three in ten also the other way
    S = _pattern(n, np.concatenate([r, c[back]]), np.concatenate([c, r[back]]))
    T = sp.csc_matrix(S)
    assert (S != S.T).nnz > 0 and S.multiply(S.T).nnz > S.diagonal().sum() and S.diagonal().sum() > 0
    assert S.indptr[8] - S.indptr[7] > MERGE_STEP and T.indptr[8] - T.indptr[7] > MERGE_STEP
    got, res = _check(hb, S, _matrix(hb.g, S, dt, rng), directed=True, name=("directed", dt.__name__))
    # and the symmetrised graph of the same draw has the same edges and triangles
    _, res2 = _check(hb, sp.csr_matrix(_sym(n, S.tocoo().row, S.tocoo().col)), name="symmetrised")
    assert res2["edges"] == res["edges"] and res2["triangles"] == res["triangles"] and res2["wedges"] == res["wedges"]


@pytest.mark.parametrize("length", [MERGE_STEP - 1, MERGE_STEP, MERGE_STEP + 1, 2 * MERGE_STEP, 2 * MERGE_STEP + 1])
def test_merge_steps(hb, length):
    """a vertex whose row and column both have `length` entries, overlapping in half of them, the diagonal stored in both"""
    rng = np.random.default_rng(40 + length)
    n = 4 * length + 10
    hub = n // 2
    others = np.setdiff1d(np.arange(n), [hub])
    out = rng.choice(others, length - 1, replace=False)
    both = out[: length // 2]
    inn = np.concatenate([both, rng.choice(np.setdiff1d(others, out), length - 1 - both.size, replace=False)])
    er, ec = rng.integers(0, n, 6 * n), rng.integers(0, n, 6 * n)
    keep = (er != hub) & (ec != hub)
    S = _pattern(n, np.concatenate([np.full(out.size, hub), inn, [hub], er[keep]]), np.concatenate([out, np.full(inn.size, hub), [hub], ec[keep]]))
    T = sp.csc_matrix(S)
    assert S.indptr[hub + 1] - S.indptr[hub] == length and T.indptr[hub + 1] - T.indptr[hub] == length
    _check(hb, S, directed=True, name=("merge", length))


# ---- the thresholds of the enumeration ---------------------------------------------------------------------------------
# K_m: |O(v)| = m - 1 - v takes every value below m, so every threshold on a list's length is met from both sides in one
# graph: a wave's and a workgroup's pivots (WAVE_LEN), lane-walked and wave-walked partners (LANE_LEN) and, from
# m = KEYS + 2 on, a list that does not fit the table
@pytest.mark.parametrize("m", [WAVE_LEN + 1, WAVE_LEN + 2, KEYS + 1, KEYS + 2])
def test_complete_graph(hb, m):
    """K_m (the longest O has m - 1 entries): every lcc = 1, C(m, 3) triangles.  m - 1 = WAVE_LEN: all pivots are waves';
    WAVE_LEN + 1: one workgroup pivot.  m - 1 = KEYS: the longest list fills the table; KEYS + 1: two slices"""
    S = _complete(m)
    assert _olen(S).max() == m - 1
    want = (np.ones(m, F), dict(edges=m * (m - 1) // 2, triangles=m * (m - 1) * (m - 2) // 6, closed=m * (m - 1) * (m - 2),
                                wedges=m * (m - 1) * (m - 2), max_degree=m - 1))
    _check(hb, S, name=("K", m), want=want)


def test_complete_graph_one_way_is_half(hb):
    """K_m with every edge stored one way: every lcc = 1 / 2 under directed = 1; the table in slices"""
    m = KEYS + 40
    S = _complete(m, one_way=True)
    want = (np.full(m, 0.5, F), dict(edges=m * (m - 1) // 2, triangles=m * (m - 1) * (m - 2) // 6, closed=m * (m - 1) * (m - 2) // 2,
                                     wedges=m * (m - 1) * (m - 2), max_degree=m - 1))
    _check(hb, S, directed=True, name=("K one way", m), want=want)


@pytest.mark.parametrize("k", [WAVE_GRID - 1, WAVE_GRID, WAVE_GRID + 1, WAVE_GRID + 4000])
def test_more_wave_tasks_than_waves(hb, k):
    """k disjoint triangles: the lowest vertex of each is the pivot of one wave task with one partner, so there are k tasks,
    and beyond WAVE_GRID a wave takes a second task after its first (its sums start again, its table is built again).
    Every lcc = 1.  Then the same with one direction of half the edges dropped, directed, against the restatement"""
    n = 3 * k
    a = 3 * np.arange(k)
    S = _sym(n, np.concatenate([a, a, a + 1]), np.concatenate([a + 1, a + 2, a + 2]))
    want = (np.ones(n, F), dict(edges=3 * k, triangles=k, closed=6 * k, wedges=6 * k, max_degree=2))
    _check(hb, S, name=("triangles", k), want=want)
    if k != WAVE_GRID + 4000:
        return
    D = _one_way(S, np.random.default_rng(8), 0.5)
    ref = _ref(D)
    assert ref[1]["triangles"] == k and ref[1]["closed"] < 6 * k and set(np.unique(ref[0]).tolist()) == {0.5, 1.0}
    _check(hb, D, directed=True, name=("triangles, one-way edges", k), want=ref)


def test_more_workgroup_tasks_than_workgroups(hb):
    """a clique H of WAVE_LEN + 1 hubs and BLOCK_GRID + 300 vertices joined to all of H: each of those has the WAVE_LEN + 1
    hubs in its O and is the pivot of one workgroup task (its partners: the WAVE_LEN hubs with a non-empty O), so a
    workgroup takes a second task after its first.  The answer is a formula: an outer vertex's neighbours are a clique,
    lcc = 1; a hub has C(h - 1, 2) triangles inside H and (h - 1) m with an outer vertex and another hub"""
    h, m = WAVE_LEN + 1, BLOCK_GRID + 300
    n = h + m
    hr, hc = np.triu_indices(h, 1)
    r = np.concatenate([hr, np.repeat(h + np.arange(m), h)])
    c = np.concatenate([hc, np.tile(np.arange(h), m)])
    S = _sym(n, r, c)
    ol = _olen(S)
    assert (ol[h:] == h).all() and ol[:h].max() == h - 1 and S.nnz > 8 * 10 ** 6
    d_hub = h - 1 + m
    tri_hub = (h - 1) * (h - 2) // 2 + (h - 1) * m
    lcc = np.ones(n, np.float64)
    lcc[:h] = (2.0 * tri_hub) / (float(d_hub) * float(d_hub - 1))
    tri = h * (h - 1) * (h - 2) // 6 + m * (h * (h - 1) // 2)
    wedges = h * d_hub * (d_hub - 1) + m * h * (h - 1)
    want = (lcc.astype(F), dict(edges=h * (h - 1) // 2 + h * m, triangles=tri, closed=6 * tri, wedges=wedges, max_degree=d_hub))
    assert 2 * tri_hub * h + m * h * (h - 1) == 6 * tri
    _check(hb, S, name="hubs and outer vertices", want=want)


def test_complete_bipartite_is_zero(hb):
    a, b = 300, 2 * KEYS + 100                               # the small side's lists: 2 KEYS + 100 entries, three slices
    r = np.repeat(np.arange(a), b)
    c = a + np.tile(np.arange(b), a)
    S = _sym(a + b, r, c)
    want = (np.zeros(a + b, F), dict(edges=a * b, triangles=0, closed=0, wedges=a * b * (b - 1) + b * a * (a - 1), max_degree=b))
    _check(hb, S, name="bipartite", want=want)


def test_dense_core_in_slices(hb):
    """a random dense core whose low-ranked vertices hold lists beyond the table, one-way edges among them"""
    rng = np.random.default_rng(5)
    n = 2400
    r, c = np.triu_indices(n, 1)
    keep = rng.random(r.size) < 0.95
    S = _sym(n, r[keep], c[keep])
    ol = _olen(S)
    assert (ol > KEYS).sum() > 10 and (ol <= KEYS).sum() > 10
    want = _ref(S)
    _check(hb, S, name="core", want=want)
    D = _one_way(S, rng, 0.4)
    _check(hb, D, directed=True, name="core, one-way edges")


@pytest.mark.parametrize("t, chunk", [(4, CHUNK[0]), (WAVE_LEN + 4, CHUNK[1])])
def test_partners_per_task(hb, t, chunk):
    """pivots with chunk - 1, chunk and chunk + 1 partners: a wave's (|O| = 4; 2 chunk + 1 as well) and a workgroup's (|O| =
    WAVE_LEN + 4, partners with lists on both sides of LANE_LEN)"""
    rng = np.random.default_rng(6 + t)
    parts = [chunk - 1, chunk, chunk + 1, chunk // 2] + ([2 * chunk + 1] if t == 4 else [])
    S, mids = _layered(t, [k - (t - 1) for k in parts], max(parts) + 60)
    ol = _olen(S)
    assert all(ol[p] == t for p in mids) and ol[:t].max() == t - 1
    assert (ol[:t] > LANE_LEN).any() == (t > LANE_LEN + 1)
    want = _ref(S)
    _check(hb, S, name=("layered", t), want=want)
    if t == 4:
        _check(hb, _one_way(S, rng, 0.5), directed=True, name=("layered, one-way edges", t))


def test_hub_with_a_sprinkle(hb):
    """a hub joined to a few thousand vertices with a sprinkle of edges among them, and a second hub joined one way"""
    rng = np.random.default_rng(7)
    n = 5000
    r = np.concatenate([np.zeros(n - 1, np.int64), rng.integers(1, n, 12000), np.full(2500, 1)])
    c = np.concatenate([np.arange(1, n), rng.integers(1, n, 12000), rng.choice(np.arange(2, n), 2500, replace=False)])
    S = _sym(n, r, c)
    _check(hb, S, name="hub")
    _check(hb, _one_way(S, rng, 0.6), directed=True, name="hub, one-way edges")


# ---- the library's own triangle count and k-truss ----------------------------------------------------------------------
def test_agrees_with_tc_and_ktruss(hb):
    from graphblast_amd.graphgen import rmat_edges
    g = hb.g
    s, d, n = rmat_edges(12, 8, seed=5)
    S = _sym(n, np.asarray(s), np.asarray(d))
    A = _matrix(g, S, I)
    want = _ref(S)
    _, res = _check(hb, S, A, name="rmat12", want=want)
    desc = hb.descriptor()
    L, B = g.Matrix(n, n, I), g.Matrix(n, n, I)
    assert g.tril(L, A, desc) == 0
    info, ntris, _ = g.tc(L, B, desc)
    assert info == 0 and ntris == res["triangles"]
    T = g.Matrix(n, n, I)
    info, _ = g.ktruss(T, A, 2, desc)
    assert info == 0
    tp, ti, tv = T.host_csr()
    support = np.asarray(sp.csr_matrix((tv.astype(np.int64), ti, tp), shape=(n, n)).sum(axis=1)).ravel()
    assert np.array_equal(support, want[2]) and support.sum() == res["closed"]


# ---- the golden graphs -------------------------------------------------------------------------------------------------
def _golden(name):
    M = sp.csr_matrix(scipy.io.mmread(os.path.join(ROOT, "tests", "golden", "data", name)))
    return _pattern(M.shape[0], M.tocoo().row, M.tocoo().col)


def test_golden_chesapeake(hb):
    M = _golden("chesapeake.mtx")
    co = M.tocoo()
    S = _sym(M.shape[0], co.row, co.col)
    want = _ref(S)
    assert {k: want[1][k] for k in ("triangles", "closed", "wedges", "max_degree")} == dict(triangles=194, closed=1164, wedges=4096, max_degree=33)
    _check(hb, S, name="chesapeake", want=want)
    A = hb.matrix_from_mtx("chesapeake.mtx")                # symmetrised as the loader does
    _check(hb, S, A, name="chesapeake, loaded", want=want)


@pytest.mark.parametrize("name, closed, wedges, triangles", [("test_bc.mtx", 24, 74, 7), ("test_cc.mtx", 30, 90, 9)])
def test_golden_directed(hb, name, closed, wedges, triangles):
    S = _golden(name)
    want = _ref(S)
    assert (want[1]["closed"], want[1]["wedges"], want[1]["triangles"]) == (closed, wedges, triangles)
    _check(hb, S, directed=True, name=name, want=want)


# ---- matrices without a CSC of their own -------------------------------------------------------------------------------
def test_product_result_and_csr_only_format(hb, monkeypatch):
    """directed = 0 reads only the CSR: it works on C = A A of a symmetric A (symmetric again, no CSC of its own) and on a
    matrix of the CSR-only format; directed = 1 is GrB_INVALID_OBJECT on both.  An asymmetric product is taken on the
    caller's word: the call succeeds and stays in bounds"""
    g = hb.g
    rng = np.random.default_rng(12)
    n = 500
    S = _sym(n, rng.integers(0, n, 700), rng.integers(0, n, 700))
    One = _matrix(g, S, F)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", One, One, hb.descriptor()) == 0
    pp, pi, _ = P.host_csr()
    SP = sp.csr_matrix((np.ones(pi.size, np.int64), pi, pp), shape=(n, n))
    assert (SP != SP.T).nnz == 0 and SP.diagonal().sum() > 0
    _check(hb, SP, P, name="product")
    v = g.Vector(n, F)
    assert g.lcc(v, P, None, True)[0] == g.GrB_INVALID_OBJECT
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Q = _matrix(g, S, I)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    _check(hb, S, Q, name="CSR only")
    assert g.lcc(v, Q, None, True)[0] == g.GrB_INVALID_OBJECT
    D = _pattern(n, rng.integers(0, n, 1500), rng.integers(0, n, 1500))
    Dm = _matrix(g, D, F)
    PD = g.Matrix(n, n, F)
    assert g.mxm(PD, None, None, "PlusMultiplies", Dm, Dm, hb.descriptor()) == 0
    info, _ = g.lcc(v, PD, None, False)
    assert info == 0 and v.getStorage() == g.GrB_DENSE


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_lcc_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(13)
    n = 80
    S = _sym(n, rng.integers(0, n, 300), rng.integers(0, n, 300))
    A = _matrix(g, S, F, rng)
    before = rng.random(n).astype(F) + 2
    v = g.Vector(n, F)
    assert v.build(before, n) == 0

    def unchanged():
        return v.getStorage() == g.GrB_DENSE and np.array_equal(v.extractTuples()[1], before)

    call = lambda v_, A_, directed=0: lib.grb_lcc(v_, A_, directed, None, None)
    assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                              # null handles
    assert call(v._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(v._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT             # an unbuilt A
    R = g.Matrix(n, n + 1, F)                                                         # A not square
    assert R.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)) == 0
    assert call(v._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Vector(n + 1, F)._h, A._h) == g.GrB_DIMENSION_MISMATCH              # size(lcc) != n
    for directed in (2, -1):
        assert call(v._h, A._h, directed) == g.GrB_INVALID_VALUE
    assert unchanged()
    iv = g.Vector(n, I)                                                               # types
    assert iv.build(np.arange(n, dtype=I), n) == 0
    assert call(iv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(iv.extractTuples()[1], np.arange(n))
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
    assert call(v._h, P._h, 1) == g.GrB_INVALID_OBJECT
    assert unchanged()
    D = _pattern(n, rng.integers(0, n, 300), rng.integers(0, n, 300))                 # an asymmetric A, undirected
    assert (D != D.T).nnz > 0
    Dm = _matrix(g, D, F)
    assert call(v._h, Dm._h, 0) == g.GrB_INVALID_VALUE
    assert unchanged()
    sv = g.Vector(n, F)                                                               # ... and a sparse lcc stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], F), 2, None) == 0
    assert call(sv._h, Dm._h, 0) == g.GrB_INVALID_VALUE
    assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
    info, si, sx = sv.extractTuples(sparse=True)
    assert info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]
    assert call(v._h, Dm._h, 1) == 0 and not unchanged()                              # the same matrix, directed: fine
    # a descriptor and a null descriptor give the same result; the record is optional
    w = g.Vector(n, F)
    assert lib.grb_lcc(w._h, A._h, 0, hb.descriptor()._h, None) == 0
    assert call(v._h, A._h) == 0
    assert np.array_equal(v.extractTuples()[1].view(np.uint32), w.extractTuples()[1].view(np.uint32))
    assert np.array_equal(w.extractTuples()[1].view(np.uint32), _ref(S)[0].view(np.uint32))


# ---- degenerate shapes, lcc's storage beforehand -----------------------------------------------------------------------
def test_degenerate(hb):
    g = hb.g
    zero = dict(edges=0, triangles=0, closed=0, wedges=0, max_degree=0)
    for n, S in ((1, _sym(1, [], [])), (1, _sym(1, [], [], [0])), (50, _sym(50, [], [])), (50, _sym(50, [], [], np.arange(0, 50, 3)))):
        for directed in (False, True):
            _, res = _check(hb, S, directed=directed, name=("degenerate", n, directed), want=(np.zeros(n, F), zero))
            assert res["loop_ms"] == 0 or S.nnz > 0
    S = _sym(300, [3, 5, 3, 7], [5, 7, 7, 200])               # one triangle among 300 vertices, and one pendant edge
    got, res = _check(hb, S, name="one triangle")
    assert res["triangles"] == 1 and got[3] == 1 and got[7] == F(1 / 3) and got[200] == 0
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    v0 = g.Vector(0, F)
    info, res = g.lcc(v0, A0, None, False)
    assert info == 0 and all(res[k] == 0 for k in REC)


def test_lcc_sparse_or_dense_beforehand(hb):
    g = hb.g
    rng = np.random.default_rng(14)
    n = 400
    S = _sym(n, rng.integers(0, n, 3000), rng.integers(0, n, 3000))
    A = _matrix(g, S, F)
    want = _ref(S)
    dense = g.Vector(n, F)
    assert dense.build(np.full(n, 9, F), n) == 0
    sparse = g.Vector(n, F)
    assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], F), 3, None) == 0
    for name, v in (("dense", dense), ("sparse", sparse), ("fresh", g.Vector(n, F))):
        _check(hb, S, A, name=name, want=want, v=v)


def test_lcc_on_caller_owned_storage(hb):
    """lcc adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards around it"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(15)
    n = 1003
    S = _sym(n, rng.integers(0, n, 9000), rng.integers(0, n, 9000))
    A = _matrix(g, S, F)
    want = _ref(S)
    for k in ad.KS:
        v, t, check = ad.adopt_dense(g, np.full(n, 77, F), k)
        assert v.device_ptrs()[2] % 16 == 4 * k
        got, _ = _check(hb, S, A, name=("adopted", k), want=want, v=v)
        assert np.array_equal(ad.payload(t, k, n, F).view(np.uint32), want[0].view(np.uint32))
        check(("lcc", k))


# ---- determinism, relabelling ------------------------------------------------------------------------------------------
def test_determinism_and_relabelling(hb):
    from graphblast_amd.graphgen import rmat_edges
    g = hb.g
    s, d, n = rmat_edges(13, 8, seed=6)
    s, d = np.asarray(s), np.asarray(d)
    rng = np.random.default_rng(16)
    D = _pattern(n, s, d)                                   # as drawn: directed
    assert _olen(sp.csr_matrix(_sym(n, s, d))).max() > LANE_LEN
    want = _ref(D)
    A = _matrix(g, D, F)
    outs = []
    for _ in range(2):
        got, res = _check(hb, D, A, directed=True, name="rmat13, as drawn", want=want)
        outs.append((got.tobytes(), [res[k] for k in REC]))
    assert outs[0] == outs[1]
    perm = rng.permutation(n)                               # vertex v becomes perm[v]
    Dp = _pattern(n, perm[s], perm[d])
    gotp, resp = _check(hb, Dp, directed=True, name="relabelled")
    assert np.array_equal(gotp[perm].view(np.uint32), got.view(np.uint32)) and [resp[k] for k in REC] == outs[0][1]


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def test_cpp_frontend(tmp_path):
    """tests/tools/lcc.cpp: two triangles and a bridge undirected, a small directed graph, a NULL descriptor"""
    exe = str(tmp_path / "lcc")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "lcc.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln.split(" ")[0] in ("und", "rec", "dir", "drec", "asym")]
    S = _sym(7, [0, 0, 1, 3, 3, 4, 2], [1, 2, 2, 4, 5, 5, 3])
    lcc, rec = _ref(S)[:2]
    D = _pattern(5, [0, 1, 1, 2, 0, 3, 3], [1, 0, 2, 0, 3, 1, 3])
    dl, drec = _ref(D)[:2]
    assert drec["triangles"] == 2 and drec["closed"] > 0

    def line(tag, vals, rec_tag, r):
        return [tag + " " + " ".join("%08x" % int(x) for x in np.asarray(vals, F).view(np.uint32)),
                rec_tag + " " + " ".join(str(r[k]) for k in REC)]

    assert lines == line("und", lcc, "rec", rec) + line("dir", dl, "drec", drec) + ["asym 1"], lines
