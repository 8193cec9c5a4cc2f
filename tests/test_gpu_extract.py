"""extract on the device (csrc/extract.hip): the submatrix C = op(A)(I, J), the column w = op(A)(I, j) and the subvector
w = u(I) against a numpy restatement of the definition -- ordered, permuted, repeated and null lists, rows in every bin,
RMAT hub rows against scipy, both orientations of the result, downstream traversals and products on a result, aliasing,
every error code with the output unchanged, the INT32_MAX guard and the C++ frontend.  Nothing is computed, only copied:
every comparison is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


def _rand_csr(rng, m, n, nnz):
    """m x n, sorted rows, no duplicates"""
    key = np.unique(rng.integers(0, m, nnz).astype(np.int64) * n + rng.integers(0, n, nnz))
    ptr = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(key // n, minlength=m), out=ptr[1:])
    return ptr, (key % n).astype(np.int32)


def _transpose(m, n, p, i, v):
    """the n x m transpose of an m x n CSR (rows ascending within every column)"""
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(p))
    order = np.lexsort((rows, i))
    tp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(i, minlength=n), out=tp[1:])
    return tp, rows[order].astype(np.int32), v[order]


def _vals(rng, size, dt):
    return rng.integers(0, 5, size).astype(dt)           # a fifth of the stored values are zeros: kept


def _mat(g, m, n, p, i, v):
    M = g.Matrix(m, n, v.dtype)
    assert M.build_csr(p, i, v) == 0
    return M


def _stored(g, m, n, p, i, v, tran):
    """the matrix whose op() under `tran` is the m x n (p, i, v)"""
    return _mat(g, n, m, *_transpose(m, n, p, i, v)) if tran else _mat(g, m, n, p, i, v)


def _desc(hb, tran=False):
    d = hb.descriptor()
    if tran:
        assert d.toggle(hb.g.GrB_INP0) == 0
    return d


def _expect(m, n, p, i, v, rows, cols):
    """C = X(rows, cols) of the m x n CSR X by the definition: for every output row, every stored column of its source
    row yields the places of that column in `cols`; the row is then sorted by output column.  None: all, in order."""
    rows = np.arange(m, dtype=np.int64) if rows is None else np.asarray(rows, np.int64)
    cols = np.arange(n, dtype=np.int64) if cols is None else np.asarray(cols, np.int64)
    jpos = np.argsort(cols, kind="stable")
    jptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(cols, minlength=n), out=jptr[1:])
    cp = np.zeros(rows.size + 1, np.int64)
    ci, cv = [], []
    for k, r in enumerate(rows):
        sc, sv = i[p[r]:p[r + 1]], v[p[r]:p[r + 1]]
        cnt = jptr[sc + 1] - jptr[sc]
        tot = int(cnt.sum())
        at = np.repeat(jptr[sc] - (np.cumsum(cnt) - cnt), cnt) + np.arange(tot)
        oc, ov = jpos[at], np.repeat(sv, cnt)
        o = np.argsort(oc, kind="stable")
        ci.append(oc[o])
        cv.append(ov[o])
        cp[k + 1] = cp[k] + tot
    ci = np.concatenate(ci) if ci else np.zeros(0, np.int64)
    cv = np.concatenate(cv) if cv else np.zeros(0, v.dtype)
    return cp.astype(np.int32), ci.astype(np.int32), cv.astype(v.dtype)


def _same(got, want, name=""):
    for x, y in zip(got, want):
        assert x.shape == y.shape, (name, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint32) if x.dtype != np.int32 else x, y.view(np.uint32) if y.dtype != np.int32 else y), name


def _check_csc(C, m, n, name=""):
    """C's CSC holds the same entries and bits as the transpose of its CSR"""
    p, i, v = C.host_csr()
    _same(C.host_csc(), _transpose(m, n, p, i, v), name)


def _lists(rng, dim):
    k = max(dim // 2, 1)
    return {"ascending": np.sort(rng.choice(dim, k, replace=False)).astype(np.int32),
            "permuted": rng.permutation(dim).astype(np.int32),
            "duplicates": rng.integers(0, dim, dim + 37).astype(np.int32),
            "null": None}


def _len(lst, dim):
    return dim if lst is None else len(lst)


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("tran", [False, True])
def test_every_list_shape_and_orientation(hb, dt, tran):
    """f32 and i32, INP0 default and TRAN, four list shapes for the rows and the columns independently, a rectangular A
    with stored zeros: C's CSR is the definition's, its CSC the exact transpose of that"""
    g = hb.g
    rng = np.random.default_rng(41)
    m, n = 150, 230
    ap, ai = _rand_csr(rng, m, n, 4000)
    av = _vals(rng, ai.size, dt)
    assert (av == 0).any()
    A = _stored(g, m, n, ap, ai, av, tran)
    d = _desc(hb, tran)
    for rname, rows in _lists(rng, m).items():
        for cname, cols in _lists(rng, n).items():
            Cm = g.Matrix(_len(rows, m), _len(cols, n), dt)
            assert g.extract(Cm, None, None, A, rows, cols, d) == 0, (rname, cname)
            _same(Cm.host_csr(), _expect(m, n, ap, ai, av, rows, cols), (rname, cname))
            _check_csc(Cm, _len(rows, m), _len(cols, n), (rname, cname))


def test_rows_in_every_bin(hb):
    """source rows of 0, 1, 15, 16, 17, 63, 64, 65, 1023, 1025 and 70000 entries (the 16-lane groups, a wave per row, hub
    rows in 1024-entry segments), the longest selected three times; ordered, repeated and null column lists"""
    g = hb.g
    rng = np.random.default_rng(43)
    lens = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1025, 70000]
    n = 90000
    lists = [np.sort(rng.choice(n, k, replace=False)).astype(np.int32) for k in lens]
    ap = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=ap[1:])
    ai = np.concatenate(lists)
    for dt in (F, I):
        av = _vals(rng, ai.size, dt)
        A = _mat(g, len(lens), n, ap, ai, av)
        rows = np.r_[rng.permutation(len(lens)), 10, 3, 10].astype(np.int32)
        assert (rows == 10).sum() == 3
        col_lists = {"null": None,
                     "ascending": np.sort(rng.choice(n, n // 3, replace=False)).astype(np.int32),
                     "ascending duplicates": np.sort(rng.integers(0, n, n // 2)).astype(np.int32),
                     "unordered duplicates": rng.integers(0, n, 50000).astype(np.int32)}
        for name, cols in col_lists.items():
            Cm = g.Matrix(rows.size, _len(cols, n), dt)
            assert g.extract(Cm, None, None, A, rows, cols, hb.descriptor()) == 0, name
            _same(Cm.host_csr(), _expect(len(lens), n, ap, ai, av, rows, cols), name)
            _check_csc(Cm, rows.size, _len(cols, n), name)


def _rmat(scale, seed, symmetrize=True):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=symmetrize)
    ptr, ind = (x.cpu().numpy().astype(np.int32) for x in gr["csr"])
    return n, ptr, ind


def _scipy_sub(S, rows, cols):
    W = S[rows][:, cols].tocsr()
    W.sort_indices()
    return W


def test_rmat16_against_scipy(hb):
    """RMAT-16, hub rows included: the induced subgraph of a quarter of the vertices, A(p, p) for a random permutation
    (BFS labels and mxv on it are A's, permuted), and A(ALL, ALL) = A in both orientations"""
    import scipy.sparse as sp
    g = hb.g
    n, ap, ai = _rmat(16, 5)
    assert np.diff(ap).max() > 4 * 1024                                  # hub rows of several segments
    rng = np.random.default_rng(16)
    av = rng.integers(1, 4, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    S = sp.csr_matrix((av, ai, ap), shape=(n, n))
    # the induced subgraph
    sub = np.sort(rng.choice(n, n // 4, replace=False)).astype(np.int32)
    Cs = g.Matrix(sub.size, sub.size, F)
    assert g.extract(Cs, None, None, A, sub, sub, hb.descriptor()) == 0
    W = _scipy_sub(S, sub, sub)
    _same(Cs.host_csr(), (W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data.astype(F)), "induced")
    _check_csc(Cs, sub.size, sub.size, "induced")
    # a relabelling
    p = rng.permutation(n).astype(np.int32)
    Cp = g.Matrix(n, n, F)
    assert g.extract(Cp, None, None, A, p, p, hb.descriptor()) == 0
    W = _scipy_sub(S, p, p)
    _same(Cp.host_csr(), (W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data.astype(F)), "permuted")
    _check_csc(Cp, n, n, "permuted")
    pinv = np.empty(n, np.int64)
    pinv[p] = np.arange(n)
    for s in (int(np.argmax(np.diff(ap))), int(np.nonzero(np.diff(ap))[0][11])):
        labels = []
        for X, src in ((A, s), (Cp, int(pinv[s]))):
            v = g.Vector(n)
            info, _ = g.bfs(v, X, src, hb.descriptor(mxvmode=0, struconly=1), fused=True)
            assert info == 0
            labels.append(v.extractTuples()[1])
        assert np.array_equal(labels[1], labels[0][p]), s
    u = rng.integers(0, 4, n).astype(F)
    for mode in (1, 2):
        uv, w = g.Vector(n, F), g.Vector(n, F)
        assert uv.build(u[p], n) == 0
        assert g.mxv(w, None, None, "PlusMultiplies", Cp, uv, hb.descriptor(mxvmode=mode)) == 0
        assert np.array_equal(hb.dense_values(w).astype(np.float64), (S @ u.astype(np.float64))[p]), mode
    # everything
    Ca = g.Matrix(n, n, F)
    assert g.extract(Ca, None, None, A, None, None, hb.descriptor()) == 0
    _same(Ca.host_csr(), (ap, ai, av), "all")
    _same(Ca.host_csc(), A.host_csc(), "all")


def test_csr_only_input(hb):
    """a product result has no CSC: its extract is CSR only, its transposed extract GrB_INVALID_OBJECT until
    grb_transpose under INP0 = TRAN has given it both orientations"""
    g = hb.g
    rng = np.random.default_rng(9)
    n = 200
    ap, ai = _rand_csr(rng, n, n, 1500)
    av = rng.integers(1, 3, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    pp, pi, pv = (x.copy() for x in P.host_csr())
    rows, cols = rng.permutation(n)[:120].astype(np.int32), rng.integers(0, n, 90).astype(np.int32)
    Cm = g.Matrix(120, 90, F)
    assert g.extract(Cm, None, None, P, rows, cols, hb.descriptor()) == 0
    _same(Cm.host_csr(), _expect(n, n, pp, pi, pv, rows, cols))
    with pytest.raises(g._lib.GrbError) as e:
        Cm.host_csc()
    assert e.value.info == g.GrB_NO_VALUE
    kept = [x.copy() for x in Cm.host_csr()]
    assert g.extract(Cm, None, None, P, rows, cols, _desc(hb, True)) == g.GrB_INVALID_OBJECT
    _same(Cm.host_csr(), kept)
    w = g.Vector(120, F)
    assert g.extract(w, None, None, P, rows, 3, hb.descriptor()) == g.GrB_INVALID_OBJECT   # a column needs the CSC
    Q = g.Matrix(n, n, F)
    assert g.transpose(Q, None, None, P, _desc(hb, True)) == 0
    Ct = g.Matrix(120, 90, F)
    assert g.extract(Ct, None, None, Q, rows, cols, _desc(hb, True)) == 0
    _same(Ct.host_csr(), _expect(n, n, *_transpose(n, n, pp, pi, pv), rows, cols))
    _check_csc(Ct, 120, 90)


def test_chaining(hb):
    """the extract of an eWiseAdd result as an operand of mxm and of transpose"""
    import scipy.sparse as sp
    g = hb.g
    rng = np.random.default_rng(21)
    m, n = 180, 160
    (ap, ai), (bp, bi) = _rand_csr(rng, m, n, 3000), _rand_csr(rng, m, n, 3000)
    av, bv = rng.integers(1, 4, ai.size).astype(F), rng.integers(1, 4, bi.size).astype(F)
    A, B = _mat(g, m, n, ap, ai, av), _mat(g, m, n, bp, bi, bv)
    E = g.Matrix(m, n, F)
    assert g.eWiseAdd(E, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
    rows, cols = rng.permutation(m)[:100].astype(np.int32), np.sort(rng.choice(n, 70, replace=False)).astype(np.int32)
    X = g.Matrix(100, 70, F)
    assert g.extract(X, None, None, E, rows, cols, hb.descriptor()) == 0
    SE = (sp.csr_matrix((av, ai, ap), shape=(m, n)) + sp.csr_matrix((bv, bi, bp), shape=(m, n))).tocsr()
    W = _scipy_sub(SE, rows, cols)
    _same(X.host_csr(), (W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data.astype(F)))
    P = g.Matrix(100, 100, F)
    assert g.mxm(P, None, None, "PlusMultiplies", X, X, _desc_inp1(hb)) == 0       # X . X^T
    WP = (W @ W.T).tocsr()
    WP.sort_indices()
    _same(P.host_csr(), (WP.indptr.astype(np.int32), WP.indices.astype(np.int32), WP.data.astype(F)))
    T = g.Matrix(70, 100, F)
    assert g.transpose(T, None, None, X, hb.descriptor()) == 0
    WT = W.T.tocsr()
    WT.sort_indices()
    _same(T.host_csr(), (WT.indptr.astype(np.int32), WT.indices.astype(np.int32), WT.data.astype(F)))


def _desc_inp1(hb):
    d = hb.descriptor()
    assert d.toggle(hb.g.GrB_INP1) == 0
    return d


def test_aliasing(hb):
    """C is A for the submatrix, w is u for the subvector (dense and sparse)"""
    g = hb.g
    rng = np.random.default_rng(12)
    n = 140
    ap, ai = _rand_csr(rng, n, n, 3000)
    av = _vals(rng, ai.size, F)
    for rows, cols in ((rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)),
                       (rng.integers(0, n, n).astype(np.int32), None)):
        A = _mat(g, n, n, ap, ai, av)
        assert g.extract(A, None, None, A, rows, cols, hb.descriptor()) == 0
        _same(A.host_csr(), _expect(n, n, ap, ai, av, rows, cols))
        _check_csc(A, n, n)
    idx = rng.integers(0, n, n).astype(np.int32)
    vals = rng.integers(0, 9, n).astype(F)
    u = g.Vector(n, F)
    assert u.build(vals, n) == 0
    assert g.extract(u, None, None, u, idx, None, hb.descriptor()) == 0
    assert u.getStorage() == g.GrB_DENSE
    assert np.array_equal(hb.dense_values(u).view(np.uint32), vals[idx].view(np.uint32))
    si = np.sort(rng.choice(n, 50, replace=False)).astype(np.int32)
    sv = rng.integers(0, 9, 50).astype(F)
    s = g.Vector(n, F)
    assert s.build(si, sv, 50, None) == 0
    assert g.extract(s, None, None, s, idx, None, hb.descriptor()) == 0
    wi, wv = _expect_sparse(si, sv, idx)
    assert s.getStorage() == g.GrB_SPARSE and s.nvals() == wi.size
    gi, gv = hb.sparse_tuples(s)
    assert np.array_equal(gi, wi) and np.array_equal(gv.view(np.uint32), wv.view(np.uint32))


def _expect_sparse(l_ind, l_val, idx):
    """entries k where idx[k] is in the ascending list (l_ind, l_val)"""
    idx = np.asarray(idx, np.int64)
    at = np.searchsorted(l_ind, idx)
    hit = (at < l_ind.size) & (l_ind[np.minimum(at, max(l_ind.size - 1, 0))] == idx) if l_ind.size else np.zeros(idx.size, bool)
    return np.nonzero(hit)[0].astype(np.int32), l_val[at[hit]]


@pytest.mark.parametrize("dt", [F, I])
def test_column_form(hb, dt):
    """a column of A through its CSC and a row under INP0 = TRAN; I ascending, permuted, with duplicates and null; an
    empty column; w sparse, indices ascending, the right nvals"""
    g = hb.g
    rng = np.random.default_rng(33)
    m, n = 300, 170
    ap, ai = _rand_csr(rng, m, n, 9000)
    keep = ai != 5                                                          # column 5 is empty
    ap = np.r_[0, np.cumsum(np.bincount(np.repeat(np.arange(m), np.diff(ap))[keep], minlength=m))].astype(np.int32)
    ai = ai[keep]
    av = _vals(rng, ai.size, dt)
    A = _mat(g, m, n, ap, ai, av)
    tp, ti, tv = _transpose(m, n, ap, ai, av)
    for tran in (False, True):
        dim, other = (n, m) if tran else (m, n)                             # op(A) is dim x other
        xp, xi, xv = (ap, ai, av) if tran else (tp, ti, tv)                 # column j of op(A): row j of this
        for j in (0, 5, 17, other - 1):
            li, lv = xi[xp[j]:xp[j + 1]], xv[xp[j]:xp[j + 1]]
            for name, rows in _lists(rng, dim).items():
                w = g.Vector(_len(rows, dim), dt)
                assert g.extract(w, None, None, A, rows, j, _desc(hb, tran)) == 0, (tran, j, name)
                wi, wv = _expect_sparse(li, lv, np.arange(dim) if rows is None else rows)
                assert w.getStorage() == g.GrB_SPARSE and w.nvals() == wi.size, (tran, j, name)
                gi, gv = hb.sparse_tuples(w)
                assert np.array_equal(gi, wi) and np.array_equal(gv.view(np.uint32), wv.view(np.uint32)), (tran, j, name)
                assert (np.diff(gi) > 0).all()
    w = g.Vector(m, dt)
    assert g.extract(w, None, None, A, None, 5, hb.descriptor()) == 0 and w.nvals() == 0


@pytest.mark.parametrize("dt", [F, I])
def test_subvector_form(hb, dt):
    """a dense u gives a dense w = u[I], a sparse u a sparse w; a permutation, duplicates and null"""
    g = hb.g
    rng = np.random.default_rng(35)
    n = 5000
    vals = rng.integers(0, 100, n).astype(dt)
    si = np.sort(rng.choice(n, 700, replace=False)).astype(np.int32)
    sv = rng.integers(0, 5, 700).astype(dt)
    for name, idx in _lists(rng, n).items():
        k = _len(idx, n)
        u, w = g.Vector(n, dt), g.Vector(k, dt)
        assert u.build(vals, n) == 0
        assert g.extract(w, None, None, u, idx, None, hb.descriptor()) == 0, name
        assert w.getStorage() == g.GrB_DENSE and w.size() == k
        assert np.array_equal(hb.dense_values(w), vals if idx is None else vals[idx]), name
        s, ws = g.Vector(n, dt), g.Vector(k, dt)
        assert s.build(si, sv, 700, None) == 0
        assert g.extract(ws, None, None, s, idx, None, hb.descriptor()) == 0, name
        wi, wv = _expect_sparse(si, sv, np.arange(n) if idx is None else idx)
        assert ws.getStorage() == g.GrB_SPARSE and ws.nvals() == wi.size, name
        gi, gv = hb.sparse_tuples(ws)
        assert np.array_equal(gi, wi) and np.array_equal(gv, wv), name


def _arr(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data


def test_errors_leave_the_output_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(4)
    m, n = 100, 80
    ap, ai = _rand_csr(rng, m, n, 1500)
    av = _vals(rng, ai.size, F)
    A = _mat(g, m, n, ap, ai, av)
    rows, cols = rng.integers(0, m, 60).astype(np.int32), rng.permutation(n)[:50].astype(np.int32)
    Cm = g.Matrix(60, 50, F)
    d = hb.descriptor()
    assert g.extract(Cm, None, None, A, rows, cols, d) == 0
    before = [x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()]

    def unchanged():
        return all(np.array_equal(x, y) for x, y in zip(before, list(Cm.host_csr()) + list(Cm.host_csc())))

    (_, rp), (_, cp) = _keep = _arr(rows), _arr(cols)
    call = lambda C_, A_, r, nr, c, nc, mask=None: lib.grb_matrix_extract(C_, mask, 0, A_, r, nr, c, nc, d._h)
    assert call(None, A._h, rp, 60, cp, 50) == g.GrB_UNINITIALIZED_OBJECT
    assert call(Cm._h, None, rp, 60, cp, 50) == g.GrB_UNINITIALIZED_OBJECT
    assert g.extract(Cm, None, None, g.Matrix(m, n, F), rows, cols, d) == g.GrB_UNINITIALIZED_OBJECT   # unbuilt
    assert g.extract(Cm, A, None, A, rows, cols, d) == g.GrB_NOT_IMPLEMENTED                           # a mask
    Ai = _mat(g, m, n, ap, ai, av.astype(I))
    assert g.extract(Cm, None, None, Ai, rows, cols, d) == g.GrB_NOT_IMPLEMENTED                       # C of another type
    assert g.extract(Cm, None, None, A, rows[:59], cols, d) == g.GrB_DIMENSION_MISMATCH
    assert g.extract(Cm, None, None, A, rows, np.r_[cols, 1], d) == g.GrB_DIMENSION_MISMATCH
    assert g.extract(Cm, None, None, A, None, cols, d) == g.GrB_DIMENSION_MISMATCH                     # C has 60 rows, A 100
    assert call(Cm._h, A._h, None, 60, cp, 50) == g.GrB_DIMENSION_MISMATCH                             # a null list of 60 != 100
    assert call(Cm._h, A._h, rp, 60, None, 50) == g.GrB_DIMENSION_MISMATCH
    assert g.extract(Cm, None, None, A, rows, cols, _desc(hb, True)) == g.GrB_INDEX_OUT_OF_BOUNDS      # rows address A^T's 80
    for bad in (-1, m):
        r2 = rows.copy()
        r2[59] = bad
        assert g.extract(Cm, None, None, A, r2, cols, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    for bad in (-1, n):
        c2 = cols.copy()
        c2[0] = bad
        assert g.extract(Cm, None, None, A, rows, c2, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    assert unchanged()
    # counts of zero: empty results of that shape
    Z = g.Matrix(0, 50, F)
    assert g.extract(Z, None, None, A, [], cols, d) == 0 and Z.nvals() == 0
    Z = g.Matrix(60, 0, F)
    assert g.extract(Z, None, None, A, rows, [], d) == 0 and Z.nvals() == 0
    assert np.array_equal(Z.host_csr()[0], np.zeros(61, np.int32))
    assert g.extract(Cm, None, None, A, [], cols, d) == g.GrB_DIMENSION_MISMATCH
    assert unchanged()

    # the column form
    w = g.Vector(60, F)
    assert g.extract(w, None, None, A, rows, 7, d) == 0
    kept = (w.getStorage(), *[x.copy() for x in hb.sparse_tuples(w)])

    def w_unchanged(v=w, kept=kept):
        return v.getStorage() == kept[0] and all(np.array_equal(x, y) for x, y in zip(kept[1:], hb.sparse_tuples(v)))

    colcall = lambda w_, A_, r, nr, j, mask=None: lib.grb_matrix_extract_col(w_, mask, 0, A_, r, nr, j, d._h)
    assert colcall(None, A._h, rp, 60, 7) == g.GrB_UNINITIALIZED_OBJECT
    assert colcall(w._h, None, rp, 60, 7) == g.GrB_UNINITIALIZED_OBJECT
    assert g.extract(w, None, None, g.Matrix(m, n, F), rows, 7, d) == g.GrB_UNINITIALIZED_OBJECT
    assert g.extract(w, w, None, A, rows, 7, d) == g.GrB_NOT_IMPLEMENTED
    assert g.extract(w, None, None, Ai, rows, 7, d) == g.GrB_NOT_IMPLEMENTED
    assert g.extract(w, None, None, A, rows[:10], 7, d) == g.GrB_DIMENSION_MISMATCH
    assert colcall(w._h, A._h, None, 60, 7) == g.GrB_DIMENSION_MISMATCH
    for bad in (-1, n):
        assert g.extract(w, None, None, A, rows, bad, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    r2 = rows.copy()
    r2[3] = m
    assert g.extract(w, None, None, A, r2, 7, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    assert w_unchanged()
    z = g.Vector(0, F)
    assert g.extract(z, None, None, A, [], 7, d) == 0 and z.nvals() == 0

    # the subvector form
    u = g.Vector(m, F)
    assert u.build(np.arange(m, dtype=F), m) == 0
    x = g.Vector(60, F)
    assert g.extract(x, None, None, u, rows, None, d) == 0
    xk = hb.dense_values(x).copy()
    subcall = lambda w_, u_, r, nr, mask=None: lib.grb_vector_extract(w_, mask, 0, u_, r, nr, d._h)
    assert subcall(None, u._h, rp, 60) == g.GrB_UNINITIALIZED_OBJECT
    assert subcall(x._h, None, rp, 60) == g.GrB_UNINITIALIZED_OBJECT
    assert g.extract(x, None, None, g.Vector(m, F), rows, None, d) == g.GrB_UNINITIALIZED_OBJECT        # no storage yet
    assert g.extract(x, x, None, u, rows, None, d) == g.GrB_NOT_IMPLEMENTED
    assert g.extract(x, None, None, u, rows[:10], None, d) == g.GrB_DIMENSION_MISMATCH
    assert subcall(x._h, u._h, None, 60) == g.GrB_DIMENSION_MISMATCH
    for bad in (-1, m):
        r2 = rows.copy()
        r2[0] = bad
        assert g.extract(x, None, None, u, r2, None, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    assert x.getStorage() == g.GrB_DENSE and np.array_equal(hb.dense_values(x), xk)
    z = g.Vector(0, F)
    assert g.extract(z, None, None, u, [], None, d) == 0 and z.getStorage() == g.GrB_DENSE
    # a null descriptor means the defaults
    Cn = g.Matrix(60, 50, F)
    assert g.extract(Cn, None, None, A, rows, cols, None) == 0
    _same(Cn.host_csr(), before[:3])


def test_int32_max_guard(hb):
    """one 65536-entry row selected 40000 times with every column: 2.6e9 entries -> GrB_OUT_OF_MEMORY before anything of C
    is allocated; C unchanged, the device's free memory where it was"""
    import torch
    g = hb.g
    k = 1 << 16
    A = _mat(g, 1, k, np.array([0, k], np.int32), np.arange(k, dtype=np.int32), np.ones(k, F))
    rows = np.zeros(40000, np.int32)
    Cm = _mat(g, 40000, k, np.r_[np.zeros(40000, np.int32), 1].astype(np.int32), np.array([5], np.int32), np.array([2], F))
    kept = [x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()]
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    assert g.extract(Cm, None, None, A, rows, None, hb.descriptor()) == g.GrB_OUT_OF_MEMORY
    free1 = torch.cuda.mem_get_info()[0]
    assert abs(free1 - free0) <= 8 << 20, (free0, free1)
    assert all(np.array_equal(x, y) for x, y in zip(kept, list(Cm.host_csr()) + list(Cm.host_csc())))
    # the same through duplicates in J: known only after the symbolic pass
    assert g.extract(Cm, None, None, A, rows, np.tile(np.arange(2, dtype=np.int32), k // 2), hb.descriptor()) == g.GrB_OUT_OF_MEMORY
    assert all(np.array_equal(x, y) for x, y in zip(kept, list(Cm.host_csr()) + list(Cm.host_csc())))


def test_determinism(hb):
    """an unordered J with duplicates (the sorted path): two calls, the same bits in both orientations"""
    g = hb.g
    n, ap, ai = _rmat(13, 8)
    rng = np.random.default_rng(3)
    av = _vals(rng, ai.size, F)
    A = _mat(g, n, n, ap, ai, av)
    rows, cols = rng.integers(0, n, n).astype(np.int32), rng.integers(0, n, n + 100).astype(np.int32)
    outs = []
    for _ in range(2):
        Cm = g.Matrix(n, n + 100, F)
        assert g.extract(Cm, None, None, A, rows, cols, hb.descriptor()) == 0
        outs.append([x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()])
    _same(outs[0], outs[1])
    _same(outs[0][:3], _expect(n, n, ap, ai, av, rows, cols))


def test_cpp_frontend(tmp_path):
    """tests/tools/extract.cpp: the three overloads on a 4 x 4 literal"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "extract")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "extract.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln[:3] in ("csr", "csc", "col", "row", "sub")]
    # A = [[1 . 2 .] [. 3 . .] [4 . 5 6] [. 0 . 7]]; C = A({2, 0, 2}, {3, 0}) = [[6 4] [. 1] [6 4]]
    assert lines == ["csr 3 2 5 | 0 2 3 5 | 0 1 1 0 1 | 6 4 1 6 4",
                     "csc 3 2 5 | 0 2 5 | 0 2 0 1 2 | 6 6 4 1 4",
                     "col 3 | 0 2 3 | 4 1 1",           # column 0 at rows {2, 1, 0, 0}
                     "row 3 | 0 2 3 | 4 5 6",           # row 2, every column
                     "sub 3 | | 13 13 10"], lines
