"""assign into a matrix on the device (csrc/assign_matrix.hip): C(I, J) = A, C(I, j) = u, C(i, J) = u and C(I, J) = val
against a numpy restatement of GraphBLAS's GrB_assign without GrB_REPLACE -- every list shape, deletion inside the region,
rows in every bin of the merge, masks, the round trip through extract, RMAT hub rows against scipy, CSR-only operands,
aliasing, every error code with C unchanged, the INT32_MAX guard, determinism and the C++ frontend.  Every comparison is
bit-exact."""
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


# ---- the definition, on dense (presence, value) arrays
def _dense(m, n, p, i, v):
    pres = np.zeros((m, n), bool)
    val = np.zeros((m, n), v.dtype)
    r = np.repeat(np.arange(m), np.diff(p))
    pres[r, i] = True
    val[r, i] = v
    return pres, val


def _csr(pres, val):
    p = np.zeros(pres.shape[0] + 1, np.int32)
    np.cumsum(pres.sum(axis=1), out=p[1:])
    r, c = np.nonzero(pres)                                # row-major: columns ascending in every row
    return p, c.astype(np.int32), val[r, c]


def _accum(name, c, t):
    with np.errstate(all="ignore"):
        return {"plus": lambda: c + t, "first": lambda: c, "second": lambda: t, "minus": lambda: c - t,
                "multiplies": lambda: c * t, "minimum": lambda: np.minimum(c, t), "maximum": lambda: np.maximum(c, t)}[name]()


def _ref(C, T, rows, cols, accum=None, mask=None, scmp=False):
    """C, T: (presence, value) of C's shape; rows / cols: the region's lists (None: all); mask: (presence, value) or None"""
    cp, cv = C
    tp, tv = T
    m, n = cp.shape
    rows = np.arange(m) if rows is None else np.asarray(rows, np.int64)
    cols = np.arange(n) if cols is None else np.asarray(cols, np.int64)
    R = np.zeros((m, n), bool)
    R[np.ix_(rows, cols)] = True
    zp = tp | (cp & (~R | (accum is not None)))
    zv = np.where(tp, tv, cv)
    if accum is not None:
        zv = np.where(tp & cp, _accum(accum, cv, tv).astype(cv.dtype), zv)
    if mask is not None:
        ok = (mask[0] & (mask[1] != 0)) != scmp
        zp, zv = np.where(ok, zp, cp), np.where(ok, zv, cv)
    return zp, np.where(zp, zv, 0).astype(cv.dtype)


def _place(m, n, A, rows, cols):
    """T of the matrix form: A (presence, value) of shape len(rows) x len(cols) placed at rows x cols of an m x n matrix"""
    rows = np.arange(m) if rows is None else np.asarray(rows, np.int64)
    cols = np.arange(n) if cols is None else np.asarray(cols, np.int64)
    tp, tv = np.zeros((m, n), bool), np.zeros((m, n), A[1].dtype)
    tp[np.ix_(rows, cols)] = A[0]
    tv[np.ix_(rows, cols)] = A[1]
    return tp, tv


def _rand_csr(rng, m, n, nnz):
    key = np.unique(rng.integers(0, m, nnz).astype(np.int64) * n + rng.integers(0, n, nnz))
    ptr = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(key // n, minlength=m), out=ptr[1:])
    return ptr, (key % n).astype(np.int32)


def _transpose(m, n, p, i, v):
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


def _desc(hb, tran=False, scmp=False):
    d = hb.descriptor()
    if tran:
        assert d.toggle(hb.g.GrB_INP0) == 0
    if scmp:
        assert d.set(hb.g.GrB_MASK, hb.g.GrB_SCMP) == 0
    return d


def _bits(x):
    return x if x.dtype == np.int32 else x.view(np.uint32)


def _same(got, want, name=""):
    for x, y in zip(got, want):
        assert x.shape == y.shape, (name, x.shape, y.shape)
        assert np.array_equal(_bits(x), _bits(y)), name


def _check(Cm, want, name=""):
    """C's CSR is the definition's; its CSC the exact transpose of that"""
    m, n = want[0].shape
    p, i, v = Cm.host_csr()
    _same((p, i, v), _csr(*want), name)
    _same(Cm.host_csc(), _transpose(m, n, p, i, v), name)


def _lists(rng, dim):
    k = max(dim // 2, 1)
    return {"ascending": np.sort(rng.choice(dim, k, replace=False)).astype(np.int32),
            "permuted subset": rng.permutation(dim)[:k].astype(np.int32),
            "permutation": rng.permutation(dim).astype(np.int32),
            "null": None}


def _len(lst, dim):
    return dim if lst is None else len(lst)


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("tran", [False, True])
def test_every_list_shape(hb, dt, tran):
    """f32 and i32, INP0 default and TRAN, four list shapes for I and J independently, no accum / plus / first, a
    rectangular C with stored zeros: the CSR is the definition's, the CSC its exact transpose, and everything outside
    I x J is what it was"""
    g = hb.g
    rng = np.random.default_rng(51)
    m, n = 150, 230
    cp, ci = _rand_csr(rng, m, n, 4000)
    cv = _vals(rng, ci.size, dt)
    assert (cv == 0).any()
    Cd = _dense(m, n, cp, ci, cv)
    d = _desc(hb, tran)
    for rname, rows in _lists(rng, m).items():
        for cname, cols in _lists(rng, n).items():
            ni, nj = _len(rows, m), _len(cols, n)
            ap, ai = _rand_csr(rng, ni, nj, ni * nj // 8)
            av = _vals(rng, ai.size, dt)
            A = _mat(g, nj, ni, *_transpose(ni, nj, ap, ai, av)) if tran else _mat(g, ni, nj, ap, ai, av)
            T = _place(m, n, _dense(ni, nj, ap, ai, av), rows, cols)
            for accum in (None, "plus", "first"):
                name = (rname, cname, accum)
                Cm = _mat(g, m, n, cp, ci, cv)
                assert g.assign_matrix(Cm, None, accum, A, rows, cols, d) == 0, name
                want = _ref(Cd, T, rows, cols, accum)
                _check(Cm, want, name)
                R = np.zeros((m, n), bool)
                R[np.ix_(np.arange(m) if rows is None else rows, np.arange(n) if cols is None else cols)] = True
                assert np.array_equal(want[0][~R], Cd[0][~R]) and np.array_equal(_bits(want[1])[~R], _bits(Cd[1])[~R]), name


def test_deletion(hb):
    """without an accum, what the source does not store is deleted inside the region and only there; an empty A over
    everything empties C, and leaves it alone under an accum"""
    g = hb.g
    rng = np.random.default_rng(52)
    m, n = 90, 120
    cp, ci = _rand_csr(rng, m, n, 3000)
    cv = _vals(rng, ci.size, F)
    Cd = _dense(m, n, cp, ci, cv)
    rows = rng.permutation(m)[:40].astype(np.int32)
    cols = np.sort(rng.choice(n, 50, replace=False)).astype(np.int32)
    ap, ai = _rand_csr(rng, 40, 50, 300)
    keep = np.repeat(np.arange(40), np.diff(ap)) % 3 != 0                    # every third row of A is empty
    ap = np.r_[0, np.cumsum(np.bincount(np.repeat(np.arange(40), np.diff(ap))[keep], minlength=40))].astype(np.int32)
    ai = ai[keep]
    av = _vals(rng, ai.size, F)
    A = _mat(g, 40, 50, ap, ai, av)
    Cm = _mat(g, m, n, cp, ci, cv)
    assert g.assign_matrix(Cm, None, None, A, rows, cols, hb.descriptor()) == 0
    want = _ref(Cd, _place(m, n, _dense(40, 50, ap, ai, av), rows, cols), rows, cols)
    _check(Cm, want)
    got = _dense(m, n, *Cm.host_csr())
    for k in range(0, 40, 3):                                                # cleared inside J, untouched outside it
        assert not got[0][rows[k], cols].any()
        out = np.setdiff1d(np.arange(n), cols)
        assert np.array_equal(got[0][rows[k], out], Cd[0][rows[k], out])
    z = np.zeros(m + 1, np.int32)
    E = _mat(g, m, n, z, np.zeros(0, np.int32), np.zeros(0, F))
    assert E.nvals() == 0
    Cm = _mat(g, m, n, cp, ci, cv)
    assert g.assign_matrix(Cm, None, "plus", E, None, None, hb.descriptor()) == 0
    _check(Cm, Cd)
    assert g.assign_matrix(Cm, None, None, E, None, None, hb.descriptor()) == 0
    assert Cm.nvals() == 0
    _check(Cm, (np.zeros((m, n), bool), np.zeros((m, n), F)))


def test_rows_in_every_bin(hb):
    """merged lengths (old C row plus T row) of 0, 1, 31, 32, 33 (the 16-lane groups end at 32), 2047, 2048, 2049 (a wave
    per row ends at 2048) and 7000 (a hub row of four 2048-position segments); each length as a row inside I with both
    sides, a row outside I (copied), a row of I in the old C only and a row of I in T only"""
    g = hb.g
    rng = np.random.default_rng(53)
    lens = [0, 1, 31, 32, 33, 2047, 2048, 2049, 7000]
    n = 9000
    crow, trow, in_i = [], [], []
    for L in lens:
        for la, lb, inside in ((L // 2, L - L // 2, True), (L, 0, False), (L, 0, True), (0, L, True)):
            crow.append(la)
            trow.append(lb)
            in_i.append(inside)
    m = len(crow)
    assert sorted({a + b for a, b in zip(crow, trow)}) == lens               # the merged lengths are the ones named
    rows = np.nonzero(in_i)[0].astype(np.int32)
    rows = rows[rng.permutation(rows.size)]
    pick = lambda k: np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
    cl = [pick(k) for k in crow]
    cp = np.r_[0, np.cumsum(crow)].astype(np.int32)
    ci = np.concatenate(cl)
    # row i of A goes to row rows[i] of C: half of its columns are columns of that row of C wherever both sides have some
    al = []
    for r in rows:
        k = trow[r]
        shared = min(k // 2, crow[r])
        own = cl[r][rng.permutation(crow[r])[:shared]] if shared else np.zeros(0, np.int32)
        rest = np.setdiff1d(np.arange(n, dtype=np.int32), cl[r])
        al.append(np.sort(np.r_[own, rest[rng.permutation(rest.size)[:k - shared]]]).astype(np.int32))
    ap = np.r_[0, np.cumsum([a.size for a in al])].astype(np.int32)
    ai = np.concatenate(al)
    for dt in (F, I):
        cv, av = _vals(rng, ci.size, dt), _vals(rng, ai.size, dt)
        Cd = _dense(m, n, cp, ci, cv)
        A = _mat(g, rows.size, n, ap, ai, av)
        T = _place(m, n, _dense(rows.size, n, ap, ai, av), rows, None)
        for accum in (None, "plus"):
            Cm = _mat(g, m, n, cp, ci, cv)
            assert g.assign_matrix(Cm, None, accum, A, rows, None, hb.descriptor()) == 0
            _check(Cm, _ref(Cd, T, rows, None, accum), (dt, accum))


def _mask_of(rng, m, n, dt):
    mp, mi = _rand_csr(rng, m, n, m * n // 3)
    mv = rng.integers(0, 2, mi.size).astype(dt)                              # half of the mask's stored values are zeros
    return mp, mi, mv


@pytest.mark.parametrize("dt", [F, I])
def test_mask(hb, dt):
    """the matrix and the constant form under a mask with stored zeros, default and SCMP, with and without an accum; a
    mask of the other element type; a mask that is C itself"""
    g = hb.g
    rng = np.random.default_rng(54)
    m, n = 110, 140
    cp, ci = _rand_csr(rng, m, n, 4000)
    cv = _vals(rng, ci.size, dt)
    Cd = _dense(m, n, cp, ci, cv)
    rows, cols = rng.permutation(m)[:60].astype(np.int32), rng.permutation(n)[:70].astype(np.int32)
    ap, ai = _rand_csr(rng, 60, 70, 1500)
    av = _vals(rng, ai.size, dt)
    A = _mat(g, 60, 70, ap, ai, av)
    T = _place(m, n, _dense(60, 70, ap, ai, av), rows, cols)
    Tc = _place(m, n, (np.ones((60, 70), bool), np.full((60, 70), 3, dt)), rows, cols)
    for mdt in (dt, I if dt == F else F):
        mp, mi, mv = _mask_of(rng, m, n, mdt)
        M = _mat(g, m, n, mp, mi, mv)
        Md = _dense(m, n, mp, mi, mv)
        for scmp in (False, True):
            for accum in (None, "plus"):
                name = (mdt, scmp, accum)
                Cm = _mat(g, m, n, cp, ci, cv)
                assert g.assign_matrix(Cm, M, accum, A, rows, cols, _desc(hb, scmp=scmp)) == 0, name
                _check(Cm, _ref(Cd, T, rows, cols, accum, Md, scmp), name)
                Cm = _mat(g, m, n, cp, ci, cv)
                assert g.assign_matrix(Cm, M, accum, 3, rows, cols, _desc(hb, scmp=scmp)) == 0, name
                _check(Cm, _ref(Cd, Tc, rows, cols, accum, Md, scmp), name)
    for scmp in (False, True):                                               # C is its own mask
        Cm = _mat(g, m, n, cp, ci, cv)
        assert g.assign_matrix(Cm, Cm, None, A, rows, cols, _desc(hb, scmp=scmp)) == 0
        _check(Cm, _ref(Cd, T, rows, cols, None, Cd, scmp), scmp)


@pytest.mark.parametrize("dt", [F, I])
def test_row_column_and_constant_forms(hb, dt):
    """C(I, j) = u and C(i, J) = u for a sparse and a dense u, every list shape, no accum and plus; C(I, J) = val"""
    g = hb.g
    rng = np.random.default_rng(55)
    m, n = 130, 90
    cp, ci = _rand_csr(rng, m, n, 3500)
    cv = _vals(rng, ci.size, dt)
    Cd = _dense(m, n, cp, ci, cv)
    for is_col in (True, False):
        dim, other = (m, n) if is_col else (n, m)
        for lname, lst in _lists(rng, dim).items():
            k = _len(lst, dim)
            idx = np.arange(dim) if lst is None else lst
            dense_vals = _vals(rng, k, dt)
            si = np.sort(rng.choice(k, max(k // 3, 1), replace=False)).astype(np.int32)
            sv = _vals(rng, si.size, dt)
            for fixed in (0, other - 1, other // 2):
                for sparse in (False, True):
                    u = g.Vector(k, dt)
                    up, uv = np.zeros(k, bool), np.zeros(k, dt)
                    if sparse:
                        assert u.build(si, sv, si.size, None) == 0
                        up[si], uv[si] = True, sv
                    else:
                        assert u.build(dense_vals, k) == 0
                        up[:], uv[:] = True, dense_vals
                    tp, tv = np.zeros((m, n), bool), np.zeros((m, n), dt)
                    if is_col:
                        tp[idx, fixed], tv[idx, fixed] = up, uv
                    else:
                        tp[fixed, idx], tv[fixed, idx] = up, uv
                    for accum in (None, "plus"):
                        name = (is_col, lname, fixed, sparse, accum)
                        Cm = _mat(g, m, n, cp, ci, cv)
                        r_, c_ = (lst, fixed) if is_col else (fixed, lst)
                        assert g.assign_matrix(Cm, None, accum, u, r_, c_, hb.descriptor()) == 0, name
                        rr, cc = (lst, [fixed]) if is_col else ([fixed], lst)
                        _check(Cm, _ref(Cd, (tp, tv), rr, cc, accum), name)
    for rname, rows in _lists(rng, m).items():
        for cname, cols in _lists(rng, n).items():
            ni, nj = _len(rows, m), _len(cols, n)
            Tc = _place(m, n, (np.ones((ni, nj), bool), np.full((ni, nj), 7, dt)), rows, cols)
            for accum in (None, "minus"):
                Cm = _mat(g, m, n, cp, ci, cv)
                assert g.assign_matrix(Cm, None, accum, 7, rows, cols, hb.descriptor()) == 0, (rname, cname, accum)
                _check(Cm, _ref(Cd, Tc, rows, cols, accum), (rname, cname, accum))


def test_every_accum_operator(hb):
    """the operators of the dense reference above on both types; all 17 codes are accepted"""
    g = hb.g
    rng = np.random.default_rng(56)
    m = n = 60
    cp, ci = _rand_csr(rng, m, n, 1200)
    ap, ai = _rand_csr(rng, m, n, 1200)
    for dt in (F, I):
        cv, av = _vals(rng, ci.size, dt), _vals(rng, ai.size, dt)
        Cd, Ad = _dense(m, n, cp, ci, cv), _dense(m, n, ap, ai, av)
        A = _mat(g, m, n, ap, ai, av)
        for op in g.BINARY_OPS:
            Cm = _mat(g, m, n, cp, ci, cv)
            assert g.assign_matrix(Cm, None, op, A, None, None, hb.descriptor()) == 0, op
            if op in ("plus", "first", "second", "minus", "multiplies", "minimum", "maximum"):
                _check(Cm, _ref(Cd, Ad, None, None, op), (dt, op))


def test_round_trip_and_identities(hb):
    """extract(assign(C, A, I, J), I, J) is A; assign over everything with plus is eWiseAdd under PlusMultiplies; assign
    over everything without an accum is a copy of A"""
    g = hb.g
    rng = np.random.default_rng(57)
    m, n = 170, 150
    cp, ci = _rand_csr(rng, m, n, 5000)
    cv = _vals(rng, ci.size, F)
    for rows, cols in ((rng.permutation(m)[:80].astype(np.int32), rng.permutation(n)[:60].astype(np.int32)),
                       (np.sort(rng.choice(m, 80, replace=False)).astype(np.int32), None)):
        ni, nj = _len(rows, m), _len(cols, n)
        ap, ai = _rand_csr(rng, ni, nj, 1500)
        av = _vals(rng, ai.size, F)
        A = _mat(g, ni, nj, ap, ai, av)
        Cm = _mat(g, m, n, cp, ci, cv)
        assert g.assign_matrix(Cm, None, None, A, rows, cols, hb.descriptor()) == 0
        X = g.Matrix(ni, nj, F)
        assert g.extract(X, None, None, Cm, rows, cols, hb.descriptor()) == 0
        _same(X.host_csr(), (ap, ai, av))
        _same(X.host_csc(), A.host_csc())
    bp, bi = _rand_csr(rng, m, n, 5000)
    bv = (rng.random(bi.size) * 3).astype(F)
    cv2 = (rng.random(ci.size) * 3).astype(F)
    B = _mat(g, m, n, bp, bi, bv)
    Cm, C2, E = _mat(g, m, n, cp, ci, cv2), _mat(g, m, n, cp, ci, cv2), g.Matrix(m, n, F)
    assert g.assign_matrix(Cm, None, "plus", B, None, None, hb.descriptor()) == 0
    assert g.eWiseAdd(E, None, None, "PlusMultiplies", C2, B, hb.descriptor()) == 0
    _same(Cm.host_csr(), E.host_csr())
    _same(Cm.host_csc(), E.host_csc())
    assert g.assign_matrix(Cm, None, None, B, None, None, hb.descriptor()) == 0
    _same(Cm.host_csr(), (bp, bi, bv))
    _same(Cm.host_csc(), B.host_csc())


def _rmat(scale, seed):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=True)
    ptr, ind = (x.cpu().numpy().astype(np.int32) for x in gr["csr"])
    return n, ptr, ind


def test_rmat16_against_scipy(hb):
    """RMAT-16, hub rows included: C(p, p) = extract(B, q, q) for permuted random halves p and q of the vertices, without
    an accum and with plus.  All values are nonzero integers, so scipy drops and rounds nothing"""
    import scipy.sparse as sp
    g = hb.g
    n, cp, ci = _rmat(16, 5)
    _, bp, bi = _rmat(16, 6)
    assert np.diff(cp).max() > 2 * 2048                                      # hub rows of several segments
    rng = np.random.default_rng(58)
    cv, bv = rng.integers(1, 4, ci.size).astype(F), rng.integers(1, 4, bi.size).astype(F)
    B = _mat(g, n, n, bp, bi, bv)
    k = n // 2
    p, q = rng.permutation(n)[:k].astype(np.int32), rng.permutation(n)[:k].astype(np.int32)
    A = g.Matrix(k, k, F)
    assert g.extract(A, None, None, B, q, q, hb.descriptor()) == 0
    SC = sp.csr_matrix((cv, ci, cp), shape=(n, n))
    SA = sp.csr_matrix((bv, bi, bp), shape=(n, n))[q][:, q]
    sel = sp.csr_matrix((np.ones(k, F), (p, np.arange(k))), shape=(n, k))    # column i is the unit vector of p[i]
    T = (sel @ SA @ sel.T).tocsr()
    ind = np.zeros(n, F)
    ind[p] = 1
    inside = (sp.diags(ind) @ SC @ sp.diags(ind)).tocsr()
    for accum in (None, "plus"):
        W = (SC + T if accum else SC - inside + T).tocsr()
        W.eliminate_zeros()                                                  # (what SC - inside cancelled)
        W.sort_indices()
        Cm = _mat(g, n, n, cp, ci, cv)
        assert g.assign_matrix(Cm, None, accum, A, p, p, hb.descriptor()) == 0
        got = Cm.host_csr()
        _same(got, (W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data.astype(F)), accum)
        _same(Cm.host_csc(), _transpose(n, n, *got), accum)


def test_csr_only_operands(hb):
    """a product result has no CSC: assigning it, or into it, gives a CSR-only C that mxv accepts; its transposed use is
    GrB_INVALID_OBJECT"""
    g = hb.g
    rng = np.random.default_rng(59)
    n = 200
    ap, ai = _rand_csr(rng, n, n, 1500)
    av = rng.integers(1, 3, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    Pd = _dense(n, n, *P.host_csr())
    Ad = _dense(n, n, ap, ai, av)
    rows, cols = rng.permutation(n).astype(np.int32), np.sort(rng.choice(n, n, replace=False)).astype(np.int32)
    x = rng.integers(0, 4, n).astype(F)

    def mxv_ok(Cm, want):
        u, w = g.Vector(n, F), g.Vector(n, F)
        assert u.build(x, n) == 0
        assert g.mxv(w, None, None, "PlusMultiplies", Cm, u, hb.descriptor(mxvmode=2)) == 0
        assert np.array_equal(hb.dense_values(w).astype(np.float64), np.where(want[0], want[1], 0).astype(np.float64) @ x)

    Cm = _mat(g, n, n, ap, ai, av)                                           # the source is CSR only
    assert g.assign_matrix(Cm, None, "plus", P, rows, cols, hb.descriptor()) == 0
    want = _ref(Ad, _place(n, n, Pd, rows, cols), rows, cols, "plus")
    _same(Cm.host_csr(), _csr(*want))
    with pytest.raises(g._lib.GrbError) as e:
        Cm.host_csc()
    assert e.value.info == g.GrB_NO_VALUE
    mxv_ok(Cm, want)
    kept = [y.copy() for y in Cm.host_csr()]
    assert g.assign_matrix(Cm, None, None, P, rows, cols, _desc(hb, tran=True)) == g.GrB_INVALID_OBJECT
    _same(Cm.host_csr(), kept)
    assert g.assign_matrix(P, None, None, A, rows, cols, hb.descriptor()) == 0     # C is CSR only
    want = _ref(Pd, _place(n, n, Ad, rows, cols), rows, cols)
    _same(P.host_csr(), _csr(*want))
    with pytest.raises(g._lib.GrbError):
        P.host_csc()
    mxv_ok(P, want)


def test_aliasing(hb):
    """C is A (a square C over permuted lists) and C is the mask"""
    g = hb.g
    rng = np.random.default_rng(60)
    n = 140
    cp, ci = _rand_csr(rng, n, n, 3000)
    cv = _vals(rng, ci.size, F)
    Cd = _dense(n, n, cp, ci, cv)
    rows, cols = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    for accum in (None, "plus"):
        Cm = _mat(g, n, n, cp, ci, cv)
        assert g.assign_matrix(Cm, None, accum, Cm, rows, cols, hb.descriptor()) == 0
        _check(Cm, _ref(Cd, _place(n, n, Cd, rows, cols), rows, cols, accum), accum)
    Cm = _mat(g, n, n, cp, ci, cv)
    assert g.assign_matrix(Cm, Cm, None, 9, rows[:70], cols[:90], hb.descriptor()) == 0
    Tc = _place(n, n, (np.ones((70, 90), bool), np.full((70, 90), 9, F)), rows[:70], cols[:90])
    _check(Cm, _ref(Cd, Tc, rows[:70], cols[:90], None, Cd, False))


def _arr(a):
    a = np.ascontiguousarray(a, np.int32)
    return a, a.ctypes.data


def test_errors_leave_c_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(61)
    m, n = 100, 80
    cp, ci = _rand_csr(rng, m, n, 1500)
    cv = _vals(rng, ci.size, F)
    Cm = _mat(g, m, n, cp, ci, cv)
    rows, cols = rng.permutation(m)[:60].astype(np.int32), rng.permutation(n)[:50].astype(np.int32)
    ap, ai = _rand_csr(rng, 60, 50, 700)
    av = _vals(rng, ai.size, F)
    A = _mat(g, 60, 50, ap, ai, av)
    d = hb.descriptor()
    before = [x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()]

    def unchanged():
        return all(np.array_equal(x, y) for x, y in zip(before, list(Cm.host_csr()) + list(Cm.host_csc())))

    (_, rp), (_, cq) = _keep = _arr(rows), _arr(cols)
    call = lambda C_, A_, r, nr, c, nc, mask=None: lib.grb_matrix_assign(C_, mask, -1, A_, r, nr, c, nc, d._h)
    assert call(None, A._h, rp, 60, cq, 50) == g.GrB_UNINITIALIZED_OBJECT
    assert call(Cm._h, None, rp, 60, cq, 50) == g.GrB_UNINITIALIZED_OBJECT
    assert g.assign_matrix(Cm, None, None, g.Matrix(60, 50, F), rows, cols, d) == g.GrB_UNINITIALIZED_OBJECT   # unbuilt A
    assert g.assign_matrix(Cm, g.Matrix(m, n, F), None, A, rows, cols, d) == g.GrB_UNINITIALIZED_OBJECT        # unbuilt mask
    assert g.assign_matrix(Cm, g.Matrix(m, n, F), None, 1, rows, cols, d) == g.GrB_UNINITIALIZED_OBJECT
    Ai = _mat(g, 60, 50, ap, ai, av.astype(I))
    assert g.assign_matrix(Cm, None, None, Ai, rows, cols, d) == g.GrB_NOT_IMPLEMENTED                         # another type
    assert g.assign_matrix(Cm, None, None, A, rows[:59], cols, d) == g.GrB_DIMENSION_MISMATCH
    assert g.assign_matrix(Cm, None, None, A, rows, np.r_[cols, 79 - cols[0]], d) == g.GrB_DIMENSION_MISMATCH
    assert g.assign_matrix(Cm, None, None, A, None, cols, d) == g.GrB_DIMENSION_MISMATCH                       # A has 60 rows
    assert g.assign_matrix(Cm, None, None, A, rows, cols, _desc(hb, tran=True)) == g.GrB_DIMENSION_MISMATCH    # A^T is 50 x 60
    assert call(Cm._h, A._h, None, 60, cq, 50) == g.GrB_DIMENSION_MISMATCH                                     # a null list of 60 != 100
    assert call(Cm._h, A._h, rp, 60, None, 50) == g.GrB_DIMENSION_MISMATCH
    assert lib.grb_matrix_assign_scalar(Cm._h, None, -1, 1.0, None, 60, cq, 50, d._h) == g.GrB_DIMENSION_MISMATCH
    Mbad = _mat(g, m, n + 1, np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, F))
    assert g.assign_matrix(Cm, Mbad, None, A, rows, cols, d) == g.GrB_DIMENSION_MISMATCH                       # a mask not of C's shape
    assert g.assign_matrix(Cm, Mbad, None, 1, rows, cols, d) == g.GrB_DIMENSION_MISMATCH
    for bad in (-1, m):
        r2 = rows.copy()
        r2[59] = bad
        assert g.assign_matrix(Cm, None, None, A, r2, cols, d) == g.GrB_INDEX_OUT_OF_BOUNDS
        assert g.assign_matrix(Cm, None, None, 1, r2, cols, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    for bad in (-1, n):
        c2 = cols.copy()
        c2[0] = bad
        assert g.assign_matrix(Cm, None, "plus", A, rows, c2, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    for lst, which in ((rows, 0), (cols, 1)):                                                                  # a repeated index
        l2 = lst.copy()
        l2[7] = l2[31]
        args = (l2, cols) if which == 0 else (rows, l2)
        assert g.assign_matrix(Cm, None, None, A, *args, d) == g.GrB_INVALID_INDEX
        assert g.assign_matrix(Cm, None, "plus", 2, *args, d) == g.GrB_INVALID_INDEX
        assert g.assign_matrix(Cm, None, None, A, *(np.sort(x) for x in args), d) == g.GrB_INVALID_INDEX
    assert unchanged()
    # the row and column forms
    u = g.Vector(60, F)
    assert u.build(np.arange(60, dtype=F), 60) == 0
    assert lib.grb_matrix_assign_col(None, None, -1, u._h, rp, 60, 3, d._h) == g.GrB_UNINITIALIZED_OBJECT
    assert lib.grb_matrix_assign_row(Cm._h, None, -1, None, 3, cq, 50, d._h) == g.GrB_UNINITIALIZED_OBJECT
    assert g.assign_matrix(Cm, None, None, g.Vector(60, F), rows, 3, d) == g.GrB_UNINITIALIZED_OBJECT          # no storage yet
    assert lib.grb_matrix_assign_col(Cm._h, u._h, -1, u._h, rp, 60, 3, d._h) == g.GrB_NOT_IMPLEMENTED          # a vector mask
    assert lib.grb_matrix_assign_row(Cm._h, u._h, -1, u._h, 3, cq, 60, d._h) == g.GrB_NOT_IMPLEMENTED
    ui = g.Vector(60, I)
    assert ui.build(np.arange(60, dtype=I), 60) == 0
    assert g.assign_matrix(Cm, None, None, ui, rows, 3, d) == g.GrB_NOT_IMPLEMENTED
    assert g.assign_matrix(Cm, None, None, u, rows[:59], 3, d) == g.GrB_DIMENSION_MISMATCH
    assert g.assign_matrix(Cm, None, None, u, 3, cols, d) == g.GrB_DIMENSION_MISMATCH                          # u has 60, J 50
    assert lib.grb_matrix_assign_col(Cm._h, None, -1, u._h, None, 60, 3, d._h) == g.GrB_DIMENSION_MISMATCH
    for bad in (-1, n):
        assert g.assign_matrix(Cm, None, None, u, rows, bad, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    for bad in (-1, m):
        assert g.assign_matrix(Cm, None, None, u, bad, np.arange(60, dtype=np.int32), d) == g.GrB_INDEX_OUT_OF_BOUNDS
    r2 = rows.copy()
    r2[3] = m
    assert g.assign_matrix(Cm, None, None, u, r2, 3, d) == g.GrB_INDEX_OUT_OF_BOUNDS
    r2[3] = r2[4]
    assert g.assign_matrix(Cm, None, None, u, r2, 3, d) == g.GrB_INVALID_INDEX
    assert unchanged()
    # counts of zero are legal and leave C as it was
    Z = _mat(g, 0, 50, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, F))
    assert g.assign_matrix(Cm, None, None, Z, [], cols, d) == 0
    assert g.assign_matrix(Cm, None, None, 5, rows, [], d) == 0
    assert g.assign_matrix(Cm, None, None, g.Vector(0, F), [], 3, d) in (0, g.GrB_UNINITIALIZED_OBJECT)
    assert unchanged()
    # a null descriptor means the defaults
    assert g.assign_matrix(Cm, None, None, A, rows, cols, None) == 0
    _check(Cm, _ref(_dense(m, n, cp, ci, cv), _place(m, n, _dense(60, 50, ap, ai, av), rows, cols), rows, cols))


def test_int32_max_guard(hb):
    """a constant over all of an empty 50 000 x 50 000 C is 2.5e9 entries: GrB_OUT_OF_MEMORY before anything is
    allocated, C unchanged, the device's free memory where it was"""
    import torch
    g = hb.g
    k = 50000
    Cm = _mat(g, k, k, np.zeros(k + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, F))
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    assert g.assign_matrix(Cm, None, None, 1, None, None, hb.descriptor()) == g.GrB_OUT_OF_MEMORY
    free1 = torch.cuda.mem_get_info()[0]
    assert abs(free1 - free0) <= 8 << 20, (free0, free1)
    assert Cm.nvals() == 0
    assert not Cm.host_csr()[0].any() and not Cm.host_csc()[0].any()
    # a never-built C counts as empty, and is still unbuilt afterwards
    Cn = g.Matrix(k, k, F)
    assert g.assign_matrix(Cn, None, "plus", 1, None, None, hb.descriptor()) == g.GrB_OUT_OF_MEMORY
    assert g.assign_matrix(Cn, None, None, 2, [7, 3], [1, 49999], hb.descriptor()) == 0
    p, i, v = Cn.host_csr()
    assert np.array_equal(np.nonzero(np.diff(p))[0], [3, 7]) and np.array_equal(i, [1, 49999, 1, 49999]) and (v == 2).all()


def test_determinism(hb):
    """unordered lists (the sorted path) under a mask with an accum: two calls, the same bits in both orientations"""
    g = hb.g
    n, cp, ci = _rmat(13, 8)
    rng = np.random.default_rng(62)
    cv = (rng.random(ci.size) * 3).astype(F)
    rows, cols = rng.permutation(n).astype(np.int32), rng.permutation(n).astype(np.int32)
    A = _mat(g, n, n, cp, ci, (rng.random(ci.size) * 3).astype(F))
    outs = []
    for _ in range(2):
        Cm = _mat(g, n, n, cp, ci, cv)
        assert g.assign_matrix(Cm, A, "plus", A, rows, cols, hb.descriptor()) == 0
        outs.append([x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()])
    _same(outs[0], outs[1])


def _line(tag, m, n, p, i, v):
    return "%s %d %d %d | %s | %s | %s" % (tag, m, n, i.size, " ".join(str(x) for x in p), " ".join(str(x) for x in i),
                                          " ".join("%.9g" % x for x in v))


def test_cpp_frontend(tmp_path):
    """tests/tools/assign.cpp: one call of each of the four overloads on a 4 x 4 literal"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "assign")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "assign.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln[:3] in ("csr", "csc")]
    # A = [[1 . 2 .] [. 3 . .] [4 . 5 6] [. 0 . 7]]
    ap, ai = np.array([0, 2, 3, 6, 8], np.int32), np.array([0, 2, 1, 0, 2, 3, 1, 3], np.int32)
    Cd = _dense(4, 4, ap, ai, np.array([1, 2, 3, 4, 5, 6, 0, 7], F))
    B = (np.eye(2, dtype=bool), np.diag(np.array([10, 20], F)))
    col = (np.zeros((4, 4), bool), np.zeros((4, 4), F))
    col[0][[3, 1], 2], col[1][[3, 1], 2] = True, [30, 40]
    row = (np.zeros((4, 4), bool), np.zeros((4, 4), F))
    row[0][2, 1], row[1][2, 1] = True, 50
    cases = [("mat", _ref(Cd, _place(4, 4, B, [2, 0], [3, 0]), [2, 0], [3, 0])),
             ("const", _ref(Cd, _place(4, 4, (np.ones((2, 4), bool), np.full((2, 4), 9, F)), [1, 3], None), [1, 3], None, "plus")),
             ("col", _ref(Cd, col, [3, 1], [2])),
             ("row", _ref(Cd, row, [2], [0, 1]))]
    want = []
    for tag, w in cases:
        p, i, v = _csr(*w)
        want.append(_line("csr " + tag, 4, 4, p, i, v))
        want.append(_line("csc " + tag, 4, 4, *_transpose(4, 4, p, i, v)))
    # C({2, 0}, {3, 0}) = [[10 .] [. 20]]: row 2 loses its 4 (deleted: B(0, 1) is not stored) and its 6 becomes 10
    assert want[0] == "csr mat 4 4 7 | 0 2 3 5 7 | 0 2 1 2 3 1 3 | 20 2 3 5 10 0 7", want[0]
    assert lines == want, lines
