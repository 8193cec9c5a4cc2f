"""Matrix eWiseAdd / eWiseMult and transpose (csrc/ewise_matrix.hip): every semiring and orientation against a numpy
restatement of the union / intersection, rows in every bin, RMAT hub rows against scipy, masks, the orientations of the
result, downstream traversals and products on a result, aliasing, the error codes and the C++ frontend."""
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


def _from_keys(m, n, key):
    ptr = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(key // n, minlength=m), out=ptr[1:])
    return ptr, (key % n).astype(np.int32)


def _keys(n, p, i):
    return np.repeat(np.arange(p.size - 1, dtype=np.int64), np.diff(p)) * n + i


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


def _desc(hb, ta=False, tb=False, scmp=False):
    g = hb.g
    d = hb.descriptor()
    if ta:
        assert d.toggle(g.GrB_INP0) == 0
    if tb:
        assert d.toggle(g.GrB_INP1) == 0
    if scmp:
        assert d.set(g.GrB_MASK, g.GrB_SCMP) == 0
    return d


class _Registered:
    """a registered semiring restated with the oracle's operators"""
    def __init__(self, add, ident, mul, dt):
        from oracle.semiring import binary_op
        self.add_op, self.mul_op, self._id = binary_op(add, dt), binary_op(mul, dt), dt(ident)


def _expect(add, sr, m, n, a, b, mask=None, scmp=False):
    """C = A (+) B (union, add) or A (x) B (intersection, mul), entries kept where the mask passes"""
    ka, kb = _keys(n, a[0], a[1]), _keys(n, b[0], b[1])
    key = np.union1d(ka, kb) if add else np.intersect1d(ka, kb)
    ia = np.minimum(np.searchsorted(ka, key), max(ka.size - 1, 0))
    ib = np.minimum(np.searchsorted(kb, key), max(kb.size - 1, 0))
    in_a = (ka[ia] == key) if ka.size else np.zeros(key.size, bool)
    in_b = (kb[ib] == key) if kb.size else np.zeros(key.size, bool)
    dt = a[2].dtype
    val = np.zeros(key.size, dt)
    both = in_a & in_b
    op = sr.add_op if add else sr.mul_op
    if both.any():
        val[both] = op(a[2][ia[both]], b[2][ib[both]])
    val[in_a & ~in_b] = a[2][ia[in_a & ~in_b]]
    val[in_b & ~in_a] = b[2][ib[in_b & ~in_a]]
    if mask is not None:
        km = _keys(n, mask[0], mask[1])[mask[2] != 0]
        keep = np.isin(key, km) != scmp
        key, val = key[keep], val[keep]
    return (*_from_keys(m, n, key), val)


def _check(got, want, name=""):
    cp, ci, cv = got
    wp, wi, wv = want
    assert np.array_equal(cp, wp), name
    assert np.array_equal(ci, wi), name
    if cv.dtype == np.int32:
        assert np.array_equal(cv, wv), name
    elif name == "PlusDivides/mult":
        assert np.allclose(cv, wv, rtol=4e-7, atol=0, equal_nan=True), name
    else:
        assert np.array_equal(cv.view(np.uint32), wv.view(np.uint32)) or np.array_equal(cv, wv, equal_nan=True), \
            (name, int((cv != wv).sum()))


def _check_csc(C, m, n, name=""):
    """C's CSC holds the same entries and bits as the transpose of its CSR"""
    p, i, v = C.host_csr()
    tp, ti, tv = C.host_csc()
    wp, wi, wv = _transpose(m, n, p, i, v)
    assert np.array_equal(tp, wp) and np.array_equal(ti, wi), name
    assert np.array_equal(tv.view(np.uint32), wv.view(np.uint32)), name


def _cases(g, dt):
    from oracle.semiring import Semiring, SEMIRINGS
    sid = g.register_semiring("maximum", 0.0, "minus")
    return [(name, name, Semiring(name, dt)) for name in SEMIRINGS] + [("registered", sid, _Registered("maximum", 0.0, "minus", dt))]


@pytest.mark.parametrize("dt", [F, I])
def test_every_semiring_and_orientation(hb, dt):
    """all 17 built-in semirings and a registered one, both ops, four orientations, A != B, stored zeros, a rectangular
    shape; C's CSC (every input has both orientations) is the transpose of its CSR, bit for bit"""
    g = hb.g
    rng = np.random.default_rng(17)
    m, n = 150, 230
    (ap, ai), (bp, bi) = _rand_csr(rng, m, n, 3000), _rand_csr(rng, m, n, 3000)
    av, bv = _vals(rng, ai.size, dt), _vals(rng, bi.size, dt)
    for ta in (False, True):
        for tb in (False, True):
            d = _desc(hb, ta, tb)
            A, B = _stored(g, m, n, ap, ai, av, ta), _stored(g, m, n, bp, bi, bv, tb)
            for label, op, sr in _cases(g, dt):
                for add in (True, False):
                    Cm = g.Matrix(m, n, dt)
                    fn = g.eWiseAdd if add else g.eWiseMult
                    assert fn(Cm, None, None, op, A, B, d) == 0, (label, ta, tb, add)
                    name = label + ("/add" if add else "/mult")
                    _check(Cm.host_csr(), _expect(add, sr, m, n, (ap, ai, av), (bp, bi, bv)), name)
                    _check_csc(Cm, m, n, name)


def _bin_rows(rng, n):
    """rows for every bin and shape of overlap: (A columns, B columns) per row"""
    rows = []
    for length in (0, 1, 7, 16, 40, 300, 1000, 1500, 5000, 9000):
        k = max(length, 1)
        cols = np.sort(rng.choice(n, min(2 * k, n), replace=False)).astype(np.int32)
        half = cols[:length]
        rows += [(half, np.zeros(0, np.int32)),                          # only in A
                 (np.zeros(0, np.int32), half),                          # only in B
                 (half, half),                                           # identical
                 (cols[0:2 * length:2], cols[1:2 * length:2])]           # disjoint, interleaved
        sa = np.sort(rng.choice(n, length, replace=False)).astype(np.int32)
        sb = np.sort(rng.choice(n, length, replace=False)).astype(np.int32)
        rows.append((sa, sb))                                            # random overlap
    # one row's columns shared at the segment boundaries of the hub bin: A = evens, B = every third
    rows.append((np.arange(0, 24000, 2, dtype=np.int32), np.arange(0, 24000, 3, dtype=np.int32)))
    rows.append((np.zeros(0, np.int32), np.zeros(0, np.int32)))
    return rows


def _csr_of(rows, pick):
    lists = [r[pick] for r in rows]
    ptr = np.zeros(len(lists) + 1, np.int32)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    return ptr, np.concatenate(lists).astype(np.int32)


@pytest.mark.parametrize("dt", [F, I])
def test_rows_in_every_bin(hb, dt):
    """empty rows, rows only in A or only in B, identical, disjoint and overlapping rows of every length: the 16-lane
    groups (up to 32 merged), a wave per row (up to 2048), and hub rows cut into 2048-long segments; with and without a
    mask, both orientations of B"""
    from oracle.semiring import Semiring
    g = hb.g
    rng = np.random.default_rng(23)
    n = 30000
    rows = _bin_rows(rng, n)
    m = len(rows)
    ap, ai = _csr_of(rows, 0)
    bp, bi = _csr_of(rows, 1)
    lens = np.diff(ap) + np.diff(bp)
    assert (lens > 0).any() and (lens <= 32).sum() > 5 and ((lens > 32) & (lens <= 2048)).sum() > 5 and (lens > 2048).sum() > 5
    av, bv = _vals(rng, ai.size, dt), _vals(rng, bi.size, dt)
    mp, mi = _rand_csr(rng, m, n, 200000)
    mv = rng.integers(0, 3, mi.size).astype(dt)
    Mk = _mat(g, m, n, mp, mi, mv)
    for tb in (False, True):
        A, B = _mat(g, m, n, ap, ai, av), _stored(g, m, n, bp, bi, bv, tb)
        for name in ("PlusMultiplies", "PlusMinus", "MinimumPlus", "PlusDivides"):
            sr = Semiring(name, dt)
            for add in (True, False):
                fn = g.eWiseAdd if add else g.eWiseMult
                label = name + ("/add" if add else "/mult")
                Cm = g.Matrix(m, n, dt)
                assert fn(Cm, None, None, name, A, B, _desc(hb, False, tb)) == 0
                _check(Cm.host_csr(), _expect(add, sr, m, n, (ap, ai, av), (bp, bi, bv)), label)
                _check_csc(Cm, m, n, label)
                for scmp in (False, True):
                    Cm = g.Matrix(m, n, dt)
                    assert fn(Cm, Mk, None, name, A, B, _desc(hb, False, tb, scmp)) == 0
                    _check(Cm.host_csr(), _expect(add, sr, m, n, (ap, ai, av), (bp, bi, bv), (mp, mi, mv), scmp), label)
                    _check_csc(Cm, m, n, label)


def _rmat(scale, seed, symmetrize=True):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=symmetrize)
    ptr, ind = (x.cpu().numpy().astype(np.int32) for x in gr["csr"])
    return n, ptr, ind


def test_hub_rows_rmat16_complete(hb):
    """A + B and A .* B of two RMAT-16 graphs, whole, against scipy (values 1..3: no sum or product is 0)"""
    import scipy.sparse as sp
    g = hb.g
    n, ap, ai = _rmat(16, 1)
    n2, bp, bi = _rmat(16, 2)
    assert n == n2
    rng = np.random.default_rng(16)
    av, bv = rng.integers(1, 4, ai.size).astype(F), rng.integers(1, 4, bi.size).astype(F)
    assert (np.diff(ap) + np.diff(bp)).max() > 2 * 2048                 # hub rows of several segments
    A, B = _mat(g, n, n, ap, ai, av), _mat(g, n, n, bp, bi, bv)
    SA, SB = sp.csr_matrix((av, ai, ap), shape=(n, n)), sp.csr_matrix((bv, bi, bp), shape=(n, n))
    for add in (True, False):
        Cm = g.Matrix(n, n, F)
        assert (g.eWiseAdd if add else g.eWiseMult)(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
        W = (SA + SB if add else SA.multiply(SB)).tocsr()
        W.sort_indices()
        cp, ci, cv = Cm.host_csr()
        assert np.array_equal(cp, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(cv, W.data.astype(F))
        _check_csc(Cm, n, n)


def test_masks_f32_and_i32(hb):
    """f32 and i32 masks holding stored zeros, with and without GrB_SCMP, on f32 and i32 operands"""
    from oracle.semiring import Semiring
    g = hb.g
    rng = np.random.default_rng(5)
    m, n = 300, 200
    (ap, ai), (bp, bi), (mp, mi) = _rand_csr(rng, m, n, 8000), _rand_csr(rng, m, n, 8000), _rand_csr(rng, m, n, 20000)
    for dt in (F, I):
        av, bv = _vals(rng, ai.size, dt), _vals(rng, bi.size, dt)
        A, B = _mat(g, m, n, ap, ai, av), _mat(g, m, n, bp, bi, bv)
        sr = Semiring("MaximumMultiplies", dt)
        for mdt in (F, I):
            mv = rng.integers(0, 3, mi.size).astype(mdt)
            assert (mv == 0).any()
            Mk = _mat(g, m, n, mp, mi, mv)
            for add in (True, False):
                for scmp in (False, True):
                    Cm = g.Matrix(m, n, dt)
                    assert (g.eWiseAdd if add else g.eWiseMult)(Cm, Mk, None, "MaximumMultiplies", A, B, _desc(hb, scmp=scmp)) == 0
                    _check(Cm.host_csr(), _expect(add, sr, m, n, (ap, ai, av), (bp, bi, bv), (mp, mi, mv), scmp))
                    _check_csc(Cm, m, n)


def test_csr_only_input_gives_csr_only_result(hb):
    """a product result has no CSC: C = P + A is CSR only (host_csc -> GrB_NO_VALUE), and P cannot be transposed"""
    from oracle.semiring import Semiring
    g = hb.g
    rng = np.random.default_rng(9)
    n = 200
    ap, ai = _rand_csr(rng, n, n, 1500)
    av = rng.integers(1, 3, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    pp, pi, pv = (x.copy() for x in P.host_csr())
    Cm = g.Matrix(n, n, F)
    assert g.eWiseAdd(Cm, None, None, "PlusMultiplies", P, A, hb.descriptor()) == 0
    _check(Cm.host_csr(), _expect(True, Semiring("PlusMultiplies", F), n, n, (pp, pi, pv), (ap, ai, av)))
    with pytest.raises(g._lib.GrbError) as e:
        Cm.host_csc()
    assert e.value.info == g.GrB_NO_VALUE
    assert g.eWiseMult(Cm, None, None, "PlusMultiplies", A, P, _desc(hb, tb=True)) == g.GrB_INVALID_OBJECT
    # with a mask that is CSR only, too
    Cm2 = g.Matrix(n, n, F)
    assert g.eWiseMult(Cm2, P, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    with pytest.raises(g._lib.GrbError):
        Cm2.host_csc()


def test_symmetrised_graph_downstream(hb):
    """C = A + A^T of a directed RMAT graph (INP1 = TRAN), then BFS and mxv push / pull on C: the same labels and
    vectors as on the same CSR built with build_csr"""
    import scipy.sparse as sp
    g = hb.g
    n, ap, ai = _rmat(14, 3, symmetrize=False)
    av = np.ones(ai.size, F)
    A = _mat(g, n, n, ap, ai, av)
    Cm = g.Matrix(n, n, F)
    assert g.eWiseAdd(Cm, None, None, "PlusMultiplies", A, A, _desc(hb, tb=True)) == 0
    S = sp.csr_matrix((av, ai, ap), shape=(n, n))
    W = (S + S.T).tocsr()
    W.sort_indices()
    cp, ci, cv = (x.copy() for x in Cm.host_csr())
    assert np.array_equal(cp, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(cv, W.data.astype(F))
    _check_csc(Cm, n, n)
    R = _mat(g, n, n, cp, ci, cv)
    srcs = [int(np.argmax(np.diff(cp))), int(np.nonzero(np.diff(cp))[0][7])]
    for s in srcs:
        for mode in (0, 1, 2):
            labels = []
            for X in (Cm, R):
                d = hb.descriptor(mxvmode=mode, struconly=1)
                v = g.Vector(n)
                info, _ = g.bfs(v, X, s, d, fused=True)
                assert info == 0
                labels.append(v.extractTuples()[1])
            assert np.array_equal(labels[0], labels[1]), (s, mode)
    rng = np.random.default_rng(2)
    u = rng.integers(0, 4, n).astype(F)
    for mode in (1, 2):
        outs = []
        for X in (Cm, R):
            uv, w = g.Vector(n, F), g.Vector(n, F)
            assert uv.build(u, n) == 0
            assert g.mxv(w, None, None, "PlusMultiplies", X, uv, hb.descriptor(mxvmode=mode)) == 0
            outs.append(hb.dense_values(w))
        assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), mode
        assert np.array_equal(outs[0].astype(np.float64), W @ u.astype(np.float64))


def test_transpose(hb):
    """of built matrices (f32, i32, rectangular, empty) and of a CSR-only product result, plain and with INP0 = TRAN
    (C = A with both orientations): rows ascending inside every column, the same bits from call to call, and a product
    with the result as a transposed operand"""
    import scipy.sparse as sp
    g = hb.g
    rng = np.random.default_rng(31)
    for dt in (F, I):
        m, n = 170, 90
        ap, ai = _rand_csr(rng, m, n, 4000)
        av = _vals(rng, ai.size, dt)
        A = _mat(g, m, n, ap, ai, av)
        T = g.Matrix(n, m, dt)
        assert g.transpose(T, None, None, A, hb.descriptor()) == 0
        _check(T.host_csr(), _transpose(m, n, ap, ai, av))
        _check_csc(T, n, m)
        T2 = g.Matrix(m, n, dt)
        assert g.transpose(T2, None, None, A, _desc(hb, ta=True)) == 0
        _check(T2.host_csr(), (ap, ai, av))
        _check_csc(T2, m, n)
        E = _mat(g, 5, 7, np.zeros(6, np.int32), np.zeros(0, np.int32), np.zeros(0, dt))
        Et = g.Matrix(7, 5, dt)
        assert g.transpose(Et, None, None, E, hb.descriptor()) == 0
        p, i, v = Et.host_csr()
        assert np.array_equal(p, np.zeros(8, np.int32)) and i.size == 0
    # a CSR-only product result: the sort path
    n, ptr, ind = _rmat(12, 4)
    val = rng.integers(1, 4, ind.size).astype(F)
    A = _mat(g, n, n, ptr, ind, val)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    pp, pi, pv = (x.copy() for x in P.host_csr())
    T = g.Matrix(n, n, F)
    assert g.transpose(T, None, None, P, hb.descriptor()) == 0
    want = _transpose(n, n, pp, pi, pv)
    _check(T.host_csr(), want)
    _check_csc(T, n, n)
    tp, ti, _ = T.host_csc()
    assert np.array_equal(tp, pp) and np.array_equal(ti, pi)            # C's CSC is P's CSR
    T1 = g.Matrix(n, n, F)
    assert g.transpose(T1, None, None, P, hb.descriptor()) == 0
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(T.host_csr(), T1.host_csr()))
    cp, ci, _ = T.host_csr()                                             # rows ascending within every column of P
    assert all((np.diff(ci[cp[r]:cp[r + 1]]) > 0).all() for r in range(0, n, 97))
    # INP0 = TRAN: P with both orientations; then P^T . A works and is right
    Q = g.Matrix(n, n, F)
    assert g.transpose(Q, None, None, P, _desc(hb, ta=True)) == 0
    _check(Q.host_csr(), (pp, pi, pv))
    _check_csc(Q, n, n)
    X = g.Matrix(n, n, F)
    assert g.mxm(X, None, None, "PlusMultiplies", P, A, _desc(hb, ta=True)) == g.GrB_INVALID_OBJECT
    assert g.mxm(X, None, None, "PlusMultiplies", Q, A, _desc(hb, ta=True)) == 0
    SP, SA = sp.csr_matrix((pv, pi, pp), shape=(n, n)), sp.csr_matrix((val, ind, ptr), shape=(n, n))
    rows = np.unique(np.r_[np.argsort(-np.diff(pp))[:20], rng.choice(n, 200, replace=False)])
    W = (SP.T.tocsr()[rows] @ SA).tocsr()
    W.sort_indices()
    xp, xi, xv = X.host_csr()
    for t, r in enumerate(rows):
        assert np.array_equal(xi[xp[r]:xp[r + 1]], W.indices[W.indptr[t]:W.indptr[t + 1]])
        assert np.allclose(xv[xp[r]:xp[r + 1]], W.data[W.indptr[t]:W.indptr[t + 1]], rtol=1e-6, atol=0)


def test_aliasing(hb):
    """C == A, C == B, C == mask, and transpose in place, each against the result in a fresh matrix"""
    g = hb.g
    rng = np.random.default_rng(12)
    m, n = 120, 140
    (ap, ai), (bp, bi), (mp, mi) = _rand_csr(rng, m, n, 3000), _rand_csr(rng, m, n, 3000), _rand_csr(rng, m, n, 6000)
    av, bv, mv = _vals(rng, ai.size, F), _vals(rng, bi.size, F), _vals(rng, mi.size, F)

    def fresh():
        return _mat(g, m, n, ap, ai, av), _mat(g, m, n, bp, bi, bv), _mat(g, m, n, mp, mi, mv)

    for add in (True, False):
        fn = g.eWiseAdd if add else g.eWiseMult
        A, B, Mk = fresh()
        Cm = g.Matrix(m, n, F)
        assert fn(Cm, Mk, None, "PlusMinus", A, B, hb.descriptor()) == 0
        want = [x.copy() for x in Cm.host_csr()]
        for which in range(3):
            A, B, Mk = fresh()
            target = (A, B, Mk)[which]
            assert fn(target, Mk, None, "PlusMinus", A, B, hb.descriptor()) == 0, which
            _check(target.host_csr(), want, str(which))
            _check_csc(target, m, n, str(which))
    sp_, si = _rand_csr(rng, m, m, 2000)                                # a square one for the in-place transpose
    sv = _vals(rng, si.size, F)
    S = _mat(g, m, m, sp_, si, sv)
    assert g.transpose(S, None, None, S, hb.descriptor()) == 0
    _check(S.host_csr(), _transpose(m, m, sp_, si, sv))
    _check_csc(S, m, m)


def test_errors_leave_c_unchanged(hb):
    g = hb.g
    rng = np.random.default_rng(4)
    m, n = 100, 80
    (ap, ai), (bp, bi) = _rand_csr(rng, m, n, 1500), _rand_csr(rng, m, n, 1500)
    av, bv = _vals(rng, ai.size, F), _vals(rng, bi.size, F)
    A, B = _mat(g, m, n, ap, ai, av), _mat(g, m, n, bp, bi, bv)
    Cm = g.Matrix(m, n, F)
    assert g.eWiseAdd(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
    before = [x.copy() for x in Cm.host_csr()]
    before_csc = [x.copy() for x in Cm.host_csc()]

    def unchanged():
        return all(np.array_equal(x, y) for x, y in zip(before, Cm.host_csr())) and \
            all(np.array_equal(x, y) for x, y in zip(before_csc, Cm.host_csc()))

    d = hb.descriptor()
    for fn in (g.eWiseAdd, g.eWiseMult):
        assert fn(Cm, None, None, "PlusMultiplies", A, None, d) == g.GrB_UNINITIALIZED_OBJECT
        assert fn(Cm, None, None, "PlusMultiplies", None, B, d) == g.GrB_UNINITIALIZED_OBJECT
        assert fn(Cm, None, None, "PlusMultiplies", A, g.Matrix(m, n, F), d) == g.GrB_UNINITIALIZED_OBJECT
        assert fn(Cm, g.Matrix(m, n, F), None, "PlusMultiplies", A, B, d) == g.GrB_UNINITIALIZED_OBJECT
        Ai = _mat(g, m, n, ap, ai, av.astype(I))
        assert fn(Cm, None, None, "PlusMultiplies", A, Ai, d) == g.GrB_NOT_IMPLEMENTED       # mixed types
        assert fn(Cm, None, None, "PlusMultiplies", Ai, Ai, d) == g.GrB_NOT_IMPLEMENTED      # C of another type
        R = g.Matrix(m, n - 1, F)
        rp, ri = _rand_csr(rng, m, n - 1, 100)
        assert R.build_csr(rp, ri, np.ones(ri.size, F)) == 0
        assert fn(Cm, None, None, "PlusMultiplies", A, R, d) == g.GrB_DIMENSION_MISMATCH
        assert fn(Cm, None, None, "PlusMultiplies", A, B, _desc(hb, tb=True)) == g.GrB_DIMENSION_MISMATCH   # B^T is 80 x 100
        assert fn(Cm, R, None, "PlusMultiplies", A, B, d) == g.GrB_DIMENSION_MISMATCH       # the mask's shape
        # a transposed operand without a CSC of its own: a product result
        sp_, si = _rand_csr(rng, n, n, 400)
        Sq = _mat(g, n, n, sp_, si, np.ones(si.size, F))
        P = g.Matrix(n, n, F)
        assert g.mxm(P, None, None, "PlusMultiplies", Sq, Sq, d) == 0
        Cq = g.Matrix(n, n, F)
        assert fn(Cq, None, None, "PlusMultiplies", Sq, Sq, d) == 0
        q_before = [x.copy() for x in Cq.host_csr()]
        assert fn(Cq, None, None, "PlusMultiplies", Sq, P, _desc(hb, tb=True)) == g.GrB_INVALID_OBJECT
        assert fn(Cq, None, None, "PlusMultiplies", P, Sq, _desc(hb, ta=True)) == g.GrB_INVALID_OBJECT
        assert all(np.array_equal(x, y) for x, y in zip(q_before, Cq.host_csr()))
        assert unchanged()
    # transpose
    T = g.Matrix(n, m, F)
    assert g.transpose(T, None, None, A, d) == 0
    tb_ = [x.copy() for x in T.host_csr()]
    assert g.transpose(T, A, None, A, d) == g.GrB_NOT_IMPLEMENTED                              # a mask
    assert g.transpose(T, None, None, _mat(g, m, n, ap, ai, av.astype(I)), d) == g.GrB_NOT_IMPLEMENTED
    assert g.transpose(T, None, None, None, d) == g.GrB_UNINITIALIZED_OBJECT
    assert g.transpose(T, None, None, g.Matrix(m, n, F), d) == g.GrB_UNINITIALIZED_OBJECT
    assert g.transpose(T, None, None, A, _desc(hb, ta=True)) == g.GrB_DIMENSION_MISMATCH
    assert all(np.array_equal(x, y) for x, y in zip(tb_, T.host_csr()))
    assert unchanged()


def test_int32_max_guard(hb):
    """two CSR-only matrices with disjoint columns, 2^30 entries each: the union has 2^31 entries -> GrB_OUT_OF_MEMORY
    before C's arrays are allocated, C unchanged; their intersection (empty) still works"""
    import torch
    g = hb.g
    dev = torch.device("cuda", 0)
    rows, k = 1 << 16, 1 << 14
    ptr = torch.arange(0, rows + 1, dtype=torch.int32, device=dev) * k
    cols_a = torch.arange(k, dtype=torch.int32, device=dev).repeat(rows)
    cols_b = cols_a + k
    vals = torch.ones(rows * k, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    A, B = g.Matrix(rows, 2 * k, F), g.Matrix(rows, 2 * k, F)
    assert A.build_device_csr(ptr.data_ptr(), cols_a.data_ptr(), vals.data_ptr(), rows * k, keep=(ptr, cols_a, vals)) == 0
    assert B.build_device_csr(ptr.data_ptr(), cols_b.data_ptr(), vals.data_ptr(), rows * k, keep=(ptr, cols_b, vals)) == 0
    Cm = g.Matrix(rows, 2 * k, F)
    small = _mat(g, rows, 2 * k, np.r_[np.zeros(rows, np.int32), 1].astype(np.int32), np.array([5], np.int32), np.array([2], F))
    assert g.eWiseAdd(Cm, None, None, "PlusMultiplies", small, small, hb.descriptor()) == 0
    kept = [x.copy() for x in Cm.host_csr()]
    assert g.eWiseAdd(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == g.GrB_OUT_OF_MEMORY
    assert all(np.array_equal(x, y) for x, y in zip(kept, Cm.host_csr()))
    assert g.eWiseMult(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
    assert Cm.nvals() == 0
    del A, B
    del cols_a, cols_b, vals, ptr
    torch.cuda.empty_cache()


def test_cpp_frontend(tmp_path):
    import scipy.sparse as sp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "ewise_matrix")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "ewise_matrix.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    mtx = os.path.join(root, "tests", "golden", "data", "chesapeake.mtx")
    lines = [ln for ln in subprocess.check_output([exe, mtx]).decode().split("\n") if ln.startswith(("csr ", "csc "))]
    assert len(lines) == 5, lines

    def parse(ln):
        t = ln.split("|")
        head = [int(x) for x in t[0].split()[1:]]
        return head, [np.array(x.split(), dtype=dt) for x, dt in zip(t[1:], (np.int32, np.int32, np.float32))]

    (nr, nc, _), (ap, ai, av) = parse(lines[0])
    S = sp.csr_matrix((av, ai, ap), shape=(nr, nc))
    P = (S @ S).tocsr()
    wants = [P + S, P.multiply(S), P.T, P.T.T]
    for ln, W in zip(lines[1:], wants):
        W = sp.csr_matrix(W)
        W.sort_indices()
        (r, c, nv), (p, i, v) = parse(ln)
        assert nv == W.nnz and ai.size > 0
        assert np.array_equal(p, W.indptr) and np.array_equal(i, W.indices) and np.array_equal(v, W.data.astype(F))
