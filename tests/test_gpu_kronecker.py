"""kronecker on the device (csrc/kronecker.hip): C = op(A) (x) op(B) against a numpy restatement of the definition in
include/grb_hip.h -- every built-in multiply and a registered one, both element types and the four reads of A and B, entry
counts around the kernel's tile, a row of C over many tiles, runs of empty rows, degenerate shapes and empty operands, the
algebraic identities that tie it to mxm, transpose, select and the triangle count, a CSR-only input, aliasing, every error
code with C unchanged, determinism and the C++ frontend.  Values are small integers (stored zeros among them; the divisors
1 .. 4), so every comparison is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
T = 2048                                                 # kKronTile: the positions of C one workgroup writes

# the multiply of each built-in semiring (csrc/common.hpp: GRB_DEF_SR)
MUL = {"LogicalOrAnd": "land", "PlusMultiplies": "times", "MinimumPlus": "plus", "MaximumMultiplies": "times",
       "PlusDivides": "div", "PlusGreater": "gt", "GreaterPlus": "plus", "PlusMinus": "minus", "PlusLess": "lt",
       "CustomLessPlus": "plus", "MinimumMultiplies": "times", "MultipliesMultiplies": "times", "NotEqualToPlus": "plus",
       "MinimumSelectSecond": "second", "PlusNotEqualTo": "ne", "CustomLessLess": "lt", "MinimumNotEqualTo": "ne"}


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


def _mul(name, a, b):
    """csrc/common.hpp's binop<OP, T> on arrays of one element type (the values here are never negative, so an integer
    division that truncates is one that floors)"""
    dt = a.dtype.type
    if name == "land":
        return ((a != 0) & (b != 0)).astype(dt)
    if name == "gt":
        return (a > b).astype(dt)
    if name == "lt":
        return (a < b).astype(dt)
    if name == "ne":
        return (a != b).astype(dt)
    if name == "second":
        return b.copy()
    if name == "plus":
        return a + b
    if name == "minus":
        return a - b
    if name == "times":
        return a * b
    assert name == "div"
    if a.dtype == np.int32:
        return np.where(b == 0, 0, a // np.where(b == 0, 1, b)).astype(dt)
    return a / b


def _rand_csr(rng, m, n, nnz):
    """m x n, sorted rows, no duplicates, exactly nnz entries"""
    key = np.sort(rng.choice(m * n, nnz, replace=False).astype(np.int64))
    ptr = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(key // n, minlength=m), out=ptr[1:])
    return ptr, (key % n).astype(np.int32)


def _from_lens(rng, lens, n):
    """rows of the given lengths over n columns"""
    ptr = np.zeros(len(lens) + 1, np.int32)
    np.cumsum(lens, out=ptr[1:])
    parts = [np.sort(rng.choice(n, k, replace=False)) for k in lens if k]
    return ptr, (np.concatenate(parts) if parts else np.zeros(0)).astype(np.int32)


def _transpose(m, n, p, i, v):
    """the n x m transpose of an m x n CSR (rows ascending within every column)"""
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(p))
    order = np.lexsort((rows, i))
    tp = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(i, minlength=n), out=tp[1:])
    return tp, rows[order].astype(np.int32), v[order]


def _vals(rng, size, dt, lo=0):
    return rng.integers(lo, 5, size).astype(dt)          # lo = 0: a fifth of the stored values are zeros


def _mat(g, m, n, p, i, v):
    M = g.Matrix(m, n, v.dtype)
    assert M.build_csr(p, i, v) == 0
    return M


def _stored(g, m, n, p, i, v, tran):
    """the matrix whose op() under `tran` is the m x n (p, i, v)"""
    return _mat(g, n, m, *_transpose(m, n, p, i, v)) if tran else _mat(g, m, n, p, i, v)


def _desc(hb, ta=False, tb=False):
    d = hb.descriptor()
    if ta:
        assert d.toggle(hb.g.GrB_INP0) == 0
    if tb:
        assert d.toggle(hb.g.GrB_INP1) == 0
    return d


def _expect(a, b, mul):
    """The definition: a = (mA, nA, ptr, ind, val) and b likewise.  Row iA * mB + iB begins at
    ptrA[iA] * nnzB + lenA(iA) * ptrB[iB]; its entry t pairs A's entry t // lenB(iB) of row iA with B's entry t % lenB(iB)
    of row iB."""
    mA, nA, pA, iA, vA = a
    mB, nB, pB, iB, vB = b
    pA64, pB64 = pA.astype(np.int64), pB.astype(np.int64)
    lenA, lenB = np.diff(pA64), np.diff(pB64)
    nnzB, nnz = int(pB64[-1]), int(pA64[-1]) * int(pB64[-1])
    ptr = np.empty(mA * mB + 1, np.int64)
    ptr[:-1] = (np.repeat(pA64[:-1], mB) * nnzB + np.repeat(lenA, mB) * np.tile(pB64[:-1], mA))
    ptr[-1] = nnz
    assert nnz <= 2 ** 31 - 1
    lens = np.diff(ptr)
    assert np.array_equal(lens, np.repeat(lenA, mB) * np.tile(lenB, mA))
    rows = np.repeat(np.arange(mA * mB, dtype=np.int64), lens)
    t = np.arange(nnz, dtype=np.int64) - np.repeat(ptr[:-1], lens)
    ra, rb = rows // mB, rows % mB
    ea = pA64[ra] + t // np.maximum(lenB[rb], 1)
    eb = pB64[rb] + t % np.maximum(lenB[rb], 1)
    ind = (iA.astype(np.int64)[ea] * nB + iB.astype(np.int64)[eb]).astype(np.int32)
    with np.errstate(all="ignore"):
        val = _mul(mul, vA[ea], vB[eb])
    assert val.dtype == vA.dtype
    return ptr.astype(np.int32), ind, val


def _same(got, want, name=""):
    for x, y in zip(got, want):
        assert x.shape == y.shape, (name, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint32) if x.dtype != np.int32 else x, y.view(np.uint32) if y.dtype != np.int32 else y), name


def _check_csc(C, m, n, name=""):
    """C's CSC holds the same entries and bits as the transpose of its CSR"""
    p, i, v = C.host_csr()
    _same(C.host_csc(), _transpose(m, n, p, i, v), name)


def _check(hb, a, b, op="PlusMultiplies", mul="times", ta=False, tb=False, name=""):
    """kronecker of op(A) = a and op(B) = b: the definition's CSR, and the exact transpose of it as the CSC"""
    g = hb.g
    A, B = _stored(g, *a, ta), _stored(g, *b, tb)
    m, n = a[0] * b[0], a[1] * b[1]
    Cm = g.Matrix(m, n, a[4].dtype)
    assert g.kronecker(Cm, None, None, op, A, B, _desc(hb, ta, tb)) == 0, (name, op)
    want = _expect(a, b, mul)
    _same(Cm.host_csr(), want, (name, op))
    assert Cm.nvals() == want[1].size == A.nvals() * B.nvals()
    _check_csc(Cm, m, n, (name, op))
    return Cm


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("ta", [False, True])
@pytest.mark.parametrize("tb", [False, True])
def test_every_operator(hb, dt, ta, tb):
    """the 17 built-in semirings and a registered (max, minus), f32 and i32, the four combinations of INP0 / INP1 = TRAN: a
    7 x 5 A of 11 entries against a 4 x 6 B of 9; B's values 1 .. 4 for divides"""
    g = hb.g
    rng = np.random.default_rng(71)
    pa, ia = _rand_csr(rng, 7, 5, 11)
    pb, ib = _rand_csr(rng, 4, 6, 9)
    va, vb0, vb1 = _vals(rng, 11, dt), _vals(rng, 9, dt), _vals(rng, 9, dt, lo=1)
    va[0], vb0[0] = 0, 0                                 # stored zeros, whatever the draw
    sid = g.register_semiring("maximum", 0.0, "minus")
    assert sid >= 64
    for name, op, mul in [(s, s, m) for s, m in MUL.items()] + [("registered", sid, "minus")]:
        vb = vb1 if mul == "div" else vb0
        _check(hb, (7, 5, pa, ia, va), (4, 6, pb, ib, vb), op, mul, ta, tb, name)


def test_tile_edges(hb):
    """nnz(A) * nnz(B) = T - 1, T, T + 1, 2T, 2T + 1 for the kernel's tile of T positions: through a one-entry B (in a
    2 x 3 B, so with an empty row) and through two factors above 1"""
    rng = np.random.default_rng(72)
    one = (2, 3, np.array([0, 0, 1], np.int32), np.array([2], np.int32), np.array([3], F))
    for nnz in (T - 1, T, T + 1, 2 * T, 2 * T + 1):
        pa, ia = _rand_csr(rng, 90, 70, nnz)
        Cm = _check(hb, (90, 70, pa, ia, _vals(rng, nnz, F)), one, name=nnz)
        assert Cm.nvals() == nnz
    for fa, fb in ((23, 89), (64, 32), (3, 683), (64, 64), (17, 241)):
        assert fa * fb in (T - 1, T, T + 1, 2 * T, 2 * T + 1)
        pa, ia = _rand_csr(rng, 9, 11, fa)
        pb, ib = _rand_csr(rng, 31, 29, fb)
        for dt in (F, I):
            _check(hb, (9, 11, pa, ia, _vals(rng, fa, dt)), (31, 29, pb, ib, _vals(rng, fb, dt)), name=(fa, fb))


def test_row_shapes(hb):
    rng = np.random.default_rng(73)
    # a 300-entry row of A against a 300-entry row of B: one row of C of 90000 entries, over 44 tiles
    pa, ia = _from_lens(rng, [2, 300, 0, 5], 400)
    pb, ib = _from_lens(rng, [300, 1, 7], 350)
    for dt in (F, I):
        Cm = _check(hb, (4, 400, pa, ia, _vals(rng, ia.size, dt)), (3, 350, pb, ib, _vals(rng, ib.size, dt)), name="hub")
        assert np.diff(Cm.host_csr()[0]).max() == 90000
    # 5000 consecutive empty rows of A between two stored rows: 15000 consecutive empty rows of C inside one tile
    pa, ia = _from_lens(rng, [3] + [0] * 5000 + [4], 6)
    pb, ib = _from_lens(rng, [2, 0, 3], 5)
    a, b = (5002, 6, pa, ia, _vals(rng, 7, F)), (3, 5, pb, ib, _vals(rng, 5, F))
    _check(hb, a, b, name="empty rows of A")
    _check(hb, b, a, name="empty rows of B")             # ... and the same run in every block of B's rows
    # B with an empty first and an empty last row (and A with both, too)
    pb, ib = _from_lens(rng, [0, 4, 0, 2, 0], 9)
    pa, ia = _from_lens(rng, [0, 3, 5, 0], 8)
    _check(hb, (4, 8, pa, ia, _vals(rng, 8, F)), (5, 9, pb, ib, _vals(rng, 6, F)), name="empty first and last")
    # 1 x 1 operands, 1 x n against m x 1
    p1, i1 = np.array([0, 1], np.int32), np.array([0], np.int32)
    pr, ir = _rand_csr(rng, 40, 30, 500)
    big = (40, 30, pr, ir, _vals(rng, 500, F))
    _check(hb, (1, 1, p1, i1, np.array([3], F)), big, name="A 1 x 1")
    Cm = _check(hb, big, (1, 1, p1, i1, np.array([3], F)), name="B 1 x 1")
    _same(Cm.host_csr(), (pr, ir, big[4] * F(3)), "C = 3 A")
    _check(hb, (1, 1, p1, i1, np.array([2], F)), (1, 1, p1, i1, np.array([4], F)), name="1 x 1 both")
    prow, irow = _from_lens(rng, [700], 1000)
    pcol, icol = _transpose(1, 900, *_from_lens(rng, [600], 900), np.zeros(600, F))[:2]
    row, col = (1, 1000, prow, irow, _vals(rng, 700, F)), (900, 1, pcol, icol, _vals(rng, 600, F))
    _check(hb, row, col, name="1 x n (x) m x 1")
    _check(hb, col, row, name="m x 1 (x) 1 x n")
    # an operand with no entries, in each position
    pe, ie = _rand_csr(rng, 6, 4, 0)
    none = (6, 4, pe, ie, np.zeros(0, F))
    for a, b in ((none, big), (big, none), (none, none)):
        for ta, tb in ((False, False), (True, True)):
            Cm = _check(hb, a, b, ta=ta, tb=tb, name="no entries")
            assert Cm.nvals() == 0 and not Cm.host_csr()[0].any() and not Cm.host_csc()[0].any()


def test_identities(hb):
    """(A (x) B) . (C (x) D) = (A . C) (x) (B . D) through the unmasked f32 mxm (whose results are CSR only);
    transpose(A (x) B) = A^T (x) B^T; nvals; all on 0 / 1 patterns, exact"""
    g = hb.g
    rng = np.random.default_rng(74)
    d = hb.descriptor()
    shapes = {"A": (12, 9), "B": (5, 7), "C": (9, 8), "D": (7, 6)}
    M = {}
    for k, (m, n) in shapes.items():
        p, i = _rand_csr(rng, m, n, m * n // 3)
        M[k] = _mat(g, m, n, p, i, np.ones(i.size, F))
    AB, CD, L = g.Matrix(60, 63, F), g.Matrix(63, 48, F), g.Matrix(60, 48, F)
    assert g.kronecker(AB, None, None, "PlusMultiplies", M["A"], M["B"], d) == 0
    assert g.kronecker(CD, None, None, "PlusMultiplies", M["C"], M["D"], d) == 0
    assert AB.nvals() == M["A"].nvals() * M["B"].nvals() and CD.nvals() == M["C"].nvals() * M["D"].nvals()
    assert g.mxm(L, None, None, "PlusMultiplies", AB, CD, d) == 0
    AC, BD, R = g.Matrix(12, 8, F), g.Matrix(5, 6, F), g.Matrix(60, 48, F)
    assert g.mxm(AC, None, None, "PlusMultiplies", M["A"], M["C"], d) == 0
    assert g.mxm(BD, None, None, "PlusMultiplies", M["B"], M["D"], d) == 0
    assert g.kronecker(R, None, None, "PlusMultiplies", AC, BD, d) == 0             # CSR-only inputs
    assert R.nvals() == AC.nvals() * BD.nvals() > 0
    _same(R.host_csr(), L.host_csr(), "mixed product")
    # transpose(A (x) B) = A^T (x) B^T: grb_transpose of the product, and the product of the transposed reads
    Tr, Kt = g.Matrix(63, 60, F), g.Matrix(63, 60, F)
    assert g.transpose(Tr, None, None, AB, d) == 0
    assert g.kronecker(Kt, None, None, "PlusMultiplies", M["A"], M["B"], _desc(hb, True, True)) == 0
    _same(Kt.host_csr(), Tr.host_csr(), "transpose")
    _same(Kt.host_csc(), Tr.host_csc(), "transpose, CSC")
    _same(Kt.host_csr(), AB.host_csc(), "transpose = the CSC")


def test_triangles_of_a_kronecker_square(hb):
    """chesapeake, symmetrised and loop-free, with itself: trace((A (x) A)^3) = trace(A^3)^2, so the square has 6 t^2
    triangles where A has t; both counts by grb_tc on select(tril, -1)"""
    import scipy.io
    import scipy.sparse as sp
    g = hb.g
    root = os.path.dirname(os.path.abspath(__file__))
    S = sp.csr_matrix(scipy.io.mmread(os.path.join(root, "golden", "data", "chesapeake.mtx")))
    S = ((S + S.T) != 0).astype(np.int32).tolil()
    S.setdiag(0)
    S = S.tocsr()
    S.eliminate_zeros()
    S.sort_indices()
    n = S.shape[0]
    A = _mat(g, n, n, S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, I))
    K = g.Matrix(n * n, n * n, I)
    d = hb.descriptor()
    assert g.kronecker(K, None, None, "PlusMultiplies", A, A, d) == 0
    assert K.nvals() == S.nnz ** 2
    counts = []
    for X, dim in ((A, n), (K, n * n)):
        L = g.Matrix(dim, dim, I)
        assert g.select(L, None, None, "tril", X, -1, d) == 0
        assert 2 * L.nvals() == X.nvals()                                           # symmetric, no loops
        info, ntri, _ = g.tc(L, g.Matrix(dim, dim, I), hb.descriptor())
        assert info == 0
        counts.append(ntri)
    assert counts[0] > 0 and counts[1] == 6 * counts[0] ** 2, counts


def test_csr_only_input(hb):
    """a product result has no CSC: its kronecker product is CSR only, in either position, and reading it transposed is
    GrB_INVALID_OBJECT with C unchanged"""
    g = hb.g
    rng = np.random.default_rng(75)
    n = 30
    ap, ai = _rand_csr(rng, n, n, 120)
    A = _mat(g, n, n, ap, ai, rng.integers(1, 3, ai.size).astype(F))
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    pp, pi, pv = (x.copy() for x in P.host_csr())
    bp, bi = _rand_csr(rng, 4, 6, 9)
    b = (4, 6, bp, bi, _vals(rng, 9, F))
    B = _mat(g, *b)
    for first in (True, False):
        Cm = g.Matrix(4 * n, 6 * n, F)
        X, Y = (P, B) if first else (B, P)
        x, y = ((n, n, pp, pi, pv), b) if first else (b, (n, n, pp, pi, pv))
        assert g.kronecker(Cm, None, None, "PlusMultiplies", X, Y, hb.descriptor()) == 0
        _same(Cm.host_csr(), _expect(x, y, "times"))
        with pytest.raises(g._lib.GrbError) as e:
            Cm.host_csc()
        assert e.value.info == g.GrB_NO_VALUE
        kept = [v.copy() for v in Cm.host_csr()]
        Ct = g.Matrix(6 * n, 4 * n, F)
        assert g.kronecker(Ct, None, None, "PlusMultiplies", X, Y, _desc(hb, True, True)) == g.GrB_INVALID_OBJECT
        assert g.kronecker(Cm, None, None, "PlusMultiplies", X, Y, _desc(hb, first, not first)) == g.GrB_INVALID_OBJECT
        _same(Cm.host_csr(), kept)


def test_aliasing(hb):
    """C is A, C is B, C is both: 1 x 1 (x) 1 x 1, and a 1 x 1 operand with C the other one"""
    g = hb.g
    rng = np.random.default_rng(76)
    d = hb.descriptor()
    p1, i1 = np.array([0, 1], np.int32), np.array([0], np.int32)
    one = lambda x: _mat(g, 1, 1, p1, i1, np.array([x], F))
    X, Y = one(3), one(5)
    assert g.kronecker(X, None, None, "PlusMinus", X, Y, d) == 0                     # C is A: 3 - 5
    _same(X.host_csr(), (p1, i1, np.array([-2], F)))
    assert g.kronecker(Y, None, None, "PlusMinus", X, Y, d) == 0                     # C is B: -2 - 5
    _same(Y.host_csr(), (p1, i1, np.array([-7], F)))
    assert g.kronecker(Y, None, None, "PlusMultiplies", Y, Y, d) == 0                # C is A is B
    _same(Y.host_csr(), (p1, i1, np.array([49], F)))
    _check_csc(Y, 1, 1)
    p, i = _rand_csr(rng, 60, 50, 2100)                  # more than one tile
    v = _vals(rng, i.size, F)
    big = (60, 50, p, i, v)
    s = (1, 1, p1, i1, np.array([2], F))
    B = _mat(g, *big)
    assert g.kronecker(B, None, None, "PlusMinus", one(2), B, d) == 0                # a 1 x 1 A, C is B
    _same(B.host_csr(), _expect(s, big, "minus"))
    _check_csc(B, 60, 50)
    A = _mat(g, *big)
    assert g.kronecker(A, None, None, "PlusMinus", A, one(2), d) == 0                # a 1 x 1 B, C is A
    _same(A.host_csr(), _expect(big, s, "minus"))
    _check_csc(A, 60, 50)


def test_errors_leave_c_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(77)
    pa, ia = _rand_csr(rng, 7, 5, 11)
    pb, ib = _rand_csr(rng, 4, 6, 9)
    va, vb = _vals(rng, 11, F), _vals(rng, 9, F)
    A, B = _mat(g, 7, 5, pa, ia, va), _mat(g, 4, 6, pb, ib, vb)
    Ai, Bi = _mat(g, 7, 5, pa, ia, va.astype(I)), _mat(g, 4, 6, pb, ib, vb.astype(I))
    d = hb.descriptor()
    Cm, Ci = g.Matrix(28, 30, F), g.Matrix(28, 30, I)
    assert g.kronecker(Cm, None, None, "MinimumPlus", A, B, d) == 0
    assert g.kronecker(Ci, None, None, "MinimumPlus", Ai, Bi, d) == 0
    before = {id(X): [x.copy() for x in X.host_csr()] + [x.copy() for x in X.host_csc()] for X in (Cm, Ci)}

    def unchanged(*Xs):
        return all(np.array_equal(x, y) for X in Xs for x, y in zip(before[id(X)], list(X.host_csr()) + list(X.host_csc())))

    call = lambda C_, A_, B_, op=1, mask=None: lib.grb_kronecker(C_, mask, 0, op, A_, B_, d._h)
    assert call(None, A._h, B._h) == g.GrB_UNINITIALIZED_OBJECT                     # null handles
    assert call(Cm._h, None, B._h) == g.GrB_UNINITIALIZED_OBJECT
    assert call(Cm._h, A._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert g.kronecker(Cm, None, None, "PlusMultiplies", g.Matrix(7, 5, F), B, d) == g.GrB_UNINITIALIZED_OBJECT   # unbuilt
    assert g.kronecker(Cm, None, None, "PlusMultiplies", A, g.Matrix(4, 6, F), d) == g.GrB_UNINITIALIZED_OBJECT
    assert unchanged(Cm, Ci)
    assert g.kronecker(g.Matrix(28, 31, F), None, None, "PlusMultiplies", A, B, d) == g.GrB_DIMENSION_MISMATCH
    assert g.kronecker(g.Matrix(30, 28, F), None, None, "PlusMultiplies", A, B, d) == g.GrB_DIMENSION_MISMATCH
    assert g.kronecker(Cm, None, None, "PlusMultiplies", A, B, _desc(hb, True, False)) == g.GrB_DIMENSION_MISMATCH   # 20 x 42
    assert g.kronecker(Cm, None, None, "PlusMultiplies", A, B, _desc(hb, False, True)) == g.GrB_DIMENSION_MISMATCH   # 42 x 20
    assert unchanged(Cm, Ci)
    assert g.kronecker(Cm, None, None, "PlusMultiplies", Ai, B, d) == g.GrB_NOT_IMPLEMENTED    # f32 / i32
    assert g.kronecker(Cm, None, None, "PlusMultiplies", A, Bi, d) == g.GrB_NOT_IMPLEMENTED
    assert g.kronecker(Ci, None, None, "PlusMultiplies", A, B, d) == g.GrB_NOT_IMPLEMENTED
    assert g.kronecker(Cm, Cm, None, "PlusMultiplies", A, B, d) == g.GrB_NOT_IMPLEMENTED       # a mask
    assert unchanged(Cm, Ci)
    for sid in (-1, 17, 64 + 100000):                                               # no such semiring
        assert call(Cm._h, A._h, B._h, op=sid) == g.GrB_INVALID_VALUE, sid
        assert call(Ci._h, Ai._h, Bi._h, op=sid) == g.GrB_INVALID_VALUE, sid
    assert unchanged(Cm, Ci)
    # a transposed operand without a CSC of its own
    sq = _mat(g, 5, 5, *_rand_csr(rng, 5, 5, 10), np.ones(10, F))
    P = g.Matrix(5, 5, F)
    assert g.mxm(P, None, None, "PlusMultiplies", sq, sq, d) == 0
    C2 = g.Matrix(20, 30, F)
    assert g.kronecker(C2, None, None, "PlusMultiplies", P, B, d) == 0
    kept = [x.copy() for x in C2.host_csr()]
    assert g.kronecker(C2, None, None, "PlusMultiplies", P, B, _desc(hb, True, False)) == g.GrB_INVALID_OBJECT
    C3 = g.Matrix(35, 25, F)
    assert g.kronecker(C3, None, None, "PlusMultiplies", A, P, d) == 0
    assert g.kronecker(C3, None, None, "PlusMultiplies", A, P, _desc(hb, False, True)) == g.GrB_INVALID_OBJECT
    _same(C2.host_csr(), kept)
    # more than INT32_MAX entries: 1 x 50000 (dense) (x) 50000 x 1 (dense), 2.5e9 of them, into a 50000 x 50000 C
    n = 50000
    row = _mat(g, 1, n, np.array([0, n], np.int32), np.arange(n, dtype=np.int32), np.ones(n, F))
    col = _mat(g, n, 1, np.arange(n + 1, dtype=np.int32), np.zeros(n, np.int32), np.ones(n, F))
    hp, hi = _rand_csr(rng, n, n, 1000)
    hv = _vals(rng, 1000, F)
    Big = _mat(g, n, n, hp, hi, hv)
    held = [x.copy() for x in Big.host_csr()] + [x.copy() for x in Big.host_csc()]
    for x, y in ((row, col), (col, row)):
        assert g.kronecker(Big, None, None, "PlusMultiplies", x, y, d) == g.GrB_OUT_OF_MEMORY
        assert g.kronecker(Big, None, None, "PlusMultiplies", x, y, _desc(hb, True, True)) == g.GrB_OUT_OF_MEMORY
    _same(list(Big.host_csr()) + list(Big.host_csc()), held)
    assert Big.nvals() == 1000
    assert unchanged(Cm, Ci)
    # a null descriptor means the defaults
    Cn = g.Matrix(28, 30, F)
    assert g.kronecker(Cn, None, None, "MinimumPlus", A, B, None) == 0
    _same(Cn.host_csr(), before[id(Cm)][:3])


def test_determinism(hb):
    """RMAT-8 (x) RMAT-8 (a hub row against a hub row, a few million entries): two calls, the same bytes in both orientations"""
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    g = hb.g
    s, dd, n = rmat_edges(8, 8, seed=5)
    gr = finalize_edges(s, dd, n, symmetrize=True)
    p, i = (np.asarray(x).astype(np.int32) for x in gr["csr"])
    rng = np.random.default_rng(78)
    A = _mat(g, n, n, p, i, _vals(rng, i.size, F))
    B = _mat(g, n, n, p, i, _vals(rng, i.size, F))
    assert np.diff(p).max() ** 2 > 4 * T                                            # a row of C over several tiles
    outs = []
    for _ in range(2):
        Cm = g.Matrix(n * n, n * n, F)
        assert g.kronecker(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
        assert Cm.nvals() == i.size ** 2
        outs.append([x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()])
    _same(outs[0], outs[1])
    assert all(x.tobytes() == y.tobytes() for x, y in zip(outs[0], outs[1]))
    # ... and the definition's row lengths
    lens = np.diff(p).astype(np.int64)
    assert np.array_equal(np.diff(outs[0][0]), np.repeat(lens, n) * np.tile(lens, n))


def test_cpp_frontend(tmp_path):
    """tests/tools/kronecker.cpp: a 2 x 2 against a 2 x 3 literal, PlusMultiplies and MinimumPlus"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "kronecker")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "kronecker.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln.split(" ")[0] in ("kron", "kronT", "minplus")]
    # A = [[1 2] [. 3]], B = [[1 . 2] [. 3 .]]
    assert lines == ["kron 4 6 9 | 0 4 6 8 9 | 0 2 3 5 1 4 3 5 4 | 1 2 2 4 3 6 3 6 9",
                     "kronT 4 6 9 | 0 1 2 3 5 7 9 | 0 1 0 0 2 1 3 0 2 | 1 3 2 2 3 6 9 4 6",
                     "minplus 4 6 9 | 0 4 6 8 9 | 0 2 3 5 1 4 3 5 4 | 2 3 3 4 4 5 4 5 6"], lines
