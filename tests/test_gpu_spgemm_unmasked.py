"""The unmasked product C = op(A) (+.x) op(B) (csrc/spgemm.hip; grb_mxm with a null mask) for f32 matrices: every
semiring against a numpy restatement of the ascending-k fold, the four orientations, stored zeros, rectangular and
degenerate shapes, hub rows on RMAT graphs against scipy, determinism, chaining, the error codes and the C++ frontend."""
import os
import subprocess

import numpy as np
import pytest

from backends import HipBackend
from mxm_masked_cases import fold as _fold        # the ascending-k join, shared with the masked product's tests

pytestmark = pytest.mark.gpu

F = np.float32
INT32_MAX = 2**31 - 1


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


def _rand_csr(rng, m, n, nnz):
    """m x n, sorted rows, no duplicates (finalize_edges on a square index space, cut to the shape)"""
    from graphblast_amd.graphgen import finalize_edges
    big = max(m, n)
    gr = finalize_edges(rng.integers(0, m, nnz), rng.integers(0, n, nnz), big, symmetrize=False)
    ptr, ind = gr["csr"]
    return np.ascontiguousarray(ptr[:m + 1], dtype=np.int32), np.ascontiguousarray(ind[:ptr[m]], dtype=np.int32)


def _transpose(m, n, p, i, v):
    import scipy.sparse as sp
    t = sp.csr_matrix((v, i, p), shape=(m, n)).T.tocsr()
    t.sort_indices()
    return t.indptr.astype(np.int32), t.indices.astype(np.int32), t.data.astype(v.dtype)


class _Registered:
    """a registered semiring restated with the oracle's operators (max, +) with identity 0"""
    def __init__(self, add, ident, mul):
        from oracle.semiring import binary_op
        self.add_op, self.mul_op, self._id = binary_op(add, F), binary_op(mul, F), F(ident)

    def identity(self):
        return self._id


def _desc(hb, ta, tb):
    g = hb.g
    d = hb.descriptor()
    if ta:
        assert d.toggle(g.GrB_INP0) == 0
    if tb:
        assert d.toggle(g.GrB_INP1) == 0
    return d


def _mat(g, m, n, p, i, v):
    M = g.Matrix(m, n, F)
    assert M.build_csr(p, i, v) == 0
    return M


def _check(got, want, name=""):
    cp, ci, cv = got
    wp, wi, wv = want
    assert np.array_equal(cp, wp), name
    assert np.array_equal(ci, wi), name
    if name == "PlusDivides":
        assert np.allclose(cv, wv, rtol=4e-7, atol=0, equal_nan=True), name
    else:
        assert np.array_equal(cv.view(np.uint32), wv.view(np.uint32)) or np.array_equal(cv, wv, equal_nan=True), \
            (name, int((cv != wv).sum()))


def test_every_semiring_and_orientation(hb):
    """all 17 built-in semirings and one registered one, A != B, four orientations, stored zeros"""
    from oracle.semiring import Semiring, SEMIRINGS
    g = hb.g
    rng = np.random.default_rng(17)
    n = 300
    (ap, ai), (bp, bi) = _rand_csr(rng, n, n, 6000), _rand_csr(rng, n, n, 6000)
    av = rng.integers(0, 5, ai.size).astype(F)              # a fifth of the stored values are zeros: kept
    bv = rng.integers(0, 5, bi.size).astype(F)
    A, B = _mat(g, n, n, ap, ai, av), _mat(g, n, n, bp, bi, bv)
    sid = g.register_semiring("maximum", 0.0, "plus")
    cases = [(name, name, Semiring(name, F)) for name in SEMIRINGS] + [("registered", sid, _Registered("maximum", 0.0, "plus"))]
    for ta in (False, True):
        for tb in (False, True):
            d = _desc(hb, ta, tb)
            oa = _transpose(n, n, ap, ai, av) if ta else (ap, ai, av)
            ob = _transpose(n, n, bp, bi, bv) if tb else (bp, bi, bv)
            for label, op, sr in cases:
                Cm = g.Matrix(n, n, F)
                assert g.mxm(Cm, None, None, op, A, B, d) == 0, (label, ta, tb)
                _check(Cm.host_csr(), _fold(sr, n, n, *oa, *ob), label)


def _bins(ap, ai, bp):
    """rows per bin of spgemm.hip for op(A) = (ap, ai), op(B) row pointers bp: tiny16, tiny64, mid, wide"""
    m = ap.size - 1
    ub = np.bincount(np.repeat(np.arange(m), np.diff(ap)), weights=np.diff(bp)[ai], minlength=m)
    da = np.diff(ap)
    nz = ub > 0
    t16 = nz & (ub <= 16) & (da <= 16)
    t64 = nz & ~t16 & (ub <= 64) & (da <= 64)
    mid = nz & ~t16 & ~t64 & (ub <= 1024)
    return [int(x.sum()) for x in (t16, t64, mid, nz & (ub > 1024))]


def _stored(g, m, n, p, i, v, tran):
    """the matrix whose op() under `tran` is the m x n (p, i, v): itself, or its transpose stored"""
    if not tran:
        return _mat(g, m, n, p, i, v)
    return _mat(g, n, m, *_transpose(m, n, p, i, v))


@pytest.mark.parametrize("case", ["tiny", "tiny_mixed", "wide_windows"])
def test_every_semiring_in_every_bin(hb, case):
    """the same semirings and orientations on inputs whose rows land in each numeric kernel: short rows (the 16- and
    64-lane groups), and rows of more than 1 024 products with more than 64 entries over several 4 096-column windows
    with an empty stretch between them (the window kernel).  The non-order-free monoids see the fold's order."""
    from oracle.semiring import Semiring, SEMIRINGS
    g = hb.g
    rng = np.random.default_rng({"tiny": 61, "tiny_mixed": 62, "wide_windows": 63}[case])
    if case == "wide_windows":
        m, k, n = 40, 3000, 13000
        ap, ai = _rand_csr(rng, m, k, 4200)                          # ~100 entries per row
        bp, bi = _rand_csr(rng, k, n, 80000)                          # ~26 per row
        # columns in two clusters, [0, 4000) and [9000, 13000): an empty window between them
        keep = (bi < 4000) | (bi >= 9000)
        rows = np.repeat(np.arange(k), np.diff(bp))[keep]
        bi = bi[keep]
        bp = np.r_[0, np.cumsum(np.bincount(rows, minlength=k))].astype(np.int32)
    else:
        m = k = n = 300
        nnz = 600 if case == "tiny" else 2000
        ap, ai = _rand_csr(rng, m, k, nnz)
        bp, bi = _rand_csr(rng, k, n, nnz)
    av = rng.integers(0, 5, ai.size).astype(F)
    bv = rng.integers(0, 5, bi.size).astype(F)
    bins = _bins(ap, ai, bp)
    if case == "tiny":
        assert bins[0] > 200 and bins[3] == 0, bins
    elif case == "tiny_mixed":
        assert bins[0] > 0 and bins[1] > 100, bins
    else:
        assert bins[3] == m and np.diff(ap).min() > 64 and bi.max() > 2 * 4096, (bins, int(np.diff(ap).min()))
    sid = g.register_semiring("maximum", 0.0, "plus")
    cases = [(name, name, Semiring(name, F)) for name in SEMIRINGS] + [("registered", sid, _Registered("maximum", 0.0, "plus"))]
    for ta in (False, True):
        for tb in (False, True):
            d = _desc(hb, ta, tb)
            A, B = _stored(g, m, k, ap, ai, av, ta), _stored(g, k, n, bp, bi, bv, tb)
            for label, op, sr in cases:
                Cm = g.Matrix(m, n, F)
                assert g.mxm(Cm, None, None, op, A, B, d) == 0, (label, ta, tb)
                _check(Cm.host_csr(), _fold(sr, m, n, ap, ai, av, bp, bi, bv), label)


def test_rectangular_and_degenerate_shapes(hb):
    from oracle.semiring import Semiring
    g = hb.g
    rng = np.random.default_rng(3)
    sr = Semiring("PlusMultiplies", F)
    m, k, n = 37, 53, 71
    ap, ai = _rand_csr(rng, m, k, 400)
    bp, bi = _rand_csr(rng, k, n, 500)
    # empty rows in A and in B
    keep_a = ~np.isin(np.repeat(np.arange(m), np.diff(ap)), [0, 5, 36])
    keep_b = ~np.isin(np.repeat(np.arange(k), np.diff(bp)), [1, 2, 52])
    ap = np.r_[0, np.cumsum(np.bincount(np.repeat(np.arange(m), np.diff(ap))[keep_a], minlength=m))].astype(np.int32)
    ai = ai[keep_a]
    bp = np.r_[0, np.cumsum(np.bincount(np.repeat(np.arange(k), np.diff(bp))[keep_b], minlength=k))].astype(np.int32)
    bi = bi[keep_b]
    av = rng.integers(1, 4, ai.size).astype(F)
    bv = rng.integers(1, 4, bi.size).astype(F)
    A, B = _mat(g, m, k, ap, ai, av), _mat(g, k, n, bp, bi, bv)
    Cm = g.Matrix(m, n, F)
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
    want = _fold(sr, m, n, ap, ai, av, bp, bi, bv)
    _check(Cm.host_csr(), want)
    assert want[0][1] == 0 and want[0][6] == want[0][5]              # rows 0 and 5 are empty
    # B^T (n x k) times A^T (k x m) = (A B)^T
    Ct = g.Matrix(n, m, F)
    assert g.mxm(Ct, None, None, "PlusMultiplies", B, A, _desc(hb, True, True)) == 0
    _check(Ct.host_csr(), _transpose(m, n, *want))
    # A or B without entries: C is built and empty
    E1 = _mat(g, m, k, np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, F))
    E2 = _mat(g, k, n, np.zeros(k + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, F))
    for X, Y in ((E1, B), (A, E2), (E1, E2)):
        Ce = g.Matrix(m, n, F)
        assert g.mxm(Ce, None, None, "PlusMultiplies", X, Y, hb.descriptor()) == 0
        cp, ci, cv = Ce.host_csr()
        assert np.array_equal(cp, np.zeros(m + 1, np.int32)) and ci.size == 0 and cv.size == 0
    # 1 x 1
    one = _mat(g, 1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3], F))
    two = _mat(g, 1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([5], F))
    C1 = g.Matrix(1, 1, F)
    assert g.mxm(C1, None, None, "PlusMultiplies", one, two, hb.descriptor()) == 0
    cp, ci, cv = C1.host_csr()
    assert list(cp) == [0, 1] and list(ci) == [0] and list(cv) == [15.0]


def _rmat(scale, seed=2):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=True)
    ptr, ind = (x.cpu().numpy().astype(np.int32) for x in gr["csr"])
    return n, ptr, ind


def _scipy(n, p, i, v):
    import scipy.sparse as sp
    return sp.csr_matrix((v, i, p), shape=(n, n))


def test_hub_rows_rmat14_complete(hb):
    g = hb.g
    n, ptr, ind = _rmat(14)
    rng = np.random.default_rng(14)
    val = rng.integers(1, 4, ind.size).astype(F)
    A = _mat(g, n, n, ptr, ind, val)
    Cm = g.Matrix(n, n, F)
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    S = _scipy(n, ptr, ind, val)
    W = (S @ S).tocsr()
    W.sort_indices()
    cp, ci, cv = Cm.host_csr()
    assert np.diff(cp).max() > 4096                                  # rows over more than one window of the wide kernel
    assert np.array_equal(cp, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(cv, W.data)


def test_hub_rows_rmat16_sampled(hb):
    g = hb.g
    n, ptr, ind = _rmat(16)
    rng = np.random.default_rng(16)
    val = rng.integers(1, 4, ind.size).astype(F)
    A = _mat(g, n, n, ptr, ind, val)
    Cm = g.Matrix(n, n, F)
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    cp, ci, cv = Cm.host_csr()
    S = _scipy(n, ptr, ind, val)
    # the row pointers complete: the structure of A.A row by row (the pattern's product in float64: no sum is 0, and
    # scipy drops the entries that sum to 0)
    Sb = _scipy(n, ptr, ind, np.ones(ind.size, np.float64))
    rowlen = np.diff((Sb @ Sb).tocsr().indptr)
    assert np.array_equal(np.diff(cp), rowlen) and cp[-1] == rowlen.sum()
    longest = np.argsort(-rowlen, kind="stable")[:50]
    rows = np.unique(np.r_[longest, rng.choice(n, 1950, replace=False)])
    W = (S[rows] @ S).tocsr()
    W.sort_indices()
    for t, r in enumerate(rows):
        got_i, got_v = ci[cp[r]:cp[r + 1]], cv[cp[r]:cp[r + 1]]
        want_i, want_v = W.indices[W.indptr[t]:W.indptr[t + 1]], W.data[W.indptr[t]:W.indptr[t + 1]]
        assert np.array_equal(got_i, want_i) and np.array_equal(got_v, want_v), int(r)


def test_random_real_values_and_determinism(hb):
    g = hb.g
    n, ptr, ind = _rmat(14)
    rng = np.random.default_rng(41)
    val = rng.random(ind.size).astype(F)
    A = _mat(g, n, n, ptr, ind, val)
    C1, C2 = g.Matrix(n, n, F), g.Matrix(n, n, F)
    assert g.mxm(C1, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    assert g.mxm(C2, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    p1, i1, v1 = C1.host_csr()
    p2, i2, v2 = C2.host_csr()
    assert np.array_equal(p1, p2) and np.array_equal(i1, i2) and np.array_equal(v1.view(np.uint32), v2.view(np.uint32))
    S = _scipy(n, ptr, ind, val.astype(np.float64))
    W = (S @ S).tocsr()
    W.sort_indices()
    assert np.array_equal(p1, W.indptr) and np.array_equal(i1, W.indices)
    assert np.allclose(v1, W.data, rtol=1e-5, atol=0)


def test_chaining_and_reuse(hb):
    from oracle import ops as oops
    from oracle.semiring import Semiring
    g = hb.g
    rng = np.random.default_rng(8)
    n = 400
    sr = Semiring("PlusMultiplies", F)
    ap, ai = _rand_csr(rng, n, n, 3000)
    av = rng.integers(1, 3, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    Cm = g.Matrix(n, n, F)
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    cw = _fold(sr, n, n, ap, ai, av, ap, ai, av)
    _check(Cm.host_csr(), cw)
    # D = C . A (C as the left operand of another unmasked product)
    Dm = g.Matrix(n, n, F)
    assert g.mxm(Dm, None, None, "PlusMultiplies", Cm, A, hb.descriptor()) == 0
    _check(Dm.host_csr(), _fold(sr, n, n, *cw, ap, ai, av))
    # a masked product with C as A: C<A> = C . A
    Mm = g.Matrix(n, n, F)
    assert g.mxm(Mm, A, None, "PlusMultiplies", Cm, A, hb.descriptor()) == 0
    Co, Ao = oops.Matrix(n, n, F), oops.Matrix(n, n, F)
    Co.build_csr(*cw); Ao.build_csr(ap, ai, av)
    do = oops.Descriptor(); do.loadArgs()
    mp, mi, mv = Mm.host_csr()
    assert np.array_equal(mp, ap) and np.array_equal(mi, ai)
    assert np.array_equal(mv, oops.mxm_masked(Ao, sr, Co, Ao, do))
    # mxv on C
    u = rng.integers(0, 4, n).astype(F)
    uv, w = g.Vector(n, F), g.Vector(n, F)
    assert uv.build(u, n) == 0
    assert g.mxv(w, None, None, "PlusMultiplies", Cm, uv, hb.descriptor(mxvmode=2)) == 0
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(cw[0])), cw[1]] = cw[2]
    assert np.array_equal(hb.dense_values(w).astype(np.float64), dense @ u.astype(np.float64))
    # C overwritten by a product of the same shape, then by one of another shape
    bp, bi = _rand_csr(rng, n, n, 2000)
    bv = rng.integers(1, 3, bi.size).astype(F)
    B = _mat(g, n, n, bp, bi, bv)
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
    _check(Cm.host_csr(), _fold(sr, n, n, ap, ai, av, bp, bi, bv))
    m2, k2 = 50, 90
    xp, xi = _rand_csr(rng, m2, k2, 300)
    yp, yi = _rand_csr(rng, k2, n, 700)
    xv, yv = rng.integers(1, 3, xi.size).astype(F), rng.integers(1, 3, yi.size).astype(F)
    Co2 = g.Matrix(m2, n, F)
    assert g.mxm(Co2, None, None, "PlusMultiplies", A, B, hb.descriptor()) == g.GrB_DIMENSION_MISMATCH
    assert g.mxm(Co2, None, None, "PlusMultiplies", _mat(g, m2, k2, xp, xi, xv), _mat(g, k2, n, yp, yi, yv), hb.descriptor()) == 0
    _check(Co2.host_csr(), _fold(sr, m2, n, xp, xi, xv, yp, yi, yv))
    # ... and the earlier result object reused for that shape's output once more, after a product of the first shape
    assert g.mxm(Co2, None, None, "PlusMultiplies", _mat(g, m2, k2, xp, xi, xv), _mat(g, k2, n, yp, yi, yv), hb.descriptor()) == 0
    _check(Co2.host_csr(), _fold(sr, m2, n, xp, xi, xv, yp, yi, yv))


def test_errors_leave_c_unchanged(hb):
    g = hb.g
    rng = np.random.default_rng(4)
    n = 200
    ap, ai = _rand_csr(rng, n, n, 1500)
    av = rng.integers(1, 3, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    Cm = g.Matrix(n, n, F)
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    before = [x.copy() for x in Cm.host_csr()]

    def unchanged():
        after = Cm.host_csr()
        return all(np.array_equal(x, y) for x, y in zip(before, after))

    Ai = g.Matrix(n, n, np.int32)
    assert Ai.build_csr(ap, ai, av.astype(np.int32)) == 0
    Ci = g.Matrix(n, n, np.int32)
    assert g.mxm(Ci, None, None, "PlusMultiplies", Ai, Ai, hb.descriptor()) == g.GrB_NOT_IMPLEMENTED
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, Ai, hb.descriptor()) == g.GrB_NOT_IMPLEMENTED      # mixed types
    assert unchanged()
    assert g.mxm(A, None, None, "PlusMultiplies", A, A, hb.descriptor()) == g.GrB_NOT_IMPLEMENTED       # C == A
    rp, ri = _rand_csr(rng, 7, n, 100)
    R = _mat(g, 7, n, rp, ri, np.ones(ri.size, F))
    assert g.mxm(Cm, None, None, "PlusMultiplies", A, R, hb.descriptor()) == g.GrB_DIMENSION_MISMATCH
    assert unchanged()
    # A^T of a product result (CSR only, no CSC)
    Dm = g.Matrix(n, n, F)
    assert g.mxm(Dm, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    assert g.mxm(Cm, None, None, "PlusMultiplies", Dm, A, _desc(hb, True, False)) == g.GrB_INVALID_OBJECT
    assert unchanged()
    # more than INT32_MAX outputs: a column of ones times its transpose (2.5e9, then 4.9e9 -- over 2^32)
    for big in (50000, 70000):
        col = _mat(g, big, 1, np.arange(big + 1, dtype=np.int32), np.zeros(big, np.int32), np.ones(big, F))
        row = _mat(g, 1, big, np.array([0, big], np.int32), np.arange(big, dtype=np.int32), np.ones(big, F))
        Cb = g.Matrix(big, big, F)
        assert g.mxm(Cb, None, None, "PlusMultiplies", col, row, hb.descriptor()) == g.GrB_OUT_OF_MEMORY
        # a small product in that object first: it must survive the refused one
        assert g.mxm(Cb, None, None, "PlusMultiplies", col, _mat(g, 1, big, np.array([0, 1], np.int32),
                                                                   np.array([3], np.int32), np.array([2], F)),
                     hb.descriptor()) == 0
        kept = [x.copy() for x in Cb.host_csr()]
        assert kept[0][-1] == big and np.all(kept[1] == 3) and np.all(kept[2] == 2)
        assert g.mxm(Cb, None, None, "PlusMultiplies", col, row, hb.descriptor()) == g.GrB_OUT_OF_MEMORY
        assert all(np.array_equal(x, y) for x, y in zip(kept, Cb.host_csr()))
    assert unchanged()


def test_cpp_frontend(tmp_path):
    import scipy.sparse as sp
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "spgemm_unmasked")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "spgemm_unmasked.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    mtx = os.path.join(root, "tests", "golden", "data", "chesapeake.mtx")
    lines = [ln for ln in subprocess.check_output([exe, mtx]).decode().split("\n") if ln.startswith("csr ")]
    assert len(lines) == 2, lines

    def parse(ln):
        t = ln.split("|")
        head = [int(x) for x in t[0].split()[1:]]
        return head, [np.array(x.split(), dtype=dt) for x, dt in zip(t[1:], (np.int32, np.int32, np.float32))]

    (nr, nc, av_n), (ap, ai, av) = parse(lines[0])
    (cr, cc, cv_n), (cp, ci, cv) = parse(lines[1])
    assert (cr, cc) == (nr, nc) and av_n == ai.size and cv_n == ci.size and ap.size == nr + 1 and cp.size == nr + 1
    S = sp.csr_matrix((av, ai, ap), shape=(nr, nc))
    W = (S @ S).tocsr()
    W.sort_indices()
    assert ai.size > 0 and W.nnz == cv_n
    assert np.array_equal(cp, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(cv, W.data)
