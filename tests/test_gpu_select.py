"""select on the device (csrc/select.hip): C = select(op(A), f, thunk) and w = select(u, f, thunk) against a numpy
restatement of GraphBLAS's definition -- every operator, both element types and both reads of A, entry counts around every
power-of-two tile boundary, hub rows and runs of empty rows, keep-all and keep-none, NaN / inf / -0.0 / denormals, the host
tril and the triangle count on RMAT-16, dropping the zeros of an eWiseAdd, a CSR-only input, aliasing, the vector form,
every error code with the output unchanged, determinism and the C++ frontend.  Nothing is computed, only copied: every
comparison is bit-exact."""
import os
import subprocess

import numpy as np
import pytest

from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
POSITIONAL = ["tril", "triu", "diag", "offdiag", "rowle", "rowgt", "colle", "colgt"]
VALUE = ["valueeq", "valuene", "valuelt", "valuele", "valuegt", "valuege"]


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


def _rand_csr(rng, m, n, nnz):
    """m x n, sorted rows, no duplicates, exactly nnz entries"""
    key = np.sort(rng.choice(m * n, nnz, replace=False).astype(np.int64))
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
    return rng.integers(0, 5, size).astype(dt)           # a fifth of the stored values are zeros


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


def _pred(op, i, j, a, k):
    """the table of the issue: i, j int64, a in its element type, k the thunk"""
    if op in POSITIONAL:
        k = int(k)
        return {"tril": j <= i + k, "triu": j >= i + k, "diag": j == i + k, "offdiag": j != i + k,
                "rowle": i <= k, "rowgt": i > k, "colle": j <= k, "colgt": j > k}[op]
    t = a.dtype.type(k)
    with np.errstate(invalid="ignore"):
        return {"valueeq": a == t, "valuene": a != t, "valuelt": a < t, "valuele": a <= t, "valuegt": a > t,
                "valuege": a >= t}[op]


def _expect(m, p, i, v, op, k):
    rows = np.repeat(np.arange(m, dtype=np.int64), np.diff(p))
    keep = _pred(op, rows, i.astype(np.int64), v, k)
    cp = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=m), out=cp[1:])
    return cp, i[keep], v[keep]


def _same(got, want, name=""):
    for x, y in zip(got, want):
        assert x.shape == y.shape, (name, x.shape, y.shape)
        assert np.array_equal(x.view(np.uint32) if x.dtype != np.int32 else x, y.view(np.uint32) if y.dtype != np.int32 else y), name


def _check_csc(C, m, n, name=""):
    """C's CSC holds the same entries and bits as the transpose of its CSR"""
    p, i, v = C.host_csr()
    _same(C.host_csc(), _transpose(m, n, p, i, v), name)


def _check(hb, A, m, n, p, i, v, op, k, tran=False, name=""):
    """select of op(A) = the m x n (p, i, v): the definition's CSR, and the exact transpose of it as the CSC"""
    g = hb.g
    Cm = g.Matrix(m, n, v.dtype)
    assert g.select(Cm, None, None, op, A, k, _desc(hb, tran)) == 0, (name, op, k)
    want = _expect(m, p, i, v, op, k)
    _same(Cm.host_csr(), want, (name, op, k))
    assert Cm.nvals() == want[1].size
    _check_csc(Cm, m, n, (name, op, k))
    return Cm


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("tran", [False, True])
def test_every_operator(hb, dt, tran):
    """14 operators, f32 and i32, INP0 default and TRAN, on a rectangular 37 x 53 matrix of 400 entries, a fifth of them
    stored zeros; positional thunks -3, 0, 2 and 2^40 (everything passes TRIL, nothing TRIU), value thunks 0 and 2"""
    rng = np.random.default_rng(51)
    m, n = 37, 53
    p, i = _rand_csr(rng, m, n, 400)
    v = _vals(rng, i.size, dt)
    assert (v == 0).any()
    A = _stored(hb.g, m, n, p, i, v, tran)
    for op in POSITIONAL:
        for k in (-3, 0, 2, 2 ** 40):
            Cm = _check(hb, A, m, n, p, i, v, op, k, tran)
            if k == 2 ** 40 and op in ("tril", "triu"):
                assert Cm.nvals() == (i.size if op == "tril" else 0)
    for op in VALUE:
        for k in (0, 2):
            _check(hb, A, m, n, p, i, v, op, k, tran)


def test_tile_edges(hb):
    """300 rows with 0, 1 and 2^k - 1, 2^k, 2^k + 1 entries for k = 8 .. 14: every boundary of a power-of-two tile up to
    16384 entries (the kernel's steps of 64, waves of 512 and tiles of 2048 among them)"""
    rng = np.random.default_rng(52)
    m, n = 300, 200
    for nnz in [0, 1] + [2 ** k + d for k in range(8, 15) for d in (-1, 0, 1)]:
        p, i = _rand_csr(rng, m, n, nnz)
        v = _vals(rng, nnz, F)
        A = _mat(hb.g, m, n, p, i, v)
        _check(hb, A, m, n, p, i, v, "valuene", 0, name=nnz)
        _check(hb, A, m, n, p, i, v, "tril", 0, name=nnz)


def test_row_shapes(hb):
    """one matrix with rows of 0, 1, 63, 64, 65 and 70000 entries and 5000 consecutive empty rows at the start, in the middle
    and at the end; the 70000-entry row cut mid-row by TRIL and by COLLE; and the shapes 1 x n, n x 1 and 1 x 1"""
    rng = np.random.default_rng(53)
    n = 90000
    lens = [0] * 5000 + [0, 1, 63, 64, 65, 70000, 1, 0, 64] + [0] * 5000 + [65, 0, 63, 1] + [0] * 5000
    m = len(lens)
    p = np.zeros(m + 1, np.int32)
    np.cumsum(lens, out=p[1:])
    i = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens if k]).astype(np.int32)
    hub = 5005
    assert lens[hub] == 70000
    for dt in (F, I):
        v = _vals(rng, i.size, dt)
        A = _mat(hb.g, m, n, p, i, v)
        for op, k in (("tril", 40000), ("colle", 45000), ("triu", 40000), ("colgt", 45000), ("rowle", hub), ("rowgt", hub),
                      ("diag", 100), ("offdiag", 100), ("valuene", 0), ("valuelt", 2)):
            Cm = _check(hb, A, m, n, p, i, v, op, k)
            if op in ("tril", "colle"):
                kept = np.diff(Cm.host_csr()[0])[hub]
                assert 0 < kept < 70000, (op, kept)                     # cut mid-row
    # 1 x n, n x 1, 1 x 1
    rj = np.sort(rng.choice(3000, 1500, replace=False)).astype(np.int32)
    rp = np.array([0, 1500], np.int32)
    v = _vals(rng, 1500, F)
    row = _mat(hb.g, 1, 3000, rp, rj, v)
    cp, ci, cv = _transpose(1, 3000, rp, rj, v)
    col = _mat(hb.g, 3000, 1, cp, ci, cv)
    for op, k in (("tril", 1000), ("triu", -1000), ("colle", 7), ("rowgt", 7), ("valuene", 0), ("diag", 0)):
        _check(hb, row, 1, 3000, rp, rj, v, op, k, name="1 x n")
        _check(hb, col, 3000, 1, cp, ci, cv, op, -k if op in ("tril", "triu") else k, name="n x 1")
    one = _mat(hb.g, 1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3], F))
    for op, k in (("diag", 0), ("offdiag", 0), ("valueeq", 3), ("valueeq", 0), ("tril", -1)):
        _check(hb, one, 1, 1, np.array([0, 1], np.int32), np.array([0], np.int32), np.array([3], F), op, k, name="1 x 1")


def test_keep_all_and_keep_none(hb):
    """OFFDIAG on a matrix without a diagonal returns A bit for bit in both orientations; VALUEGT 1e30 an all-zero pointer
    array and nvals == 0, and that empty result is still an operand of mxv"""
    g = hb.g
    rng = np.random.default_rng(54)
    n = 500
    p, i = _rand_csr(rng, n, n, 9000)
    rows = np.repeat(np.arange(n), np.diff(p))
    keep = i != rows
    p = np.r_[0, np.cumsum(np.bincount(rows[keep], minlength=n))].astype(np.int32)
    i = i[keep]
    v = _vals(rng, i.size, F)
    A = _mat(g, n, n, p, i, v)
    Cm = g.Matrix(n, n, F)
    assert g.select(Cm, None, None, "offdiag", A, 0, hb.descriptor()) == 0
    _same(Cm.host_csr(), (p, i, v))
    _same(Cm.host_csc(), A.host_csc())
    E = g.Matrix(n, n, F)
    assert g.select(E, None, None, "valuegt", A, 1e30, hb.descriptor()) == 0
    assert E.nvals() == 0
    ep, ei, ev = E.host_csr()
    assert np.array_equal(ep, np.zeros(n + 1, np.int32)) and ei.size == 0 and ev.size == 0
    assert np.array_equal(E.host_csc()[0], np.zeros(n + 1, np.int32))
    for mode in (1, 2):
        u, w = g.Vector(n, F), g.Vector(n, F)
        assert u.build(np.ones(n, F), n) == 0
        assert g.mxv(w, None, None, "PlusMultiplies", E, u, hb.descriptor(mxvmode=mode)) == 0
        assert not hb.dense_values(w).any(), mode


def test_value_corner_cases(hb):
    """f32: stored NaN, +-inf, -0.0 and denormals against VALUEEQ / NE / LT / GE with thunk 0 (NaN passes only VALUENE,
    -0.0 == 0.0); i32: the thunks INT32_MIN and INT32_MAX"""
    rng = np.random.default_rng(55)
    m, n = 40, 60
    p, i = _rand_csr(rng, m, n, 600)
    special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-45, 1e-39, 1.0, -1.0], F)
    v = special[rng.integers(0, special.size, 600)]
    v[:special.size] = special
    A = _mat(hb.g, m, n, p, i, v)
    for op in ("valueeq", "valuene", "valuelt", "valuege"):
        Cm = _check(hb, A, m, n, p, i, v, op, 0)
        kv = Cm.host_csr()[2]
        assert np.isnan(kv).any() == (op == "valuene")
        if op in ("valueeq", "valuege"):
            assert (kv.view(np.uint32) == 0x80000000).any()                 # -0.0 == 0.0, kept with its sign
    lim = np.array([-2 ** 31, 2 ** 31 - 1, 0, -1, 1, -2 ** 31 + 1, 2 ** 31 - 2], I)
    vi = lim[rng.integers(0, lim.size, 600)]
    Ai = _mat(hb.g, m, n, p, i, vi)
    for op in VALUE:
        for k in (-2 ** 31, 2 ** 31 - 1):
            _check(hb, Ai, m, n, p, i, vi, op, k)


@pytest.fixture(scope="module")
def rmat16(hb):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(16, 16, seed=5, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=True)
    ptr, ind = (x.cpu().numpy().astype(np.int32) for x in gr["csr"])
    return n, ptr, ind


def test_against_the_existing_paths(hb, rmat16):
    """RMAT-16: TRIL 0 has the CSR bits of grb_matrix_tril and grb_tc counts the same triangles on either; TRIL -1 and
    TRIU 1 are scipy's tril(A, -1) and triu(A, 1); the three parts add up to A"""
    import scipy.sparse as sp
    g = hb.g
    n, p, i = rmat16
    assert np.diff(p).max() > 2048                                          # a hub row over several tiles
    v = np.ones(i.size, I)
    A = _mat(g, n, n, p, i, v)
    L0, L1 = g.Matrix(n, n, I), g.Matrix(n, n, I)
    assert g.tril(L0, A, hb.descriptor()) == 0
    assert g.select(L1, None, None, "tril", A, 0, hb.descriptor()) == 0
    _same(L1.host_csr(), L0.host_csr())
    _check_csc(L1, n, n)
    counts = []
    for L in (L0, L1):
        info, ntri, _ = g.tc(L, g.Matrix(n, n, I), hb.descriptor())
        assert info == 0
        counts.append(ntri)
    assert counts[0] == counts[1] and counts[0] > 0
    S = sp.csr_matrix((np.arange(1, i.size + 1, dtype=np.float64), i, p), shape=(n, n))
    vf = np.arange(1, i.size + 1).astype(F)
    Af = _mat(g, n, n, p, i, vf)
    nv = {}
    for op, k, W in (("tril", -1, sp.tril(S, -1)), ("triu", 1, sp.triu(S, 1)), ("diag", 0, None)):
        Cm = g.Matrix(n, n, F)
        assert g.select(Cm, None, None, op, Af, k, hb.descriptor()) == 0
        nv[op] = Cm.nvals()
        if W is not None:
            W = W.tocsr()
            W.sort_indices()
            _same(Cm.host_csr(), (W.indptr.astype(I), W.indices.astype(I), W.data.astype(F)), op)
            _check_csc(Cm, n, n, op)
    assert nv["tril"] + nv["diag"] + nv["triu"] == i.size


def test_dropping_zeros_in_a_chain(hb):
    """eWiseAdd(A, -A) under Plus stores only zeros and VALUENE 0 of it is empty; VALUENE 0 of A + B keeps exactly the
    structure scipy's eliminate_zeros leaves"""
    import scipy.sparse as sp
    g = hb.g
    rng = np.random.default_rng(57)
    m, n = 180, 160
    (ap, ai), (bp, bi) = _rand_csr(rng, m, n, 6000), _rand_csr(rng, m, n, 6000)
    av, bv = rng.integers(-2, 3, ai.size).astype(F), rng.integers(-2, 3, bi.size).astype(F)
    A, B, N = _mat(g, m, n, ap, ai, av), _mat(g, m, n, bp, bi, bv), _mat(g, m, n, ap, ai, av)
    assert g.apply(N, None, None, "ainv", N, hb.descriptor()) == 0
    Z = g.Matrix(m, n, F)
    assert g.eWiseAdd(Z, None, None, "PlusMultiplies", A, N, hb.descriptor()) == 0
    assert Z.nvals() == ai.size and not Z.host_csr()[2].any()
    assert g.select(Z, None, None, "valuene", Z, 0, hb.descriptor()) == 0
    assert Z.nvals() == 0 and not Z.host_csr()[0].any()
    E = g.Matrix(m, n, F)
    assert g.eWiseAdd(E, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0
    before = E.nvals()
    assert g.select(E, None, None, "valuene", E, 0, hb.descriptor()) == 0
    W = (sp.csr_matrix((av, ai, ap), shape=(m, n)) + sp.csr_matrix((bv, bi, bp), shape=(m, n))).tocsr()
    W.eliminate_zeros()
    W.sort_indices()
    assert E.nvals() == W.nnz < before
    _same(E.host_csr(), (W.indptr.astype(I), W.indices.astype(I), W.data.astype(F)))
    _check_csc(E, m, n)


def test_csr_only_input(hb):
    """a product result has no CSC: its select is CSR only, its transposed select GrB_INVALID_OBJECT until grb_transpose
    under INP0 = TRAN has given it both orientations"""
    g = hb.g
    rng = np.random.default_rng(58)
    n = 200
    ap, ai = _rand_csr(rng, n, n, 1500)
    av = rng.integers(1, 3, ai.size).astype(F)
    A = _mat(g, n, n, ap, ai, av)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, A, hb.descriptor()) == 0
    pp, pi, pv = (x.copy() for x in P.host_csr())
    Cm = g.Matrix(n, n, F)
    assert g.select(Cm, None, None, "triu", P, 1, hb.descriptor()) == 0
    _same(Cm.host_csr(), _expect(n, pp, pi, pv, "triu", 1))
    with pytest.raises(g._lib.GrbError) as e:
        Cm.host_csc()
    assert e.value.info == g.GrB_NO_VALUE
    kept = [x.copy() for x in Cm.host_csr()]
    assert g.select(Cm, None, None, "triu", P, 1, _desc(hb, True)) == g.GrB_INVALID_OBJECT
    _same(Cm.host_csr(), kept)
    Q = g.Matrix(n, n, F)
    assert g.transpose(Q, None, None, P, _desc(hb, True)) == 0
    tp, ti, tv = _transpose(n, n, pp, pi, pv)
    for op, k in (("triu", 1), ("valuegt", 2), ("rowle", 50)):
        _check(hb, Q, n, n, tp, ti, tv, op, k, tran=True)


def test_aliasing(hb):
    """C is A; w is u, sparse and dense"""
    g = hb.g
    rng = np.random.default_rng(59)
    n = 140
    p, i = _rand_csr(rng, n, n, 3000)
    v = _vals(rng, i.size, F)
    for op, k in (("tril", -1), ("valuene", 0)):
        A = _mat(g, n, n, p, i, v)
        assert g.select(A, None, None, op, A, k, hb.descriptor()) == 0
        _same(A.host_csr(), _expect(n, p, i, v, op, k), op)
        _check_csc(A, n, n, op)
    vals = rng.integers(0, 9, n).astype(F)
    u = g.Vector(n, F)
    assert u.build(vals, n) == 0
    assert g.select(u, None, None, "valuegt", u, 4, hb.descriptor()) == 0
    keep = np.nonzero(vals > 4)[0]
    assert u.getStorage() == g.GrB_SPARSE and u.nvals() == keep.size
    gi, gv = hb.sparse_tuples(u)
    assert np.array_equal(gi, keep) and np.array_equal(gv, vals[keep])
    si = np.sort(rng.choice(n, 50, replace=False)).astype(np.int32)
    sv = rng.integers(0, 9, 50).astype(F)
    s = g.Vector(n, F)
    assert s.build(si, sv, 50, None) == 0
    assert g.select(s, None, None, "rowgt", s, 70, hb.descriptor()) == 0
    assert s.getStorage() == g.GrB_SPARSE and s.nvals() == int((si > 70).sum())
    gi, gv = hb.sparse_tuples(s)
    assert np.array_equal(gi, si[si > 70]) and np.array_equal(gv, sv[si > 70])


@pytest.mark.parametrize("dt", [F, I])
def test_vector_form(hb, dt):
    """sizes 1, 63, 64, 65 and 100003, a sparse u (a third stored) and a dense one; ROWLE, ROWGT, TRIL with j = 0 and the
    six value operators; w sparse, indices ascending, the right nvals"""
    g = hb.g
    rng = np.random.default_rng(60)
    for n in (1, 63, 64, 65, 100003):
        k3 = max(n // 3, 1)
        si = np.sort(rng.choice(n, k3, replace=False)).astype(np.int32)
        sv = _vals(rng, k3, dt)
        dv = _vals(rng, n, dt)
        for sparse in (True, False):
            idx, val = (si, sv) if sparse else (np.arange(n, dtype=np.int32), dv)
            u = g.Vector(n, dt)
            assert (u.build(si, sv, k3, None) if sparse else u.build(dv, n)) == 0
            for op, k in [("rowle", n // 2), ("rowgt", n // 2), ("tril", -(n // 4)), ("tril", 0), ("triu", 0), ("colle", -1)] + \
                         [(op, 2) for op in VALUE]:
                w = g.Vector(n, dt)
                assert g.select(w, None, None, op, u, k, hb.descriptor()) == 0, (n, sparse, op)
                keep = _pred(op, idx.astype(np.int64), np.zeros(idx.size, np.int64), val, k)
                assert w.getStorage() == g.GrB_SPARSE and w.nvals() == int(keep.sum()), (n, sparse, op)
                gi, gv = hb.sparse_tuples(w)
                assert np.array_equal(gi, idx[keep]) and np.array_equal(gv, val[keep]), (n, sparse, op)
                assert (np.diff(gi) > 0).all()
            assert u.getStorage() == (g.GrB_SPARSE if sparse else g.GrB_DENSE)      # the input is left alone


def test_errors_leave_the_output_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(61)
    m, n = 100, 80
    p, i = _rand_csr(rng, m, n, 1500)
    v = _vals(rng, i.size, F)
    A = _mat(g, m, n, p, i, v)
    Ai = _mat(g, m, n, p, i, v.astype(I))
    d = hb.descriptor()
    Cm, Ci = g.Matrix(m, n, F), g.Matrix(m, n, I)
    assert g.select(Cm, None, None, "triu", A, 0, d) == 0
    assert g.select(Ci, None, None, "triu", Ai, 0, d) == 0
    before = {id(X): [x.copy() for x in X.host_csr()] + [x.copy() for x in X.host_csc()] for X in (Cm, Ci)}

    def unchanged(X):
        return all(np.array_equal(x, y) for x, y in zip(before[id(X)], list(X.host_csr()) + list(X.host_csc())))

    call = lambda C_, A_, op, k, mask=None: lib.grb_matrix_select(C_, mask, 0, op, float(k), A_, d._h)
    assert call(None, A._h, 0, 0) == g.GrB_UNINITIALIZED_OBJECT                                # null handles
    assert call(Cm._h, None, 0, 0) == g.GrB_UNINITIALIZED_OBJECT
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Cm, None, None, "tril", g.Matrix(m, n, F), 0, d) == g.GrB_UNINITIALIZED_OBJECT   # an unbuilt A
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(g.Matrix(m, n + 1, F), None, None, "tril", A, 0, d) == g.GrB_DIMENSION_MISMATCH
    assert g.select(Cm, None, None, "tril", A, 0, _desc(hb, True)) == g.GrB_DIMENSION_MISMATCH  # op(A) is 80 x 100
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Cm, None, None, "tril", Ai, 0, d) == g.GrB_NOT_IMPLEMENTED                  # f32 / i32
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Ci, None, None, "tril", A, 0, d) == g.GrB_NOT_IMPLEMENTED
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Cm, A, None, "tril", A, 0, d) == g.GrB_NOT_IMPLEMENTED                      # a mask
    assert unchanged(Cm) and unchanged(Ci)
    assert call(Cm._h, A._h, -1, 0) == g.GrB_INVALID_VALUE                                     # outside the enum
    assert unchanged(Cm) and unchanged(Ci)
    assert call(Cm._h, A._h, 14, 0) == g.GrB_INVALID_VALUE
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Cm, None, None, "tril", A, 0.5, d) == g.GrB_INVALID_VALUE                   # a positional thunk is an integer
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Cm, None, None, "rowle", A, float("nan"), d) == g.GrB_INVALID_VALUE
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Ci, None, None, "valuege", Ai, 0.5, d) == g.GrB_INVALID_VALUE               # ... and an i32 value thunk
    assert unchanged(Cm) and unchanged(Ci)
    assert g.select(Ci, None, None, "valuege", Ai, 3e9, d) == g.GrB_INVALID_VALUE
    assert unchanged(Cm) and unchanged(Ci)              # (neither is written to again below)
    Cf = g.Matrix(m, n, F)
    assert g.select(Cf, None, None, "valuege", A, 0.5, d) == 0                                  # (f32 takes any thunk)
    _same(Cf.host_csr(), _expect(m, p, i, v, "valuege", 0.5))
    P, Ct = g.Matrix(m, m, F), g.Matrix(m, m, F)
    assert g.mxm(P, None, None, "PlusMultiplies", A, _mat(g, n, m, *_transpose(m, n, p, i, v)), d) == 0
    assert g.select(Ct, None, None, "tril", P, 0, d) == 0
    kept = [x.copy() for x in Ct.host_csr()]
    assert g.select(Ct, None, None, "tril", P, 0, _desc(hb, True)) == g.GrB_INVALID_OBJECT      # TRAN on a CSR-only A
    _same(Ct.host_csr(), kept)
    assert unchanged(Cm) and unchanged(Ci)
    # a null descriptor means the defaults
    Cn = g.Matrix(m, n, F)
    assert g.select(Cn, None, None, "triu", A, 0, None) == 0
    _same(Cn.host_csr(), before[id(Cm)][:3])

    # the vector form
    u = g.Vector(m, F)
    assert u.build(np.arange(m, dtype=F), m) == 0
    w = g.Vector(m, F)
    assert g.select(w, None, None, "rowgt", u, 10, d) == 0
    kept = [x.copy() for x in hb.sparse_tuples(w)]
    vcall = lambda w_, u_, op, k, mask=None: lib.grb_vector_select(w_, mask, 0, op, float(k), u_, d._h)
    assert vcall(None, u._h, 0, 0) == g.GrB_UNINITIALIZED_OBJECT
    assert vcall(w._h, None, 0, 0) == g.GrB_UNINITIALIZED_OBJECT
    assert g.select(w, None, None, "rowle", g.Vector(m, F), 0, d) == g.GrB_UNINITIALIZED_OBJECT  # no storage yet
    assert g.select(w, w, None, "rowle", u, 0, d) == g.GrB_NOT_IMPLEMENTED
    assert g.select(g.Vector(m, I), None, None, "rowle", u, 0, d) == g.GrB_DOMAIN_MISMATCH
    assert g.select(g.Vector(m + 1, F), None, None, "rowle", u, 0, d) == g.GrB_DIMENSION_MISMATCH
    assert vcall(w._h, u._h, -1, 0) == g.GrB_INVALID_VALUE and vcall(w._h, u._h, 14, 0) == g.GrB_INVALID_VALUE
    assert g.select(w, None, None, "rowle", u, 0.5, d) == g.GrB_INVALID_VALUE
    ui = g.Vector(m, I)
    assert ui.build(np.arange(m, dtype=I), m) == 0
    wi = g.Vector(m, I)
    assert g.select(wi, None, None, "valuelt", ui, 0.5, d) == g.GrB_INVALID_VALUE
    assert g.select(wi, None, None, "valuelt", ui, -3e9, d) == g.GrB_INVALID_VALUE
    assert w.getStorage() == g.GrB_SPARSE and all(np.array_equal(x, y) for x, y in zip(kept, hb.sparse_tuples(w)))


def test_determinism(hb, rmat16):
    """RMAT-16, VALUELT at the median weight: two calls, the same bits in both orientations"""
    g = hb.g
    n, p, i = rmat16
    rng = np.random.default_rng(62)
    v = rng.integers(1, 65, i.size).astype(F)
    A = _mat(g, n, n, p, i, v)
    k = float(np.median(v))
    outs = []
    for _ in range(2):
        Cm = g.Matrix(n, n, F)
        assert g.select(Cm, None, None, "valuelt", A, k, hb.descriptor()) == 0
        outs.append([x.copy() for x in Cm.host_csr()] + [x.copy() for x in Cm.host_csc()])
    _same(outs[0], outs[1])
    _same(outs[0][:3], _expect(n, p, i, v, "valuelt", k))
    _same(outs[0][3:], _transpose(n, n, *outs[0][:3]))


def test_cpp_frontend(tmp_path):
    """tests/tools/select.cpp: both overloads on a 4 x 4 literal"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "select")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "tests", "tools", "select.cpp"),
                           "-L" + os.path.join(root, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(root, "graphblast_amd"), "-o", exe])
    lines = [ln.strip() for ln in subprocess.check_output([exe]).decode().split("\n") if ln.split(" ")[0] in ("tril", "trilT", "nz", "vgt", "vrow")]
    # A = [[1 . 2 .] [. 3 . .] [4 . 5 6] [. 0 . 7]]
    assert lines == ["tril 4 4 2 | 0 0 0 1 2 | 0 1 | 4 0",          # strictly lower: (2, 0) = 4 and the stored zero at (3, 1)
                     "trilT 4 4 2 | 0 1 2 2 2 | 2 3 | 4 0",
                     "nz 4 4 7 | 0 2 3 6 7 | 0 2 1 0 2 3 3 | 1 2 3 4 5 6 7",
                     "vgt 2 | 2 3 | 12 13",
                     "vrow 1 | 2 | 12"], lines
