"""Graph contraction on the device (csrc/contract.hip: grb_relabel, grb_contract) against numpy: np.unique(...,
return_inverse) for relabel; for contract a np.lexsort on (position, b, a) of the surviving entries and reduceat over the
runs -- PLUS in int64 wrapped to int32, or in float64 rounded once.  Everything is compared EXACTLY: pointers, indices, value
BITS, both orientations, sizes and every exact field of the record.  The single exception is f32 PLUS on inputs whose f64
sum is not exact in every order: there, with k contributions w to an entry and S = math.fsum(w), |got - S| <= E +
2^-24 (|S| + E) with E = k 2^-53 sum |w| -- an f64 sum in any order plus one rounding to f32; derived, not tuned, and the
observed difference is printed.  Every other f32 PLUS case uses integer-valued weights below 2^24.  A PLUS entry whose exact
value is a NaN (+inf and -inf met) is compared as a NaN: IEEE 754 does not fix the sign of a generated NaN."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

from backends import HipBackend
from test_gpu_msf import Graph, _bits, _grid_edges, _matrix, _random_edges

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
LANE_RUN = 32      # kCtLaneRun: a run (the contributions to one C(a, b)) of up to this many is folded by one lane, in order
PIECE = 2048       # kCtPiece: a longer run is cut into pieces of this many, a wave each; the pieces' results by one wave
WAVE = 64          # lanes that interleave inside a piece and over the pieces
OPS = ("plus", "minimum", "maximum", "first")
REC = ("kept", "loops", "entries", "clusters", "dropped", "largest")
LABELS, MATE = 0, 1


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- the reference -----------------------------------------------------------------------------------------------------
def _order_key(w):
    """the monotone map of the bits: i32 as signed integers; f32 -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN"""
    b = _bits(w).astype(np.uint32)
    if w.dtype == I:
        return b ^ np.uint32(0x80000000)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def _ref_relabel(labels, kind):
    n = labels.size
    v = np.arange(n)
    L = labels.astype(np.int64) if kind == LABELS else np.where(labels < 0, v, np.minimum(v, labels))
    uniq, inv = np.unique(L, return_inverse=True)
    return inv.reshape(-1).astype(I), int(uniq.size)


def _ref(ptr, ind, val, mp, nc, op, loops):
    """-> (CSR), (CSC), sizes, the record, (the runs' starts, the sorted values): C = S^T A S"""
    n = ptr.size - 1
    mp = np.asarray(mp, np.int64)
    rows = np.repeat(np.arange(n), np.diff(ptr))
    a, b = mp[rows], mp[ind]
    kept = (a >= 0) & (b >= 0)
    loop = kept & (a == b)
    pos = np.flatnonzero(kept if loops else kept & ~loop)
    a, b, w = a[pos], b[pos], val[pos]
    o = np.lexsort((pos, b, a))
    a, b, w = a[o], b[o], w[o]
    head = np.ones(pos.size, bool)
    head[1:] = (a[1:] != a[:-1]) | (b[1:] != b[:-1])
    starts = np.flatnonzero(head)
    ca, cb = a[starts], b[starts]
    if starts.size == 0:
        cv = np.zeros(0, val.dtype)
    elif op == "first":
        cv = w[starts]
    elif op == "plus" and val.dtype == I:
        cv = (np.add.reduceat(w.astype(np.int64), starts) & 0xffffffff).astype(np.uint32).view(I)
    elif op == "plus":
        with np.errstate(all="ignore"):
            cv = np.add.reduceat(w.astype(np.float64), starts).astype(F)
    else:
        key = _order_key(w)
        best = (np.minimum if op == "minimum" else np.maximum).reduceat(key, starts)
        if val.dtype == I:
            cv = (best ^ np.uint32(0x80000000)).view(I)
        else:
            cv = np.where(best & np.uint32(0x80000000), best & np.uint32(0x7fffffff), ~best).astype(np.uint32).view(F)
    rp = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(ca, minlength=nc), out=rp[1:])
    t = np.lexsort((ca, cb))
    cp = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(cb, minlength=nc), out=cp[1:])
    sizes = np.bincount(mp[mp >= 0], minlength=nc).astype(I)
    rec = dict(kept=int(kept.sum()), loops=int(loop.sum()), entries=int(starts.size), clusters=int((sizes > 0).sum()),
               dropped=int((mp < 0).sum()), largest=int(sizes.max()) if nc else 0)
    return (rp.astype(I), cb.astype(I), cv), (cp.astype(I), ca[t].astype(I), cv[t]), sizes, rec, (starts, w)


def _same_values(got, want, op, name):
    assert got.dtype == want.dtype and got.size == want.size, (name, got.dtype, got.size, want.size)
    if op == "plus" and want.dtype == F:
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan), (name, "NaN")
        got, want = got[~nan], want[~nan]
    bad = np.flatnonzero(_bits(got) != _bits(want))
    assert bad.size == 0, (name, "values", bad[:10], got[bad[:10]], want[bad[:10]])


def _csr_of(rng, n, m, dt, values=None):
    """a directed matrix of about m entries (duplicates merged), diagonal entries among them"""
    key = np.unique(rng.integers(0, n, m).astype(np.int64) * n + rng.integers(0, n, m))
    r, c = key // n, key % n
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    val = rng.integers(-9, 10, key.size).astype(dt) if values is None else values(key.size)
    return ptr.astype(I), c.astype(I), val


def _mat(g, ptr, ind, val, csr_only=False, monkeypatch=None):
    n = ptr.size - 1
    if csr_only:
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(n, n, val.dtype.type)
    if csr_only:
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(ptr, ind, val) == 0
    return A


def _vec(g, values):
    v = g.Vector(values.size, I)
    if values.size:
        assert v.build(np.ascontiguousarray(values, I), values.size) == 0
    return v


def _check(hb, csr, mp, nc, op, loops, A=None, Cm=None, sizes="new", mapvec=None, name="", csc=True, exact=True):
    """grb_contract against the reference, exactly; -> (C's CSR, the record, the reference's runs)"""
    g = hb.g
    ptr, ind, val = csr
    mp = np.asarray(mp, I)
    (wp, wi, wv), (tp, ti, tv), wsizes, rec, runs = _ref(ptr, ind, val, mp, nc, op, loops)
    if A is None:
        A = _mat(g, ptr, ind, val)
    if Cm is None:
        Cm = g.Matrix(nc, nc, val.dtype.type)
    if mapvec is None:
        mapvec = _vec(g, mp)
    if isinstance(sizes, str):
        sizes = g.Vector(nc, I)
    info, res = g.contract(Cm, sizes, A, mapvec, op, loops, None)
    assert info == 0, (name, info)
    print(name, {x: res[x] for x in REC}, "launches", res["launches"], "loop_ms", res["loop_ms"])
    for x in REC:
        assert res[x] == rec[x], (name, x, res, rec)
    assert res["launches"] >= 1 and res["loop_ms"] >= 0
    assert Cm.nvals() == rec["entries"]
    cp, ci, cv = Cm.host_csr()
    assert np.array_equal(cp, wp), (name, "pointers", np.flatnonzero(cp != wp)[:10])
    assert np.array_equal(ci, wi), (name, "indices", np.flatnonzero(ci != wi)[:10])
    if exact:
        _same_values(cv, wv, op, name)
    if csc:
        xp, xi, xv = Cm.host_csc()
        assert np.array_equal(xp, tp) and np.array_equal(xi, ti), (name, "the CSC")
        # the same entries and bits as the CSR, never a second fold
        t = np.lexsort((np.repeat(np.arange(nc), np.diff(cp)), ci))
        assert np.array_equal(_bits(xv), _bits(cv[t])), (name, "the CSC's values")
    if sizes is not None:
        assert sizes.getStorage() == g.GrB_DENSE and sizes.nvals() == nc
        if nc:
            assert np.array_equal(sizes.extractTuples()[1], wsizes), (name, "sizes")
    return (cp, ci, cv), res, runs


# ---- literal answers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
def test_path_of_four_in_pairs(hb, dt):
    """0 - 1 - 2 - 3 with the weights 5, 7, 11 (both directions), pairs {0, 1} and {2, 3}"""
    gr = Graph(4, [0, 1, 2], [1, 2, 3], [5, 7, 11], dt)
    csr = gr.csr()
    (cp, ci, cv), res, _ = _check(hb, csr, [0, 0, 1, 1], 2, "plus", 0, name="path")
    assert cp.tolist() == [0, 1, 2] and ci.tolist() == [1, 0] and cv.tolist() == [7, 7]
    assert (res["kept"], res["loops"], res["entries"], res["clusters"], res["dropped"], res["largest"]) == (6, 4, 2, 2, 0, 2)
    (cp, ci, cv), res, _ = _check(hb, csr, [0, 0, 1, 1], 2, "plus", 1, name="path, loops")
    assert cp.tolist() == [0, 2, 4] and ci.tolist() == [0, 1, 0, 1] and cv.tolist() == [10, 7, 7, 22]
    (_, _, cv), _, _ = _check(hb, csr, [0, 0, 1, 1], 2, "maximum", 1, name="path, max")
    assert cv.tolist() == [5, 7, 7, 11]


@pytest.mark.parametrize("dt", [F, I])
def test_triangle_into_one_vertex(hb, dt):
    gr = Graph(3, [0, 0, 1], [1, 2, 2], [1, 2, 4], dt)
    csr = gr.csr()
    (cp, ci, cv), res, _ = _check(hb, csr, [0, 0, 0], 1, "plus", 1, name="triangle, loops kept")
    assert cp.tolist() == [0, 1] and ci.tolist() == [0] and cv.tolist() == [14] and res["loops"] == 6 and res["largest"] == 3
    (cp, ci, cv), res, _ = _check(hb, csr, [0, 0, 0], 1, "plus", 0, name="triangle, loops dropped")
    assert cp.tolist() == [0, 0] and ci.size == 0 and res["entries"] == 0 and res["loops"] == 6 and res["kept"] == 6
    (_, _, cv), _, _ = _check(hb, csr, [0, 0, 0], 1, "first", 1, name="triangle, first")
    assert cv.tolist() == [1]                              # A(0, 1)
    (_, _, cv), _, _ = _check(hb, csr, [0, 0, 0], 1, "minimum", 1, name="triangle, min")
    assert cv.tolist() == [1]


# ---- identities --------------------------------------------------------------------------------------------------------
def _special_f32(rng, m):
    w = (rng.integers(-40, 40, m) / 4).astype(F)
    at = rng.choice(m, min(m, 600), replace=False)
    special = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00000, 0xffc00000, 0x7fc00001, 0xffffffff, 0x00000001,
                        0x80000001], np.uint32).view(F)
    w[at] = special[np.arange(at.size) % special.size]
    return w


@pytest.mark.parametrize("dt", [F, I])
def test_identity_map_returns_a(hb, dt):
    rng = np.random.default_rng(50)
    n = 777
    csr = _csr_of(rng, n, 6000, dt, (lambda m: _special_f32(rng, m)) if dt is F else None)
    for op in OPS:
        (cp, ci, cv), res, _ = _check(hb, csr, np.arange(n), n, op, 1, name=("identity", op))
        assert np.array_equal(cp, csr[0]) and np.array_equal(ci, csr[1]) and np.array_equal(_bits(cv), _bits(csr[2]))
        assert res["clusters"] == n and res["largest"] == 1


@pytest.mark.parametrize("dt", [F, I])
def test_permutation_returns_p_a_pt(hb, dt):
    rng = np.random.default_rng(51)
    n = 1001
    ptr, ind, val = csr = _csr_of(rng, n, 9000, dt)
    perm = rng.permutation(n)
    (cp, ci, cv), _, _ = _check(hb, csr, perm, n, "plus", 1, name="permutation")
    rows = np.repeat(np.arange(n), np.diff(ptr))
    P = sp.csr_matrix((val.astype(np.float64), (perm[rows], perm[ind])), shape=(n, n))
    P.sort_indices()
    assert np.array_equal(cp, P.indptr) and np.array_equal(ci, P.indices) and np.array_equal(cv.astype(np.float64), P.data)
    assert (np.diff(ci)[np.diff(np.repeat(np.arange(n), np.diff(cp))) == 0] > 0).all()   # columns ascend in every row


# ---- operators, special values, dropped vertices, unused ids ------------------------------------------------------------
@pytest.mark.parametrize("loops", [0, 1])
@pytest.mark.parametrize("op", OPS)
def test_every_operator_both_types(hb, op, loops):
    rng = np.random.default_rng(52)
    n, nc = 1203, 97
    mp = rng.integers(-1, 90, n)                          # some dropped, ids 90 .. 96 unused
    assert (mp == -1).any()
    for dt in (F, I):
        if dt is F and op != "plus":
            values = lambda m: _special_f32(rng, m)       # noqa: E731  -0.0 / +0.0, +-inf, both NaN signs, denormals
        elif dt is F:
            values = lambda m: rng.integers(-1000, 1000, m).astype(F)    # noqa: E731
        else:
            values = lambda m: rng.integers(-2 ** 31, 2 ** 31, m).astype(I)   # noqa: E731  PLUS wraps past INT32_MAX
        csr = _csr_of(rng, n, 20000, dt, values)
        (cp, _, cv), res, (starts, w) = _check(hb, csr, mp, nc, op, loops, name=(op, loops, dt.__name__))
        assert res["dropped"] > 0 and res["clusters"] <= 90 and (np.diff(cp)[90:] == 0).all()
        assert (np.diff(np.append(starts, w.size)) > 1).any()
        if dt is I and op == "plus":
            exact = np.add.reduceat(w.astype(np.int64), starts)
            assert (np.abs(exact) > 2 ** 31).any()


def test_f32_plus_with_infinities(hb):
    """+inf and -inf under PLUS: alone they win, together the entry is a NaN"""
    rng = np.random.default_rng(53)
    n, nc = 400, 11
    mp = rng.integers(0, nc, n)
    ptr, ind, val = _csr_of(rng, n, 9000, F, lambda m: rng.integers(-50, 50, m).astype(F))
    val[rng.choice(val.size, 12, replace=False)] = np.repeat(np.array([np.inf, -np.inf], F), 6)
    (_, _, cv), _, _ = _check(hb, (ptr, ind, val), mp, nc, "plus", 1, name="infinities")
    assert np.isposinf(cv).any() and np.isneginf(cv).any()
    gr = Graph(2, [0], [1], [np.inf], F, w_rev=[-np.inf])
    (_, _, cv), _, _ = _check(hb, gr.csr(), [0, 0], 1, "plus", 1, name="inf - inf")
    assert np.isnan(cv).all()


def test_special_values_in_one_run(hb):
    """all of -NaN, -inf, -0.0, +0.0, +inf, +NaN in one run: MIN takes -NaN's bits, MAX +NaN's, FIRST the first stored"""
    bits = np.array([0x00000000, 0x7f800000, 0x80000000, 0xffc00000, 0x3f800000, 0xff800000, 0x7fc00000], np.uint32)
    n = bits.size + 1
    ptr = np.zeros(n + 1, I)
    ptr[1:] = bits.size
    csr = (ptr, np.arange(1, n, dtype=I), bits.view(F))
    for op, want in (("minimum", 0xffc00000), ("maximum", 0x7fc00000), ("first", 0x00000000)):
        (_, _, cv), _, _ = _check(hb, csr, [0] + [1] * bits.size, 2, op, 0, name=("one run", op))
        assert _bits(cv).tolist() == [want]
    for op, want in (("minimum", 0x80000000), ("maximum", 0x00000000)):       # -0.0 < +0.0
        two = (np.array([0, 2, 2, 2], I), np.array([1, 2], I), np.array([0x00000000, 0x80000000], np.uint32).view(F))
        (_, _, cv), _, _ = _check(hb, two, [0, 1, 1], 2, op, 0, name=("zeros", op))
        assert _bits(cv).tolist() == [want]


@pytest.mark.parametrize("dt", [F, I])
def test_dropping_all_some_and_none(hb, dt):
    rng = np.random.default_rng(54)
    n, nc = 500, 40
    csr = _csr_of(rng, n, 5000, dt)
    mp = rng.integers(0, nc, n)
    _, res, _ = _check(hb, csr, mp, nc, "plus", 1, name="none dropped")
    assert res["dropped"] == 0 and res["kept"] == csr[1].size
    some = mp.copy()
    some[rng.choice(n, 200, replace=False)] = -1
    _, res, _ = _check(hb, csr, some, nc, "plus", 1, name="some dropped")
    assert res["dropped"] == 200 and 0 < res["kept"] < csr[1].size
    (cp, ci, _), res, _ = _check(hb, csr, np.full(n, -1), nc, "plus", 1, name="all dropped")
    assert res["dropped"] == n and res["kept"] == 0 and res["clusters"] == 0 and res["largest"] == 0 and ci.size == 0
    _check(hb, csr, np.full(n, -1), 0, "plus", 1, name="nc = 0", sizes=None)


def test_raw_cc_labels_with_an_n_by_n_c(hb):
    g = hb.g
    rng = np.random.default_rng(55)
    n = 900
    u, v = _random_edges(rng, n, 700)                     # many components
    gr = Graph(n, u, v, rng.integers(1, 9, u.size), I)
    A = _matrix(g, gr)
    lab = g.Vector(n, I)
    assert g.cc(lab, A, 0, hb.descriptor())[0] == 0
    labels = lab.extractTuples()[1]
    assert np.unique(labels).size > 100
    (cp, _, _), res, _ = _check(hb, gr.csr(), labels, n, "plus", 1, A=A, mapvec=lab, name="raw cc labels")
    assert res["clusters"] == np.unique(labels).size and res["entries"] <= res["clusters"]
    assert (np.diff(cp)[np.setdiff1d(np.arange(n), labels)] == 0).all()


# ---- the run-length classes --------------------------------------------------------------------------------------------
def _runs_graph(lengths, dt, rng):
    """one source vertex per length L, alone in its cluster, with L entries into the L first vertices of a shared target cluster:
    C(a, target) is a run of exactly L contributions"""
    k = len(lengths)
    width = max(lengths)
    n = k + width
    ptr = np.zeros(n + 1, np.int64)
    ptr[1:k + 1] = np.cumsum(lengths)
    ptr[k + 1:] = ptr[k]
    ind = np.concatenate([k + np.arange(L) for L in lengths])
    val = rng.integers(-100, 100, ind.size).astype(dt)
    mp = np.concatenate([np.arange(k), np.full(width, k)])
    return (ptr.astype(I), ind.astype(I), val), mp, k + 1


@pytest.mark.parametrize("dt", [F, I])
def test_every_run_class(hb, dt):
    """runs of 1, 31, 32, 33 contributions (a lane / pieces), 2 047 .. 2 049 and 4 096, 4 097 (one, two, three pieces), and
    64 and 65 pieces (the lanes of the wave that folds the pieces' results wrap round)"""
    rng = np.random.default_rng(56)
    lengths = [1, LANE_RUN - 1, LANE_RUN, LANE_RUN + 1, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE, 2 * PIECE + 1, WAVE * PIECE,
               WAVE * PIECE + 1]
    csr, mp, nc = _runs_graph(lengths, dt, rng)
    for op in OPS:
        (cp, ci, _), res, (starts, w) = _check(hb, csr, mp, nc, op, 0, name=("classes", op, dt.__name__))
        assert np.diff(np.append(starts, w.size)).tolist() == lengths and res["entries"] == len(lengths)
        assert res["largest"] == max(lengths)


def test_a_coarse_row_of_many_short_and_long_runs(hb):
    """the members of one cluster together hold runs of every class, interleaved in the CSR"""
    rng = np.random.default_rng(57)
    n, nc = 3000, 7
    mp = np.minimum(rng.integers(0, 400, n), nc - 1)     # cluster 6 is the giant, the others hold seven or eight vertices
    csr = _csr_of(rng, n, 200000, I)
    for op in OPS:
        _, res, (starts, w) = _check(hb, csr, mp, nc, op, 1, name=("mixed", op))
    lens = np.diff(np.append(starts, w.size))
    assert (lens <= LANE_RUN).any() and ((lens > LANE_RUN) & (lens <= PIECE)).any() and (lens > 2 * PIECE).any()


@pytest.mark.parametrize("dt", [F, I])
def test_everything_into_one_cluster(hb, dt):
    """n = 3 000, about 60 000 entries -> a 1 x 1 C: one run of every entry"""
    rng = np.random.default_rng(58)
    n = 3000
    csr = _csr_of(rng, n, 60500, dt)
    assert csr[1].size > 59000
    for op in OPS:
        (cp, ci, cv), res, _ = _check(hb, csr, np.zeros(n), 1, op, 1, name=("one cluster", op, dt.__name__))
        assert cp.tolist() == [0, 1] and ci.tolist() == [0] and res["loops"] == res["kept"] == csr[1].size and res["largest"] == n
    _, res, _ = _check(hb, csr, np.zeros(n), 1, "plus", 0, name="one cluster, loops dropped")
    assert res["entries"] == 0


def test_f32_plus_within_the_bound_of_an_f64_sum(hb):
    """general floats: |got - S| <= E + 2^-24 (|S| + E), E = k 2^-53 sum |w| (see the module's docstring)"""
    rng = np.random.default_rng(59)
    n, nc = 3000, 5
    mp = np.minimum(rng.integers(0, 12, n), nc - 1)
    csr = _csr_of(rng, n, 150000, F, lambda m: ((rng.random(m) - 0.3) * 10.0 ** rng.integers(-3, 4, m)).astype(F))
    (cp, ci, cv), _, (starts, w) = _check(hb, csr, mp, nc, "plus", 1, name="general floats", exact=False)
    ends = np.append(starts, w.size)
    worst = 0.0
    for r in range(starts.size):
        x = w[ends[r]:ends[r + 1]].astype(np.float64)
        S = math.fsum(x.tolist())
        E = x.size * 2.0 ** -53 * math.fsum(np.abs(x).tolist())
        bound = E + 2.0 ** -24 * (abs(S) + E)
        diff = abs(float(cv[r]) - S)
        worst = max(worst, diff / bound)
        assert diff <= bound, (r, x.size, float(cv[r]), S, diff, bound)
    print("f32 PLUS: runs", starts.size, "longest", int(np.diff(ends).max()), "largest difference / bound", worst)
    assert np.diff(ends).max() > PIECE


# ---- A and C in every form ----------------------------------------------------------------------------------------------
def test_a_product_result_csr_only_and_in_place(hb, monkeypatch):
    g = hb.g
    rng = np.random.default_rng(60)
    n, nc = 600, 50
    ptr, ind, val = _csr_of(rng, n, 2500, F, lambda m: rng.integers(1, 4, m).astype(F))
    B = _mat(g, ptr, ind, val)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", B, B, hb.descriptor()) == 0      # a product result: a CSR and no CSC
    pcsr = tuple(np.array(x) for x in P.host_csr())
    assert pcsr[1].size > 2500
    mp = rng.integers(-1, nc, n)
    for op in OPS:
        _check(hb, pcsr, mp, nc, op, 0, A=P, name=("product", op))
    csr = (ptr, ind, val)
    Aonly = _mat(g, ptr, ind, val, csr_only=True, monkeypatch=monkeypatch)
    _check(hb, csr, mp, nc, "plus", 1, A=Aonly, name="A CSR only")
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Conly = g.Matrix(nc, nc, F)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    _check(hb, csr, mp, nc, "plus", 1, Cm=Conly, csc=False, name="C CSR only")
    Cfull = _mat(g, *_csr_of(rng, nc, 300, F))            # a C that holds something else, sizes that hold something else
    sz = _vec(g, np.full(nc, 77, I))
    _check(hb, csr, mp, nc, "maximum", 0, Cm=Cfull, sizes=sz, name="prefilled")
    ssz = g.Vector(nc, I)
    assert ssz.build(np.array([1, 5], I), np.array([4, 4], I), 2, None) == 0
    _check(hb, csr, mp, nc, "plus", 0, sizes=ssz, name="sparse sizes")
    _check(hb, csr, mp, nc, "plus", 0, sizes=None, name="null sizes")
    sm = g.Vector(n, I)                                    # a map in sparse storage with every value stored
    assert sm.build(np.arange(n, dtype=I), mp.astype(I), n, None) == 0
    assert sm.getStorage() == g.GrB_SPARSE
    _check(hb, csr, mp, nc, "plus", 1, mapvec=sm, name="sparse map")
    A = _mat(g, ptr, ind, val)                             # C = A when nc = n, last: A is its own contraction now
    merge = np.arange(n) // 2 * 2                          # pairs, raw labels
    _check(hb, csr, merge, n, "plus", 1, A=A, Cm=A, name="in place")


def test_map_on_caller_owned_storage(hb):
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(61)
    n, nc = 1003, 31
    csr = _csr_of(rng, n, 5000, I)
    mp = rng.integers(-1, nc, n).astype(I)
    A = _mat(g, *csr)
    for k in ad.KS:
        mv, t, check = ad.adopt_dense(g, mp, k)
        assert mv.device_ptrs()[2] % 16 == 4 * k
        _check(hb, csr, mp, nc, "plus", 1, A=A, mapvec=mv, name=("adopted", k))
        assert np.array_equal(ad.payload(t, k, n, I), mp)
        check(("contract", k))


def test_degenerate(hb):
    g = hb.g
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    for nc in (0, 3):
        C0 = g.Matrix(nc, nc, F)
        info, res = g.contract(C0, g.Vector(nc, I), A0, g.Vector(0, I), "plus", 0, None)
        assert info == 0 and all(res[x] == 0 for x in REC) and C0.nvals() == 0
    empty = (np.zeros(51, I), np.zeros(0, I), np.zeros(0, I))
    (cp, ci, _), res, _ = _check(hb, empty, np.arange(50) % 7, 7, "plus", 1, name="no entries")
    assert ci.size == 0 and res["clusters"] == 7 and res["largest"] == 8
    info, count = g.relabel(g.Vector(0, I), g.Vector(0, I), LABELS)
    assert (info, count) == (0, 0)


# ---- grb_relabel -------------------------------------------------------------------------------------------------------
def _relabel(hb, labels, kind, in_place=False, sparse=False, name=""):
    g = hb.g
    labels = np.asarray(labels, I)
    n = labels.size
    want, nc = _ref_relabel(labels, kind)
    lv = g.Vector(n, I)
    if sparse:
        assert lv.build(np.arange(n, dtype=I), labels, n, None) == 0
    else:
        assert lv.build(labels, n) == 0
    out = lv if in_place else g.Vector(n, I)
    info, count = g.relabel(out, lv, kind)
    assert info == 0 and count == nc, (name, info, count, nc)
    assert out.getStorage() == g.GrB_DENSE and out.nvals() == n
    got = out.extractTuples()[1]
    assert got.dtype == I and np.array_equal(got, want), (name, np.flatnonzero(got != want)[:10])
    if not in_place:
        assert np.array_equal(lv.extractTuples(sparse=True)[2] if sparse else lv.extractTuples()[1], labels)
    return got, count


def test_relabel_labels_and_mate(hb):
    rng = np.random.default_rng(62)
    n = 5003
    gaps = rng.choice(np.arange(0, n, 3), n)              # labels with gaps
    for in_place in (False, True):
        for sparse in (False, True):
            got, count = _relabel(hb, gaps, LABELS, in_place, sparse, name=("gaps", in_place, sparse))
            assert count < n and got.max() == count - 1
    _relabel(hb, np.arange(n), LABELS, name="identity")
    _relabel(hb, np.zeros(n), LABELS, name="one label")
    _relabel(hb, np.full(n, n - 1), LABELS, name="the last label")
    mate = np.full(n, -1)
    pairs = rng.permutation(n)[:2000].reshape(-1, 2)
    mate[pairs[:, 0]], mate[pairs[:, 1]] = pairs[:, 1], pairs[:, 0]
    for in_place in (False, True):
        got, count = _relabel(hb, mate, MATE, in_place, name=("mate", in_place))
        assert count == n - 1000 and (got[pairs[:, 0]] == got[pairs[:, 1]]).all()
    _relabel(hb, np.full(n, -1), MATE, name="nobody matched")
    _relabel(hb, rng.integers(-1, n, n), MATE, name="no involution: the rule as written")


def test_relabel_of_a_real_matching(hb):
    g = hb.g
    rng = np.random.default_rng(63)
    n = 2000
    u, v = _random_edges(rng, n, 5000)
    gr = Graph(n, u, v, rng.integers(1, 50, u.size), I)
    A = _matrix(g, gr)
    mate = g.Vector(n, I)
    info, res = g.matching(mate, None, A, 0, 0, None)
    assert info == 0 and res["matched"] > 0
    mp = g.Vector(n, I)
    info, count = g.relabel(mp, mate, MATE)
    assert info == 0 and count == n - res["matched"]
    want, nc = _ref_relabel(mate.extractTuples()[1], MATE)
    assert nc == count and np.array_equal(mp.extractTuples()[1], want)


# ---- chains through the library ----------------------------------------------------------------------------------------
def test_cc_relabel_contract_is_empty(hb):
    g = hb.g
    rng = np.random.default_rng(64)
    n = 1500
    u, v = _random_edges(rng, n, 1300)
    gr = Graph(n, u, v, rng.integers(1, 9, u.size), I)
    A = _matrix(g, gr)
    lab = g.Vector(n, I)
    assert g.cc(lab, A, 0, hb.descriptor())[0] == 0
    info, nc = g.relabel(lab, lab, LABELS)
    assert info == 0 and 1 < nc < n
    (cp, ci, _), res, _ = _check(hb, gr.csr(), lab.extractTuples()[1], nc, "plus", 0, A=A, mapvec=lab, name="cc")
    assert ci.size == 0 and cp.size == nc + 1 and res["loops"] == res["kept"] == 2 * u.size and res["clusters"] == nc


def test_scc_relabel_contract_is_acyclic(hb):
    g = hb.g
    rng = np.random.default_rng(65)
    n = 1200
    ptr, ind, val = csr = _csr_of(rng, n, 2600, I)
    A = _mat(g, ptr, ind, val)
    lab = g.Vector(n, I)
    info, res = g.scc(lab, A, None)
    assert info == 0 and 1 < res["components"] < n and res["largest"] > 1
    mp = g.Vector(n, I)
    info, nc = g.relabel(mp, lab, LABELS)
    assert info == 0 and nc == res["components"]
    Cm = g.Matrix(nc, nc, I)
    _check(hb, csr, mp.extractTuples()[1], nc, "plus", 0, A=A, Cm=Cm, mapvec=mp, name="scc")
    again = g.Vector(nc, I)
    info, res2 = g.scc(again, Cm, None)                    # the condensation is acyclic
    assert info == 0 and res2["components"] == nc and np.array_equal(again.extractTuples()[1], np.arange(nc))


def test_matching_relabel_contract_keeps_the_weight(hb):
    g = hb.g
    rng = np.random.default_rng(66)
    u, v = _grid_edges(64)
    n = 64 * 64
    gr = Graph(n, u, v, rng.integers(1, 100, u.size), I)
    A = _matrix(g, gr)
    mate, mp = g.Vector(n, I), g.Vector(n, I)
    info, res = g.matching(mate, None, A, 2, 7, None)
    assert info == 0
    info, nc = g.relabel(mp, mate, MATE)
    assert info == 0 and nc == n - res["matched"] and nc < n
    (_, _, cv), res, _ = _check(hb, gr.csr(), mp.extractTuples()[1], nc, "plus", 1, A=A, mapvec=mp, name="grid")
    assert int(cv.astype(np.int64).sum()) == 2 * int(gr.w.astype(np.int64).sum()) and res["largest"] == 2
    # the next level: match -> coarsen once more
    C1 = g.Matrix(nc, nc, I)
    assert g.contract(C1, None, A, mp, "plus", 0, None)[0] == 0
    mate2 = g.Vector(nc, I)
    assert g.matching(mate2, None, C1, 0, 0, None)[0] == 0


def test_rmat_12_by_cdlp_labels(hb):
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    g = hb.g
    s, d, n = rmat_edges(12, 16, seed=1)
    ptr, ind = finalize_edges(s, d, n, symmetrize=True)["csr"]
    rng = np.random.default_rng(67)
    for dt in (F, I):
        csr = (ptr.astype(I), ind.astype(I), rng.integers(1, 9, ind.size).astype(dt))
        A = _mat(g, *csr)
        lab = g.Vector(n, I)
        assert g.cdlp(lab, A, None)[0] == 0
        labels = lab.extractTuples()[1]
        mp = g.Vector(n, I)
        info, nc = g.relabel(mp, lab, LABELS)
        assert info == 0 and nc == np.unique(labels).size
        for op in OPS:
            _check(hb, csr, mp.extractTuples()[1], nc, op, 1, A=A, mapvec=mp, name=("RMAT-12", op, dt.__name__))
        _check(hb, csr, labels, n, "plus", 0, A=A, mapvec=lab, name=("RMAT-12, raw labels", dt.__name__))


# ---- determinism -------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import graphblast_amd as g
d = np.load(sys.argv[2])
ptr, ind, val, mp = d["ptr"], d["ind"], d["val"], d["map"]
n, nc = ptr.size - 1, int(d["nc"])
A = g.Matrix(n, n, np.float32)
assert A.build_csr(ptr, ind, val) == 0
m = g.Vector(n, np.int32)
assert m.build(mp, n) == 0
C = g.Matrix(nc, nc, np.float32)
info, res = g.contract(C, None, A, m, "plus", 1, None)
assert info == 0, info
p, i, v = C.host_csr()
np.savez(sys.argv[3], ptr=p, ind=i, val=v.view(np.uint32))
"""


def test_two_runs_and_a_child_on_four_cus_give_the_same_bits(hb, tmp_path):
    rng = np.random.default_rng(68)
    n, nc = 4000, 9
    mp = np.minimum(rng.integers(0, 30, n), nc - 1).astype(I)
    csr = _csr_of(rng, n, 300000, F, lambda m: (rng.random(m) * 10.0 ** rng.integers(-4, 5, m)).astype(F))
    A = _mat(hb.g, *csr)
    outs = []
    for _ in range(2):
        (cp, ci, cv), _, (starts, w) = _check(hb, csr, mp, nc, "plus", 1, A=A, name="determinism", exact=False)
        outs.append((cp.tobytes(), ci.tobytes(), cv.tobytes()))
    assert outs[0] == outs[1] and np.diff(np.append(starts, w.size)).max() > 64 * PIECE
    np.savez(tmp_path / "in.npz", ptr=csr[0], ind=csr[1], val=csr[2], map=mp, nc=nc)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, GRB_NUM_CU="4")
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    assert out["ptr"].tobytes() == outs[0][0] and out["ind"].tobytes() == outs[0][1] and out["val"].tobytes() == outs[0][2]


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_c_sizes_and_map_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(69)
    n, nc = 80, 9
    ptr, ind, val = _csr_of(rng, n, 400, F)
    A = _mat(g, ptr, ind, val)
    Cm = _mat(g, *_csr_of(rng, nc, 40, F))
    cbefore = tuple(np.array(x) for x in Cm.host_csr())
    tbefore = tuple(np.array(x) for x in Cm.host_csc())
    sbefore = rng.integers(5, 1000, nc).astype(I)
    sizes = _vec(g, sbefore)
    mp = rng.integers(-1, nc, n).astype(I)
    mv = _vec(g, mp)
    PLUS, FIRST = g.BINARY_OPS.index("plus"), g.BINARY_OPS.index("first")

    def unchanged():
        assert Cm.nvals() == cbefore[1].size
        assert all(np.array_equal(x, y) for x, y in zip(Cm.host_csr(), cbefore))
        assert all(np.array_equal(x, y) for x, y in zip(Cm.host_csc(), tbefore))
        assert sizes.getStorage() == g.GrB_DENSE and np.array_equal(sizes.extractTuples()[1], sbefore)
        return True

    def call(c, s, a, m, op=PLUS, loops=0):
        return lib.grb_contract(c, s, a, m, op, loops, None, None)

    assert call(None, sizes._h, A._h, mv._h) == g.GrB_UNINITIALIZED_OBJECT             # null handles
    assert call(Cm._h, sizes._h, None, mv._h) == g.GrB_UNINITIALIZED_OBJECT
    assert call(Cm._h, sizes._h, A._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(Cm._h, sizes._h, g.Matrix(n, n, F)._h, mv._h) == g.GrB_UNINITIALIZED_OBJECT   # an unbuilt A
    R = g.Matrix(n, n + 1, F)                                                          # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(Cm._h, sizes._h, R._h, mv._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Matrix(nc, nc + 1, F)._h, sizes._h, A._h, mv._h) == g.GrB_DIMENSION_MISMATCH   # C not square
    assert call(Cm._h, sizes._h, A._h, g.Vector(n + 1, I)._h) == g.GrB_DIMENSION_MISMATCH        # size(map) != n
    assert call(Cm._h, g.Vector(nc + 1, I)._h, A._h, mv._h) == g.GrB_DIMENSION_MISMATCH          # size(sizes) != nc
    assert unchanged()
    fv = g.Vector(n, F)                                                                # a map, sizes that are not i32
    assert fv.build(np.zeros(n, F), n) == 0
    assert call(Cm._h, sizes._h, A._h, fv._h) == g.GrB_NOT_IMPLEMENTED
    fs = g.Vector(nc, F)
    assert fs.build(np.full(nc, 3, F), nc) == 0
    assert call(Cm._h, fs._h, A._h, mv._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(fs.extractTuples()[1], np.full(nc, 3, F))
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                           # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(Cm._h, sizes._h, h, mv._h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    Ci = _mat(g, *_csr_of(rng, nc, 40, I))                                             # C not of A's type
    cibefore = tuple(np.array(x) for x in Ci.host_csr())
    assert call(Ci._h, sizes._h, A._h, mv._h) == g.GrB_DOMAIN_MISMATCH
    assert all(np.array_equal(x, y) for x, y in zip(Ci.host_csr(), cibefore))
    for op in range(len(g.BINARY_OPS) + 2):                                            # every other operator
        if g.BINARY_OPS[op:op + 1] not in (["plus"], ["minimum"], ["maximum"], ["first"]):
            assert call(Cm._h, sizes._h, A._h, mv._h, op) == g.GrB_NOT_IMPLEMENTED, op
    assert call(Cm._h, sizes._h, A._h, mv._h, -1) == g.GrB_NOT_IMPLEMENTED
    for loops in (-1, 2, 7):                                                           # loops outside {0, 1}
        assert call(Cm._h, sizes._h, A._h, mv._h, PLUS, loops) == g.GrB_INVALID_VALUE
    part = g.Vector(n, I)                                                              # nvals(map) != n
    assert part.build(np.array([3, 9], I), np.array([1, 2], I), 2, None) == 0
    assert call(Cm._h, sizes._h, A._h, part._h) == g.GrB_INVALID_VALUE
    assert call(Cm._h, sizes._h, A._h, g.Vector(n, I)._h) == g.GrB_INVALID_VALUE       # a map that holds nothing yet
    assert unchanged()
    for where, bad in ((0, nc), (n - 1, -2), (n // 2, 2 ** 31 - 1), (5, -2 ** 31)):      # a map value out of range
        x = mp.copy()
        x[where] = bad
        for op in (PLUS, FIRST):
            for s_ in (sizes._h, None):
                assert call(Cm._h, s_, A._h, _vec(g, x)._h, op, 1) == g.GrB_INVALID_INDEX, (where, bad)
        sm = g.Vector(n, I)
        assert sm.build(np.arange(n, dtype=I), x, n, None) == 0
        assert call(Cm._h, sizes._h, A._h, sm._h) == g.GrB_INVALID_INDEX
        assert unchanged()
    assert np.array_equal(mv.extractTuples()[1], mp)
    # grb_relabel
    lv = _vec(g, np.arange(n, dtype=I) // 2)
    before = rng.integers(5, 1000, n).astype(I)
    out = _vec(g, before)
    cnt = ctypes.c_int32(-5)

    def rl(m, l_, kind=0):
        return lib.grb_relabel(m, l_, kind, ctypes.byref(cnt), None)

    assert rl(None, lv._h) == g.GrB_UNINITIALIZED_OBJECT and rl(out._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert rl(g.Vector(n + 1, I)._h, lv._h) == g.GrB_DIMENSION_MISMATCH
    assert rl(fv._h, lv._h) == g.GrB_NOT_IMPLEMENTED and rl(out._h, fv._h) == g.GrB_NOT_IMPLEMENTED
    assert rl(out._h, lv._h, 2) == g.GrB_INVALID_VALUE and rl(out._h, lv._h, -1) == g.GrB_INVALID_VALUE
    assert rl(out._h, part._h) == g.GrB_INVALID_VALUE
    for kind, bad in ((LABELS, -1), (LABELS, n), (MATE, -2), (MATE, n)):
        x = np.arange(n, dtype=I)
        x[n // 3] = bad
        assert rl(out._h, _vec(g, x)._h, kind) == g.GrB_INVALID_INDEX, (kind, bad)
        xv = _vec(g, x)
        assert rl(xv._h, xv._h, kind) == g.GrB_INVALID_INDEX                           # in place: labels keeps its values
        assert np.array_equal(xv.extractTuples()[1], x)
    assert np.array_equal(out.extractTuples()[1], before) and cnt.value == -5
    assert lib.grb_relabel(out._h, lv._h, 0, None, None) == 0                          # count is optional
    assert np.array_equal(out.extractTuples()[1], np.arange(n) // 2)
    # a descriptor and a null descriptor; the record is optional
    C1, C2 = g.Matrix(nc, nc, F), g.Matrix(nc, nc, F)
    assert lib.grb_contract(C1._h, None, A._h, mv._h, PLUS, 1, hb.descriptor()._h, None) == 0 and call(C2._h, None, A._h, mv._h, PLUS, 1) == 0
    assert all(np.array_equal(x, y) for x, y in zip(C1.host_csr(), C2.host_csr()))


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def test_cpp_frontend(tmp_path):
    """tests/tools/contract.cpp on chesapeake.mtx: pairs (v / 2) by PLUS without loops on a float matrix, communities (v % 5) by
    MAXIMUM with loops on an int matrix, and relabel of the labels 3 (v / 4)"""
    exe = str(tmp_path / "contract")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "contract.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    path = os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    co = sp.coo_matrix(scipy.io.mmread(path))
    n = co.shape[0]
    key = np.unique(np.concatenate([co.row.astype(np.int64) * n + co.col, co.col.astype(np.int64) * n + co.row]))
    rr, cc = key // n, key % n
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rr, minlength=n), out=ptr[1:])
    w = 1 + (rr + 3 * cc) % 7

    def line(tag, csr, rec, sizes):
        p, i, v = csr
        return "%s kept %d loops %d entries %d clusters %d dropped %d largest %d | %s | %s | %s | %s" % (
            tag, rec["kept"], rec["loops"], rec["entries"], rec["clusters"], rec["dropped"], rec["largest"], " ".join(map(str, p.tolist())),
            " ".join(map(str, i.tolist())), " ".join("%g" % x for x in v.tolist()), " ".join(map(str, sizes.tolist())))

    v = np.arange(n)
    nc = (n + 1) // 2
    csr, _, sizes, rec, _ = _ref(ptr.astype(I), cc.astype(I), w.astype(F), v // 2, nc, "plus", 0)
    assert line("pairs", csr, rec, sizes) in lines
    mp = np.where(v % 11 == 0, -1, v % 5)
    csr, _, sizes, rec, _ = _ref(ptr.astype(I), cc.astype(I), w.astype(I), mp, 5, "maximum", 1)
    assert line("communities", csr, rec, sizes) in lines
    want, count = _ref_relabel((3 * (v // 4)).astype(I), LABELS)
    assert "relabel %d | %s" % (count, " ".join(map(str, want.tolist()))) in lines
    assert lines[-1] == "ok"
