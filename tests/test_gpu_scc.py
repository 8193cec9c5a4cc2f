"""The strongly connected components on the device (csrc/scc.hip: grb_scc) against scipy.sparse.csgraph's
connected_components(directed=True, connection="strong"), relabelled to each component's smallest member as the definition
in include/grb_hip.h asks.  Every comparison is EXACT: all n labels and edges, components, largest, trivial and launches
of the record.  Random digraphs below, at and above the giant component's threshold in both element types with values that
must not matter, RMAT as drawn and relabelled, closed forms, chains of small components both ways round, a randomly
oriented grid, every row-length class of the kernel straddled, symmetric inputs against the library's own grb_cc, A against
its transpose, every error code with the output unchanged, degenerate shapes, the output's state beforehand, caller-owned
storage, determinism and the C++ frontend."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
# csrc/scc.hip.  One launch of GRID workgroups (one per CU) of THREADS threads, WAVES waves each
LANE_LEN = 8       # kScLaneLen: a frontier vertex whose row or column has up to this many entries is walked by one lane
WAVE_LEN = 2048    # kScWaveLen: ... up to this many by a wave, a longer one by the workgroup
STAGE = 256        # kScStage: appends a wave stages in LDS; it reserves room for them once more than STAGE - 64 are staged
THREADS = 1024     # kPThreads
WAVES = 16         # kPWaves: a pass deals its frontier to the GRID x WAVES waves: one vertex a wave up to that many, then
                   # ceil(frontier / waves) a wave, at most 64
LAUNCHES = 1       # what the record's launches says, whatever the graph
REC = ("edges", "components", "largest", "trivial", "launches")


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


def _grid(hb):
    """the workgroups of the launch: the device's CUs (GRB_NUM_CU takes fewer)"""
    g = next(int(x) for x in hb.g.device_info().split(":") if x.isdigit())
    e = os.environ.get("GRB_NUM_CU")
    return int(e) if e and 1 <= int(e) < g else g


# ---- graphs and the reference ------------------------------------------------------------------------------------------
def _pattern(n, r, c):
    """the 0 / 1 pattern of the entries (r, c), duplicates merged, columns ascending; the diagonal stays if given"""
    S = sp.csr_matrix((np.ones(len(r), np.int64), (np.asarray(r, np.int64), np.asarray(c, np.int64))), shape=(n, n))
    S.data[:] = 1
    S.sort_indices()
    return S


def _cat(parts):
    return np.concatenate([np.asarray(p, np.int64).ravel() for p in parts]) if parts else np.zeros(0, np.int64)


def _ref(S):
    """-> labels (i32: the smallest member of each strong component), dict(edges, components, largest, trivial, launches)"""
    n = S.shape[0]
    if n == 0:
        return np.zeros(0, I), dict(edges=0, components=0, largest=0, trivial=0, launches=0)
    k, lab = connected_components(S, directed=True, connection="strong")
    low = np.full(k, n, np.int64)
    np.minimum.at(low, lab, np.arange(n))
    sizes = np.bincount(lab, minlength=k)
    B = sp.csr_matrix(S, copy=True)
    B.setdiag(0)
    B.eliminate_zeros()
    return low[lab].astype(I), dict(edges=int(B.nnz), components=int(k), largest=int(sizes.max()), trivial=int((sizes == 1).sum()),
                                    launches=LAUNCHES)


def _matrix(g, S, dt=F, rng=None):
    """A with S's structure; values that must not matter (zeros and negatives among them)"""
    n = S.shape[0]
    vals = np.ones(S.nnz, dt) if rng is None else rng.integers(-3, 4, S.nnz).astype(dt)
    A = g.Matrix(n, n, dt)
    assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), vals) == 0
    return A


def _values(g, v, n):
    assert v.getStorage() == g.GrB_DENSE and v.nvals() == n and v.np_dtype == I
    info, vals = v.extractTuples()
    assert info == 0 and vals.dtype == I and vals.size == n
    return vals


def _check(hb, S, A=None, name="", want=None, v=None):
    """grb_scc on S's graph against the reference, exactly; -> (labels, record)"""
    g = hb.g
    n = S.shape[0]
    if A is None:
        A = _matrix(g, S)
    if want is None:
        want = _ref(S)
    if v is None:
        v = g.Vector(n, I)
    info, res = g.scc(v, A, None)
    assert info == 0, (name, info)
    got = _values(g, v, n)
    print(name, {x: res[x] for x in REC}, "trimmed", res["trimmed"], "rounds", res["rounds"], "passes", res["passes"], "loop_ms", res["loop_ms"])
    bad = np.flatnonzero(got != want[0])
    assert bad.size == 0, (name, bad.size, bad[:10], got[bad[:10]], want[0][bad[:10]])
    for x in REC:
        assert res[x] == want[1][x], (name, x, res, want[1])
    assert res["loop_ms"] >= 0 and res["passes"] >= 1 and 0 <= res["trimmed"] <= want[1]["trivial"] and res["rounds"] >= 0
    return got, res


def _relabel(S, perm):
    """vertex v becomes perm[v]"""
    co = S.tocoo()
    return _pattern(S.shape[0], perm[co.row], perm[co.col])


def _rmat(scale, seed):
    from graphblast_amd.graphgen import rmat_edges
    s, d, n = rmat_edges(scale, 16, seed=seed)
    return _pattern(n, np.asarray(s), np.asarray(d))


def _cycle(first, m):
    a = first + np.arange(m)
    return a, first + (np.arange(m) + 1) % m


# ---- random digraphs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 5000])
def test_random_digraphs(hb, dt, n):
    """about 0.5, 1.5 and 4 edges a vertex: mostly acyclic, at the giant component's threshold, one giant; with and without
    stored diagonals; values that must not matter"""
    for density in (0.5, 1.5, 4.0):
        for diag in (False, True):
            rng = np.random.default_rng(int(1000 * density) + n + diag)
            m = max(1, int(density * n))
            r, c = rng.integers(0, n, m), rng.integers(0, n, m)
            if diag:
                d = rng.integers(0, n, 1 + n // 10)
                r, c = np.concatenate([r, d]), np.concatenate([c, d])
            else:
                r, c = r[r != c], c[r != c]
            S = _pattern(n, r, c)
            assert (S.diagonal().sum() > 0) == diag
            _check(hb, S, _matrix(hb.g, S, dt, rng), name=("random", dt.__name__, n, density, diag))


@pytest.mark.parametrize("scale", [10, 12])
def test_rmat_as_drawn_and_relabelled(hb, scale):
    """directed RMAT, and again under a random relabelling: the same partition, labelled by its minima in the new numbering.
    Relabelled, the smallest vertex is not in the giant component"""
    S = _rmat(scale, 3 + scale)
    n = S.shape[0]
    want = _ref(S)
    assert want[1]["largest"] > n // 8 and want[1]["components"] > 10
    got, res = _check(hb, S, _matrix(hb.g, S, I, np.random.default_rng(scale)), name=("rmat", scale), want=want)
    perm = np.random.default_rng(63 + scale).permutation(n)
    Sp = _relabel(S, perm)
    wantp = _ref(Sp)
    giant = np.bincount(wantp[0]).argmax()
    assert giant != 0 and wantp[0][0] != giant
    gotp, resp = _check(hb, Sp, name=("rmat relabelled", scale), want=wantp)
    # the same partition: the label of perm[v] is the smallest perm[u] over v's component
    low = np.full(n, n, np.int64)
    np.minimum.at(low, got, perm)
    assert np.array_equal(gotp[perm], low[got])
    assert [resp[x] for x in REC] == [res[x] for x in REC]


# ---- closed forms ------------------------------------------------------------------------------------------------------
def _closed(hb, S, labels, name, **rec):
    """a graph whose components are a formula: the device against the formula, and the reference against it too"""
    labels = np.asarray(labels, I)
    want = _ref(S)
    assert np.array_equal(want[0], labels), name
    for x, y in rec.items():
        assert want[1][x] == y, (name, x, want[1], y)
    return _check(hb, S, name=name, want=want)


def test_closed_forms(hb):
    n = 3000
    _closed(hb, _pattern(n, *_cycle(0, n)), np.zeros(n), "cycle", components=1, largest=n, trivial=0, edges=n)
    a = np.arange(n - 1)
    _, res = _closed(hb, _pattern(n, a, a + 1), np.arange(n), "path", components=n, trivial=n, largest=1)
    assert res["rounds"] == 0 and res["trimmed"] == n
    _, res = _closed(hb, _pattern(n, a + 1, a), np.arange(n), "path down", components=n, trivial=n)
    assert res["rounds"] == 0 and res["trimmed"] == n
    rng = np.random.default_rng(20)
    r, c = rng.integers(0, n, 4 * n), rng.integers(0, n, 4 * n)
    perm = rng.permutation(n)                                   # a DAG: every edge goes up in a hidden order
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    keep = lo != hi
    _, res = _closed(hb, _pattern(n, perm[lo[keep]], perm[hi[keep]]), np.arange(n), "dag", components=n, trivial=n, largest=1)
    assert res["rounds"] == 0 and res["trimmed"] == n
    m = 200
    r, c = np.nonzero(~np.eye(m, dtype=bool))
    _closed(hb, _pattern(m, r, c), np.zeros(m), "complete", components=1, largest=m, edges=m * (m - 1))
    _, res = _closed(hb, _pattern(n, np.zeros(n - 1), 1 + a), np.arange(n), "star outward", components=n, trivial=n)
    assert res["rounds"] == 0
    _closed(hb, _pattern(n, 1 + a, np.zeros(n - 1)), np.arange(n), "star inward", components=n, trivial=n)


@pytest.mark.parametrize("way", ["low to high", "high to low"])
def test_two_cycles_joined_by_one_edge(hb, way):
    p, q = 700, 501
    r1, c1 = _cycle(0, p)
    r2, c2 = _cycle(p, q)
    e = (13, p + 7) if way == "low to high" else (p + 7, 13)
    labels = np.concatenate([np.zeros(p), np.full(q, p)])
    S = _pattern(p + q, _cat([r1, r2, [e[0]]]), _cat([c1, c2, [e[1]]]))
    _closed(hb, S, labels, ("two cycles", way), components=2, largest=p, trivial=0)
    _closed(hb, sp.csr_matrix(S.T), labels, ("two cycles reversed", way), components=2, largest=p, trivial=0)


def test_bidirected_grid(hb):
    w = 40
    idx = np.arange(w * w).reshape(w, w)
    r = _cat([idx[:, :-1], idx[:-1, :]])
    c = _cat([idx[:, 1:], idx[1:, :]])
    _closed(hb, _pattern(w * w, _cat([r, c]), _cat([c, r])), np.zeros(w * w), "grid both ways", components=1, largest=w * w)


# ---- chains of small components ----------------------------------------------------------------------------------------
def _chain_of_cycles(lengths, up=True):
    """cycles of the given lengths, one after the other; the last vertex of each has an edge to the first of the next (up)
    or the other way round"""
    r, c, first = [], [], 0
    for i, m in enumerate(lengths):
        a, b = _cycle(first, m)
        r.append(a)
        c.append(b)
        if i + 1 < len(lengths):
            x, y = first + m - 1, first + m
            r.append([x if up else y])
            c.append([y if up else x])
        first += m
    return _pattern(first, _cat(r), _cat(c))


@pytest.mark.parametrize("name", ["200 up", "200 down", "500 relabelled", "lengths 2..39", "lengths 2..39 relabelled"])
def test_chains(hb, name):
    """a one-way chain of small components costs a round a component in one direction of the colouring and one round in the
    other: alternating bounds both.  rounds <= 64 is a cap that catches a lost alternation (a synchronous model needs 13)"""
    if name.startswith("200"):
        S = _chain_of_cycles([2] * 200, up=name.endswith("up"))
    elif name.startswith("500"):
        S = _chain_of_cycles([2] * 500)
        S = _relabel(S, np.random.default_rng(21).permutation(S.shape[0]))
    else:
        S = _chain_of_cycles(list(range(2, 40)))
        assert S.shape[0] == 779
        if name.endswith("relabelled"):
            S = _relabel(S, np.random.default_rng(22).permutation(779))
    want = _ref(S)
    assert want[1]["trivial"] == 0 and want[1]["components"] == {"2": 200, "5": 500, "l": 38}[name[0]]
    _, res = _check(hb, S, name=("chain", name), want=want)
    assert 1 <= res["rounds"] <= 64, res


def test_randomly_oriented_grid(hb):
    """100 x 100, every grid edge one way by a coin: thousands of components of every small size"""
    w = 100
    idx = np.arange(w * w).reshape(w, w)
    a = _cat([idx[:, :-1], idx[:-1, :]])
    b = _cat([idx[:, 1:], idx[1:, :]])
    flip = np.random.default_rng(23).random(a.size) < 0.5
    S = _pattern(w * w, np.where(flip, b, a), np.where(flip, a, b))
    want = _ref(S)
    assert (want[1]["components"], want[1]["largest"]) == (3884, 930), want[1]   # this seed's, from scipy
    _, res = _check(hb, S, name="oriented grid", want=want)
    assert res["rounds"] >= 1


# ---- the row-length classes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [LANE_LEN - 1, LANE_LEN, LANE_LEN + 1, WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1])
@pytest.mark.parametrize("relabel", [False, True])
def test_row_length_classes(hb, length, relabel):
    """x and z: a row and a column of `length` entries each, inside one cycle through their neighbours (x -> o_i -> z ->
    i_j -> x): the sweeps of the giant component or of a colouring walk them.  s: a source whose row has `length` entries,
    each with no other in-edge: trimmed in pass 0, and its row's walk trims all of them in one pass -- `length` appends out
    of one row, more than a wave stages once length > STAGE - 64.  t: a sink whose column has `length` entries, the same
    from the other side.  Both hang on a triangle that stays"""
    L = length
    x, z = 0, 1
    o = 2 + np.arange(L)
    i = 2 + L + np.arange(L)
    nxt = 2 + 2 * L
    tri = nxt + np.arange(3)
    s, t = nxt + 3, nxt + 4
    so = nxt + 5 + np.arange(L)
    ti = nxt + 5 + L + np.arange(L)
    n = nxt + 5 + 2 * L
    r = [np.full(L, x), o, np.full(L, z), i, tri, np.full(L, s), so, np.full(L, tri[1]), ti]
    c = [o, np.full(L, z), i, np.full(L, x), np.roll(tri, -1), so, np.full(L, tri[0]), ti, np.full(L, t)]
    S = _pattern(n, _cat(r), _cat(c))
    perm = np.random.default_rng(30 + L).permutation(n) if relabel else np.arange(n)
    S = _relabel(S, perm)
    T = sp.csr_matrix(S.T)
    T.sort_indices()
    for v in (x, z):
        assert S.indptr[perm[v] + 1] - S.indptr[perm[v]] == L and T.indptr[perm[v] + 1] - T.indptr[perm[v]] == L
    assert S.indptr[perm[s] + 1] - S.indptr[perm[s]] == L and T.indptr[perm[t] + 1] - T.indptr[perm[t]] == L
    want = _ref(S)
    assert want[1]["components"] == 2 + 2 + 2 * L and want[1]["largest"] == 2 + 2 * L and want[1]["trivial"] == 2 + 2 * L
    _, res = _check(hb, S, name=("classes", L, relabel), want=want)
    assert res["trimmed"] == 2 + 2 * L


@pytest.mark.parametrize("length", [LANE_LEN - 1, LANE_LEN, LANE_LEN + 1, WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1, WAVE_LEN + 300])
def test_row_length_classes_inside_a_colouring(hb, length):
    """the same classes in the colouring rounds: a complete digraph of 60 takes the pivot (59 x 59 beats every other
    in-degree x out-degree here), so the cycle h -> o_i -> w -> h over `length` vertices o_i is left to a round: h's row is
    walked when the colours travel along rows, w's column when the component is collected along columns, and on the
    transposed graph it is w's row and h's column.  Every o_i is appended by one walk: more than a wave stages once
    length > STAGE - 64"""
    m, L = 60, length
    kr, kc = np.nonzero(~np.eye(m, dtype=bool))
    h, w = m, m + 1
    o = m + 2 + np.arange(L)
    n = m + 2 + L
    S = _pattern(n, _cat([kr, np.full(L, h), o, [w]]), _cat([kc, o, np.full(L, w), [h]]))
    assert 59 * 59 > L
    T = sp.csr_matrix(S.T)
    T.sort_indices()
    for name, G in (("hub", S), ("hub transposed", T), ("hub relabelled", _relabel(S, np.random.default_rng(31 + L).permutation(n)))):
        want = _ref(G)
        assert want[1]["components"] == 2 and want[1]["largest"] == max(L + 2, m) and want[1]["trivial"] == 0
        _, res = _check(hb, G, name=(name, L), want=want)
        assert res["rounds"] == 1 and res["trimmed"] == 0


# ---- symmetric inputs: the connected components ------------------------------------------------------------------------
def _partition_equal(a, b):
    """two labellings give the same partition"""
    _, ia = np.unique(a, return_inverse=True)
    _, ib = np.unique(b, return_inverse=True)
    return np.unique(np.stack([ia, ib]), axis=1).shape[1] == ia.max() + 1 == ib.max() + 1


def test_symmetric_inputs_give_the_connected_components(hb):
    g = hb.g
    rng = np.random.default_rng(24)
    n = 3000
    r, c = rng.integers(0, n, 2200), rng.integers(0, n, 2200)       # below the threshold: several hundred components
    M = sp.csr_matrix(scipy.io.mmread(os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")))
    co = M.tocoo()
    for name, S in (("random undirected", _pattern(n, _cat([r, c]), _cat([c, r]))),
                    ("chesapeake", _pattern(M.shape[0], _cat([co.row, co.col]), _cat([co.col, co.row])))):
        m = S.shape[0]
        want = _ref(S)
        k, weak = connected_components(S, directed=False)
        assert k == want[1]["components"] and _partition_equal(weak, want[0])
        A = _matrix(g, S, I)
        got, _ = _check(hb, S, A, name=name, want=want)
        v = g.Vector(m, I)
        info, _ = g.cc(v, A, 0, hb.descriptor())
        assert info == 0
        assert _partition_equal(v.extractTuples()[1], got), name


def test_a_and_its_transpose(hb):
    rng = np.random.default_rng(25)
    n = 4000
    r, c = rng.integers(0, n, 6000), rng.integers(0, n, 6000)
    S, T = _pattern(n, r, c), _pattern(n, c, r)
    want = _ref(S)
    assert 1 < want[1]["largest"] < n and want[1]["components"] > 100
    got, res = _check(hb, S, name="A", want=want)
    gott, rest = _check(hb, T, name="A transposed", want=want)
    assert got.tobytes() == gott.tobytes() and [res[x] for x in REC] == [rest[x] for x in REC]


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_unchanged(hb, monkeypatch):
    import test_gpu_adopted_storage as ad
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(13)
    n = 80
    S = _pattern(n, rng.integers(0, n, 300), rng.integers(0, n, 300))
    A = _matrix(g, S, F, rng)
    before = rng.integers(5, 1000, n).astype(I)
    v = g.Vector(n, I)
    assert v.build(before, n) == 0

    def unchanged():
        return v.getStorage() == g.GrB_DENSE and np.array_equal(v.extractTuples()[1], before)

    def call(v_, A_):
        return lib.grb_scc(v_, A_, None, None)

    R = g.Matrix(n, n + 1, F)                                                         # A not square
    assert R.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)) == 0
    fv = g.Vector(n, F)                                                               # an output that is not i32
    fbefore = rng.random(n).astype(F) + 2
    assert fv.build(fbefore, n) == 0
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                          # an A of element type code 2
    hp, hi, hv = S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)
    assert lib.grb_matrix_build_csr(h, hp.ctypes.data, hi.ctypes.data, hv.ctypes.data, S.nnz, None, None, None) == 0
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")                               # the CSR-only format: no CSC
    Q = _matrix(g, S, I)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    P = g.Matrix(n, n, F)                                                             # a product result: no CSC of its own
    One = _matrix(g, S, F)
    assert g.mxm(P, None, None, "PlusMultiplies", One, One, hb.descriptor()) == 0
    sv = g.Vector(n, I)                                                               # a sparse output stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0
    ev = g.Vector(n, I)                                                               # an empty one stays empty
    av, at, acheck = ad.adopt_dense(g, before, 3)                                     # caller-owned storage at an odd alignment
    assert av.device_ptrs()[2] % 16 == 12

    assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                              # null handles
    assert call(v._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(v._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT             # an unbuilt A
    assert call(v._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH              # size(scc) != n
    assert unchanged()
    assert call(fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(fv.extractTuples()[1].view(np.uint32), fbefore.view(np.uint32))
    assert call(v._h, h) == g.GrB_NOT_IMPLEMENTED
    assert unchanged()
    for bad in (Q, P):
        for code, M in ((g.GrB_INVALID_OBJECT, bad._h), (g.GrB_DIMENSION_MISMATCH, R._h), (g.GrB_NOT_IMPLEMENTED, h)):
            assert call(v._h, M) == code
            assert unchanged()
            assert call(sv._h, M) == code
            assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
            info, si, sx = sv.extractTuples(sparse=True)
            assert info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]
            assert call(ev._h, M) == code
            assert ev.nvals() == 0
            assert call(av._h, M) == code
            assert np.array_equal(ad.payload(at, 3, n, I), before)
            acheck(("scc error", code))
    assert lib.grb_matrix_free(h) == 0
    # a descriptor and a null descriptor give the same result; the record is optional
    w = g.Vector(n, I)
    assert lib.grb_scc(w._h, A._h, hb.descriptor()._h, None) == 0
    assert lib.grb_scc(v._h, A._h, None, None) == 0 and not unchanged()
    assert np.array_equal(v.extractTuples()[1], w.extractTuples()[1]) and np.array_equal(w.extractTuples()[1], _ref(S)[0])
    assert lib.grb_scc(av._h, A._h, None, None) == 0                                   # ... and into the caller's storage
    assert np.array_equal(ad.payload(at, 3, n, I), _ref(S)[0])
    acheck("scc adopted")


# ---- degenerate shapes, the output's storage beforehand ----------------------------------------------------------------
def test_degenerate(hb):
    g = hb.g
    for n, diag in ((1, []), (1, [0]), (50, []), (50, np.arange(0, 50, 3)), (50, np.arange(50))):
        S = _pattern(n, diag, diag)
        want = (np.arange(n, dtype=I), dict(edges=0, components=n, largest=1, trivial=n, launches=LAUNCHES))
        assert np.array_equal(_ref(S)[0], want[0]) and _ref(S)[1] == want[1]
        _, res = _check(hb, S, name=("degenerate", n, len(diag)), want=want)
        assert res["rounds"] == 0 and res["trimmed"] == n
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    v0 = g.Vector(0, I)
    info, res = g.scc(v0, A0, None)
    assert info == 0 and all(res[x] == 0 for x in res if x != "loop_ms") and res["loop_ms"] == 0


def test_more_vertices_than_one_pass_deals_out(hb):
    """pass 0 trims more than four isolated vertices a thread -- every wave of the scan stages 256 of them, more than it
    holds before it reserves room --; the rest are two-cycles, more than 64 a wave in the one colouring round"""
    n = 6 * _grid(hb) * THREADS + 6
    iso = 4 * _grid(hb) * THREADS + 3
    m = (n - iso) // 2
    assert 2 * m > 64 * _grid(hb) * WAVES
    a = iso + 2 * np.arange(m)
    S = _pattern(n, _cat([a, a + 1]), _cat([a + 1, a]))
    labels = np.arange(n, dtype=I)
    labels[a + 1] = a
    trivial = n - 2 * m
    want = (labels, dict(edges=2 * m, components=trivial + m, largest=2, trivial=trivial, launches=LAUNCHES))
    _, res = _check(hb, S, name="isolated and two-cycles", want=want)
    assert res["trimmed"] == trivial


def test_output_sparse_dense_or_empty_beforehand(hb):
    g = hb.g
    rng = np.random.default_rng(14)
    n = 400
    S = _pattern(n, rng.integers(0, n, 600), rng.integers(0, n, 600))
    A = _matrix(g, S, F)
    want = _ref(S)
    dense = g.Vector(n, I)
    assert dense.build(np.full(n, 9, I), n) == 0
    sparse = g.Vector(n, I)
    assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
    outs = [_check(hb, S, A, name=name, want=want, v=v)[0].tobytes()
            for name, v in (("dense", dense), ("sparse", sparse), ("fresh", g.Vector(n, I)))]
    assert outs[0] == outs[1] == outs[2]


def test_output_on_caller_owned_storage(hb):
    """the output adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(15)
    n = 1003
    S = _pattern(n, rng.integers(0, n, 1600), rng.integers(0, n, 1600))
    A = _matrix(g, S, F)
    want = _ref(S)
    for k in ad.KS:
        v, t, check = ad.adopt_dense(g, np.full(n, 77, I), k)
        assert v.device_ptrs()[2] % 16 == 4 * k
        got, _ = _check(hb, S, A, name=("adopted", k), want=want, v=v)
        assert np.array_equal(ad.payload(t, k, n, I), got)
        check(("scc", k))


# ---- determinism -------------------------------------------------------------------------------------------------------
def test_determinism(hb):
    g = hb.g
    S = _rmat(12, 6)
    want = _ref(S)
    A = _matrix(g, S, F)
    outs = []
    for _ in range(5):
        got, res = _check(hb, S, A, name="rmat12", want=want)
        assert res["launches"] == 1
        outs.append((got.tobytes(), [res[x] for x in REC]))
    assert all(o == outs[0] for o in outs)


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def test_cpp_frontend(tmp_path):
    """tests/tools/scc.cpp: two cycles and a one-way edge; a ring with a chord through a const int matrix and a NULL
    descriptor; a DAG.  It checks its own expected values"""
    exe = str(tmp_path / "scc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "scc.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    assert lines[-1] == "ok" and "bowtie scc 0 1 1 1 4 4 4 7" in lines and "ring scc 0 0 0 0 0 0 0 0" in lines
    assert "dag scc 0 1 2 3 4 5" in lines
    S = _pattern(8, [1, 2, 3, 4, 5, 6, 3, 0], [2, 3, 1, 5, 6, 4, 4, 1])
    assert _ref(S)[0].tolist() == [0, 1, 1, 1, 4, 4, 4, 7]
