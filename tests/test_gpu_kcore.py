"""The k-core decomposition on the device (csrc/kcore.hip: grb_coreness, grb_kcore) against a numpy restatement of the
definition in include/grb_hip.h: a vectorised synchronous peel (take the smallest live degree as k, remove every live vertex
of degree <= k until none is left, subtract a bincount of the removed vertices' neighbours), cross-checked once against a
sequential heap-based peel; the k-core's degrees are the row sums of the pattern restricted to core >= k.  Every
comparison is EXACT: all i32 values and every integer of the record except rounds.  Random graphs in both element types
with values that must not matter, closed forms, many rounds, many and skipped levels, every row-length class of the kernel
straddled at every frontier density, the library's own trussness as a cross-check, a golden graph, a product result, the
CSR-only format, every error code with the output unchanged, degenerate shapes, the output's state beforehand,
caller-owned storage, determinism, a relabelling and the C++ frontend."""
import ctypes
import heapq
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
# csrc/kcore.hip.  One launch of GRID workgroups (one per CU) of THREADS threads, WAVES waves each
LANE_LEN = 8       # kKcLaneLen: a frontier vertex whose CSR row has up to this many entries is walked by one lane
WAVE_LEN = 2048    # kKcWaveLen: ... up to this many by a wave, a longer one by the workgroup
STAGE = 256        # kKcStage: appends a wave stages in LDS; it reserves room for them once more than STAGE - 64 are staged
THREADS = 1024     # kPThreads
WAVES = 16         # kPWaves: a round deals the frontier to the GRID x WAVES waves: one vertex a wave up to that many, then
                   # ceil(frontier / waves) a wave, at most 64
LAUNCHES = 1       # what the record's launches says, whatever the graph
REC = ("edges", "result_edges", "kmax", "levels", "result_vertices", "launches")


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


def _sym(n, r, c, diag=None):
    """the undirected graph of the draws: loops dropped, both directions; diag: rows that also store their diagonal"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    r, c = r[keep], c[keep]
    d = np.zeros(0, np.int64) if diag is None else np.asarray(diag, np.int64)
    return _pattern(n, np.concatenate([r, c, d]), np.concatenate([c, r, d]))


def _graph(S):
    """S without its diagonal -> (pointers, indices)"""
    B = sp.csr_matrix(S, dtype=np.int64, copy=True)
    B.setdiag(0)
    B.eliminate_zeros()
    B.sort_indices()
    return B.indptr.astype(np.int64), B.indices.astype(np.int64)


def _peel(S):
    """-> core (i32), synchronous rounds, non-empty levels: the vectorised peel"""
    n = S.shape[0]
    ptr, ind = _graph(S)
    deg = np.diff(ptr)
    core = np.zeros(n, np.int64)
    live = np.ones(n, bool)
    rounds = levels = 0
    while live.any():
        k = deg[live].min()
        levels += 1
        while True:
            f = np.flatnonzero(live & (deg <= k))
            if f.size == 0:
                break
            core[f] = k
            live[f] = False
            lens = ptr[f + 1] - ptr[f]
            at = np.repeat(ptr[f] - (np.cumsum(lens) - lens), lens) + np.arange(lens.sum())
            deg = deg - np.bincount(ind[at], minlength=n)
            rounds += 1
    return core.astype(I), rounds, levels


def _heap_peel(S):
    """the sequential algorithm: always remove a vertex of the smallest degree left; core = the running maximum"""
    n = S.shape[0]
    ptr, ind = _graph(S)
    deg = np.diff(ptr).tolist()
    heap = [(d, v) for v, d in enumerate(deg)]
    heapq.heapify(heap)
    gone = [False] * n
    core = np.zeros(n, I)
    k = 0
    while heap:
        d, v = heapq.heappop(heap)
        if gone[v] or d != deg[v]:
            continue
        k = max(k, d)
        core[v] = k
        gone[v] = True
        for u in ind[ptr[v]:ptr[v + 1]].tolist():
            if not gone[u]:
                deg[u] -= 1
                heapq.heappush(heap, (deg[u], u))
    return core


def _inside(S, member):
    """-> per vertex its neighbours among `member` (0 outside it), and the edges among them"""
    ptr, ind = _graph(S)
    n = S.shape[0]
    B = sp.csr_matrix((np.ones(ind.size, np.int64), ind, ptr), shape=(n, n))
    m = member.astype(np.int64)
    d = (B @ m) * m
    return d.astype(I), int(d.sum()) // 2


def _ref(S):
    """-> core, dict(edges, result_edges, kmax, levels, result_vertices, launches), rounds of the synchronous peel"""
    n = S.shape[0]
    core, rounds, levels = _peel(S)
    kmax = int(core.max()) if n else 0
    _, inner = _inside(S, core == kmax) if n else (None, 0)
    rec = dict(edges=int(_graph(S)[1].size) // 2, result_edges=inner, kmax=kmax, levels=levels,
               result_vertices=int((core == kmax).sum()) if n else 0, launches=LAUNCHES)
    return core, rec, rounds


def _ref_kcore(S, core, k):
    member = core >= k
    v, inner = _inside(S, member)
    return v, dict(edges=int(_graph(S)[1].size) // 2, result_edges=inner, kmax=k, levels=1, result_vertices=int(member.sum()),
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


def _check(hb, S, A=None, k=None, name="", want=None, v=None):
    """coreness (k None) or kcore(k) on S's graph against the reference, exactly; -> (values, record)"""
    g = hb.g
    n = S.shape[0]
    if A is None:
        A = _matrix(g, S)
    if want is None:
        want = _ref(S)
    if k is None:
        vals, rec = want[0], want[1]
    else:
        vals, rec = _ref_kcore(S, want[0], k)
    if v is None:
        v = g.Vector(n, I)
    info, res = g.coreness(v, A, None) if k is None else g.kcore(v, A, k, None)
    assert info == 0, (name, info)
    got = _values(g, v, n)
    print(name, k, {x: res[x] for x in REC}, rec, "rounds", res["rounds"], "loop_ms", res["loop_ms"])
    bad = np.flatnonzero(got != vals)
    assert bad.size == 0, (name, k, bad.size, bad[:10], got[bad[:10]], vals[bad[:10]])
    for x in REC:
        assert res[x] == rec[x], (name, k, x, res, rec)
    assert res["loop_ms"] >= 0 and res["rounds"] >= 1
    return got, res


def _closed(hb, S, core, name, **rec):
    """a graph whose core numbers are a formula: the device against the formula, and the reference against it too"""
    core = np.asarray(core, I)
    want = _ref(S)
    assert np.array_equal(want[0], core), name
    for x, y in rec.items():
        assert want[1][x] == y, (name, x, want[1], y)
    return _check(hb, S, name=name, want=want)


def _complete(m):
    r, c = np.triu_indices(m, 1)
    return _sym(m, r, c)


def _path(n, first=0):
    a = first + np.arange(n - 1)
    return a, a + 1


def _rmat(scale, seed):
    from graphblast_amd.graphgen import rmat_edges
    s, d, n = rmat_edges(scale, 16, seed=seed)
    return _sym(n, np.asarray(s), np.asarray(d))


# ---- the reference itself ----------------------------------------------------------------------------------------------
def test_reference_agrees_with_the_heap_peel():
    rng = np.random.default_rng(1)
    n = 1024
    S = _sym(n, np.concatenate([rng.integers(0, n, 5000), rng.integers(0, 40, 1500)]),
             np.concatenate([rng.integers(0, n, 5000), rng.integers(0, 40, 1500)]), rng.integers(0, n, 100))
    core, _, levels = _peel(S)
    assert np.array_equal(core, _heap_peel(S)) and core.max() > 8 and levels == np.unique(core).size


# ---- random graphs -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1000, 4097])
def test_random_undirected(hb, dt, n):
    """isolated vertices, stored diagonals, a denser corner, values that must not matter"""
    rng = np.random.default_rng(10 + n)
    m = max(1, n - n // 20)                                   # the last twentieth stays isolated
    h = max(1, m // 10)
    S = _sym(n, np.concatenate([rng.integers(0, m, 4 * n), rng.integers(0, h, 3 * n)]),
             np.concatenate([rng.integers(0, m, 4 * n), rng.integers(0, h, 3 * n)]), rng.integers(0, n, 1 + n // 10))
    assert S.diagonal().sum() > 0
    _check(hb, S, _matrix(hb.g, S, dt, rng), name=("random", dt.__name__, n))


@pytest.fixture(scope="module")
def rmats():
    out = {}
    for scale in (12, 14):
        S = _rmat(scale, 3 + scale)
        out[scale] = (S, _ref(S))
    return out


@pytest.mark.parametrize("scale", [12, 14])
def test_rmat(hb, rmats, scale):
    S, want = rmats[scale]
    assert want[1]["kmax"] > 20 and want[1]["levels"] < want[1]["kmax"]      # levels are skipped
    _check(hb, S, _matrix(hb.g, S, I, np.random.default_rng(scale)), name=("rmat", scale), want=want)


@pytest.mark.parametrize("which", ["rmat12", "random"])
def test_kcore_at_every_k(hb, rmats, which):
    """k in {0, 1, 2, kmax - 1, kmax, kmax + 1}: the degrees inside the k-core, v > 0 <=> core >= max(k, 1), and result_edges
    = half the sum of v"""
    if which == "rmat12":
        S, want = rmats[12]
    else:
        rng = np.random.default_rng(21)
        n = 3000
        S = _sym(n, np.concatenate([rng.integers(0, n, 9000), rng.integers(0, 60, 2500)]),
                 np.concatenate([rng.integers(0, n, 9000), rng.integers(0, 60, 2500)]), rng.integers(0, n, 200))
        want = _ref(S)
    A = _matrix(hb.g, S, F, np.random.default_rng(22))
    core, kmax = want[0], want[1]["kmax"]
    assert kmax >= 4
    for k in (0, 1, 2, kmax - 1, kmax, kmax + 1):
        got, res = _check(hb, S, A, k=k, name=which, want=want)
        assert np.array_equal(got > 0, core >= max(k, 1))
        assert res["result_edges"] * 2 == int(got.astype(np.int64).sum())
        if k == 0:
            assert np.array_equal(got, np.diff(_graph(S)[0]))
        if k == kmax + 1:
            assert res["result_vertices"] == 0 and not got.any()


# ---- closed forms ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [2, 64, 65, 300, 2049])
def test_complete_graph(hb, m):
    """K_m: core m - 1.  All m vertices are the first frontier of the level m - 1, and every one of the m (m - 1) entries
    they walk meets a vertex at the level's own degree, which must not be taken below it; rows of 1, 63, 64, 299 and
    WAVE_LEN entries"""
    _closed(hb, _complete(m), np.full(m, m - 1), ("K", m), kmax=m - 1, levels=1, result_vertices=m, result_edges=m * (m - 1) // 2)


@pytest.mark.parametrize("a, b", [(3, 500), (70, 90), (300, 2100)])
def test_complete_bipartite(hb, a, b):
    """K_{a,b}: min(a, b).  The b vertices of degree a go first; each of the a others takes b decrements in one round, the
    first b - a of them real, the one that reaches the level appends, the rest are undone or skipped"""
    r = np.repeat(np.arange(a), b)
    c = a + np.tile(np.arange(b), a)
    _closed(hb, _sym(a + b, r, c), np.full(a + b, min(a, b)), ("K", a, b), kmax=min(a, b), levels=1, result_edges=a * b)


def test_cycle_is_one_frontier(hb):
    """a cycle of GRID x THREADS + 1 vertices: the whole graph is the first frontier of level 2, one vertex more than the
    launch has threads"""
    n = _grid(hb) * THREADS + 1
    a = np.arange(n)
    _closed(hb, _sym(n, a, (a + 1) % n), np.full(n, 2), "cycle", kmax=2, levels=1, result_vertices=n, result_edges=n)


def test_grid_is_two(hb):
    side = 70
    idx = np.arange(side * side).reshape(side, side)
    r = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
    c = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    _closed(hb, _sym(side * side, r, c), np.full(side * side, 2), "grid", kmax=2, levels=1)


def test_hypercube(hb):
    n = 1 << 10
    a = np.arange(n)
    r = np.concatenate([a for _ in range(10)])
    c = np.concatenate([a ^ (1 << b) for b in range(10)])
    _closed(hb, _sym(n, r, c), np.full(n, 10), "Q10", kmax=10, levels=1, result_vertices=n)


def test_random_tree_is_one(hb):
    rng = np.random.default_rng(30)
    n = 20000
    child = np.arange(1, n)
    parent = (rng.random(n - 1) * child).astype(np.int64)     # below the child
    _closed(hb, _sym(n, child, parent), np.ones(n), "tree", kmax=1, levels=1, result_vertices=n, result_edges=n - 1)


def test_star(hb):
    """200 000 leaves: 1 everywhere; the centre is hit 200 000 times in one round and the first frontier is far past a
    wave's staging buffer"""
    n = 200001
    _closed(hb, _sym(n, np.zeros(n - 1, np.int64), np.arange(1, n)), np.ones(n), "star", kmax=1, levels=1, result_vertices=n)


# ---- many rounds; many and skipped levels ------------------------------------------------------------------------------
def test_paths_rounds_and_launches(hb):
    """a path of 4000 vertices takes 2000 synchronous rounds, a path of 40 takes 20: the same launches"""
    out = {}
    for n in (40, 4000):
        S = _sym(n, *_path(n))
        want = _ref(S)
        assert want[2] == n // 2
        _, res = _closed(hb, S, np.ones(n), ("path", n), kmax=1, levels=1, result_vertices=n, result_edges=n - 1)
        out[n] = res
    assert out[40]["launches"] == out[4000]["launches"] == LAUNCHES
    assert out[4000]["rounds"] > out[40]["rounds"]


def test_chain_of_cliques(hb):
    """K_2 - K_3 - ... - K_120 joined by single bridges: a level for nearly every k up to 119"""
    r, c, core = [], [], []
    first = 0
    for m in range(2, 121):
        a, b = np.triu_indices(m, 1)
        r.append(first + a)
        c.append(first + b)
        if first:
            r.append(np.array([first - 1]))
            c.append(np.array([first]))
        core += [m - 1] * m
        first += m
    S = _sym(first, np.concatenate(r), np.concatenate(c))
    _, res = _closed(hb, S, core, "chain", kmax=119, result_vertices=120)
    assert res["levels"] >= 118


def test_skipped_levels(hb):
    """K_300 beside 500 isolated vertices and a path: the levels 0, 1 and 299"""
    r, c = np.triu_indices(300, 1)
    pr, pc = _path(700, 800)
    n = 1500
    core = np.zeros(n, I)
    core[:300] = 299
    core[800:] = 1
    _closed(hb, _sym(n, np.concatenate([r, pr]), np.concatenate([c, pc])), core, "skipped", kmax=299, levels=3, result_vertices=300)


# ---- the row-length classes --------------------------------------------------------------------------------------------
def _hub(r, c, nxt, length, stay):
    """a vertex x whose row has `length` entries: length - 2 leaves (gone after level 1), p and q.  q is one of `stay` (a
    K_5: its degree stays above the level); p is joined to x and to two more of the K_5, so x takes it from 3 to the
    level 2 and appends it.  -> x, p, the next free id"""
    x, p = nxt, nxt + 1
    leaves = nxt + 2 + np.arange(length - 2)
    r += [np.full(length - 2, x), [x, x, p, p]]
    c += [leaves, [p, stay[0], stay[1], stay[2]]]
    return x, p, nxt + length


@pytest.mark.parametrize("density", ["a vertex a wave", "two a wave", "64 a wave"])
def test_row_length_classes(hb, density):
    """level 2's first frontier holds one vertex of every class at every boundary -- rows of LANE_LEN - 1 .. + 1 and
    WAVE_LEN - 1 .. + 1 entries -- each with neighbours that are gone, one that falls to the level and one that stays above
    it; beside them enough triangles that a wave of the round holds one, two or 64 frontier vertices"""
    waves = _grid(hb) * WAVES
    triangles = {"a vertex a wave": 0, "two a wave": waves // 3 + 10, "64 a wave": (64 * waves) // 3 + 10}[density]
    r, c = [a for a in np.triu_indices(5, 1)]
    r, c = [r], [c]
    nxt = 5
    hubs = []
    for length in (LANE_LEN - 1, LANE_LEN, LANE_LEN + 1, WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1, 3 * WAVE_LEN + 5):
        x, p, nxt = _hub(r, c, nxt, length, (0, 1, 2))
        hubs.append((x, p, length))
    t = nxt + 3 * np.arange(triangles)
    r += [t, t, t + 1]
    c += [t + 1, t + 2, t + 2]
    n = nxt + 3 * triangles
    perm = np.random.default_rng(40).permutation(n)          # the hubs anywhere among the others
    S = _sym(n, perm[np.concatenate(r)], perm[np.concatenate(c)])
    want = _ref(S)
    core = want[0]
    for x, p, length in hubs:
        assert S.indptr[perm[x] + 1] - S.indptr[perm[x]] == length and core[perm[x]] == 2 and core[perm[p]] == 2
    assert (core[perm[:5]] == 4).all() and want[1]["levels"] == 3
    front = 7 + 3 * triangles                                # level 2's first frontier
    per = 64 if front >= 64 * waves else -(-front // waves)
    assert per == {"a vertex a wave": 1, "two a wave": 2, "64 a wave": 64}[density]
    _check(hb, S, name=("classes", density), want=want)
    _check(hb, S, k=2, name=("classes", density), want=want)
    _check(hb, S, k=3, name=("classes", density), want=want)


@pytest.mark.parametrize("leaves", [100, WAVE_LEN + 50])
def test_one_row_appends_more_than_a_stage(hb, leaves):
    """x: `leaves` leaves and 300 neighbours u, each joined to x and to 300 vertices of a K_700.  When x goes at level 300
    every u falls from 301 to the level: 300 appends out of one row -- a wave's (row of 400 entries) or a workgroup's --
    with consecutive ids, so one wave stages more than STAGE - 64 of them"""
    rng = np.random.default_rng(41)
    kr, kc = np.triu_indices(700, 1)
    x = 700
    u = 701 + np.arange(300)
    lv = 1001 + np.arange(leaves)
    ur = np.repeat(u, 300)
    uc = np.concatenate([rng.choice(700, 300, replace=False) for _ in range(300)])
    n = 1001 + leaves
    S = _sym(n, np.concatenate([kr, np.full(300, x), np.full(leaves, x), ur]), np.concatenate([kc, u, lv, uc]))
    want = _ref(S)
    assert 300 > STAGE - 64 and want[0][x] == 300 and (want[0][u] == 300).all() and (want[0][lv] == 1).all() and want[0][:700].min() >= 699
    _check(hb, S, name=("appends", leaves), want=want)


# ---- the library's own trussness ---------------------------------------------------------------------------------------
def test_trussness_bounds_the_core(hb, rmats):
    """both ends of an edge of trussness t have t - 2 common neighbours inside the t-truss: core >= t - 1"""
    g = hb.g
    S, want = rmats[12]
    A = _matrix(g, S, I)
    core, _ = _check(hb, S, A, name="rmat12", want=want)
    T = g.Matrix(S.shape[0], S.shape[0], I)
    info, tres = g.trussness(T, A, hb.descriptor())
    assert info == 0
    tp, ti, tv = T.host_csr()
    rows = np.repeat(np.arange(S.shape[0]), np.diff(tp))
    assert tv.size == S.nnz and tv.max() == tres["kmax"] > 3
    assert (core[rows] >= tv - 1).all() and (core[ti] >= tv - 1).all()
    assert want[1]["kmax"] >= tres["kmax"] - 1


# ---- a golden graph ----------------------------------------------------------------------------------------------------
def test_golden_chesapeake(hb):
    M = sp.csr_matrix(scipy.io.mmread(os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")))
    co = M.tocoo()
    S = _sym(M.shape[0], co.row, co.col)
    want = _ref(S)
    assert want[1]["edges"] == 170 and np.array_equal(want[0], _heap_peel(S))
    _check(hb, S, name="chesapeake", want=want)
    A = hb.matrix_from_mtx("chesapeake.mtx")                # symmetrised as the loader does
    _check(hb, S, A, name="chesapeake, loaded", want=want)
    _check(hb, S, A, k=want[1]["kmax"], name="chesapeake, loaded", want=want)


# ---- matrices without a CSC of their own -------------------------------------------------------------------------------
def test_product_result_and_csr_only_format(hb, monkeypatch):
    """only the CSR is read: both calls work on C = A A of a symmetric A (symmetric again, no CSC of its own) and on a matrix
    of the CSR-only format.  An asymmetric product is taken on the caller's word: the call succeeds and stays in bounds"""
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
    want = _ref(SP)
    _check(hb, SP, P, name="product", want=want)
    _check(hb, SP, P, k=3, name="product", want=want)
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Q = _matrix(g, S, I)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    want = _ref(S)
    _check(hb, S, Q, name="CSR only", want=want)
    _check(hb, S, Q, k=2, name="CSR only", want=want)
    D = _pattern(n, rng.integers(0, n, 1500), rng.integers(0, n, 1500))
    Dm = _matrix(g, D, F)
    PD = g.Matrix(n, n, F)
    assert g.mxm(PD, None, None, "PlusMultiplies", Dm, Dm, hb.descriptor()) == 0
    v = g.Vector(n, I)
    for call in (lambda: g.coreness(v, PD, None), lambda: g.kcore(v, PD, 2, None)):
        info, _ = call()
        assert info == 0 and v.getStorage() == g.GrB_DENSE and v.nvals() == n


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_the_output_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(13)
    n = 80
    S = _sym(n, rng.integers(0, n, 300), rng.integers(0, n, 300))
    A = _matrix(g, S, F, rng)
    before = rng.integers(5, 1000, n).astype(I)
    v = g.Vector(n, I)
    assert v.build(before, n) == 0

    def unchanged():
        return v.getStorage() == g.GrB_DENSE and np.array_equal(v.extractTuples()[1], before)

    calls = (lambda v_, A_: lib.grb_coreness(v_, A_, None, None), lambda v_, A_: lib.grb_kcore(v_, A_, 2, None, None))
    R = g.Matrix(n, n + 1, F)                                                         # A not square
    assert R.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)) == 0
    fv = g.Vector(n, F)                                                               # an output that is not i32
    fbefore = rng.random(n).astype(F) + 2
    assert fv.build(fbefore, n) == 0
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                          # an A of element type code 2
    hp, hi, hv = S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)
    assert lib.grb_matrix_build_csr(h, hp.ctypes.data, hi.ctypes.data, hv.ctypes.data, S.nnz, None, None, None) == 0
    D = _pattern(n, rng.integers(0, n, 300), rng.integers(0, n, 300))                 # an asymmetric A with its own CSC
    assert (D != D.T).nnz > 0
    Dm = _matrix(g, D, F)
    sv = g.Vector(n, I)                                                               # a sparse output stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0
    for call in calls:
        assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                          # null handles
        assert call(v._h, None) == g.GrB_UNINITIALIZED_OBJECT
        assert call(v._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT         # an unbuilt A
        assert call(v._h, R._h) == g.GrB_DIMENSION_MISMATCH
        assert call(g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH          # size(output) != n
        assert unchanged()
        assert call(fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
        assert np.array_equal(fv.extractTuples()[1].view(np.uint32), fbefore.view(np.uint32))
        assert call(v._h, h) == g.GrB_NOT_IMPLEMENTED
        assert unchanged()
        assert call(v._h, Dm._h) == g.GrB_INVALID_VALUE
        assert unchanged()
        assert call(sv._h, Dm._h) == g.GrB_INVALID_VALUE
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
        info, si, sx = sv.extractTuples(sparse=True)
        assert info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]
    for k in (-1, -2 ** 31):                                                          # k < 0
        assert lib.grb_kcore(v._h, A._h, k, None, None) == g.GrB_INVALID_VALUE
    assert lib.grb_kcore(fv._h, A._h, -1, None, None) == g.GrB_INVALID_VALUE          # ... is found before the types
    assert lib.grb_kcore(v._h, R._h, -1, None, None) == g.GrB_DIMENSION_MISMATCH      # ... and after the shapes
    assert unchanged()
    assert lib.grb_matrix_free(h) == 0
    # a descriptor and a null descriptor give the same result; the record is optional
    w = g.Vector(n, I)
    assert lib.grb_coreness(w._h, A._h, hb.descriptor()._h, None) == 0
    assert lib.grb_coreness(v._h, A._h, None, None) == 0 and not unchanged()
    assert np.array_equal(v.extractTuples()[1], w.extractTuples()[1]) and np.array_equal(w.extractTuples()[1], _ref(S)[0])
    assert lib.grb_kcore(w._h, A._h, 2, hb.descriptor()._h, None) == 0
    assert np.array_equal(w.extractTuples()[1], _ref_kcore(S, _ref(S)[0], 2)[0])


# ---- degenerate shapes, the output's storage beforehand ----------------------------------------------------------------
def test_degenerate(hb):
    g = hb.g
    for n, S in ((1, _sym(1, [], [])), (1, _sym(1, [], [], [0])), (50, _sym(50, [], [])), (50, _sym(50, [], [], np.arange(0, 50, 3)))):
        want = (np.zeros(n, I), dict(edges=0, result_edges=0, kmax=0, levels=1, result_vertices=n, launches=LAUNCHES), 1)
        assert np.array_equal(_ref(S)[0], want[0]) and _ref(S)[1] == want[1]
        _check(hb, S, name=("degenerate", n), want=want)
        for k in (0, 1):
            _, res = _check(hb, S, k=k, name=("degenerate", n), want=want)
            assert res["result_vertices"] == (n if k == 0 else 0)
    S = _sym(300, [3, 5, 3, 7], [5, 7, 7, 200])               # one triangle among 300 vertices, and one pendant edge
    got, res = _check(hb, S, name="one triangle")
    assert res["kmax"] == 2 and res["levels"] == 3 and got[3] == 2 and got[200] == 1 and got[0] == 0
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    v0 = g.Vector(0, I)
    info, res = g.coreness(v0, A0, None)
    assert info == 0 and all(res[x] == 0 for x in REC)
    info, res = g.kcore(v0, A0, 3, None)
    assert info == 0 and res["kmax"] == 3 and res["levels"] == 1 and res["result_vertices"] == 0 and res["edges"] == 0


def test_more_isolated_vertices_than_four_a_thread(hb):
    """level 0 lists 4 GRID x THREADS + 3 vertices but a triangle: every wave of the scan stages 256 of them, more than it
    holds before it reserves room"""
    n = 4 * _grid(hb) * THREADS + 6
    S = _sym(n, [n - 3, n - 3, n - 2], [n - 2, n - 1, n - 1])
    core = np.zeros(n, I)
    core[n - 3:] = 2
    want = (core, dict(edges=3, result_edges=3, kmax=2, levels=2, result_vertices=3, launches=LAUNCHES), 2)
    _check(hb, S, name="isolated", want=want)


def test_output_sparse_dense_or_empty_beforehand(hb):
    g = hb.g
    rng = np.random.default_rng(14)
    n = 400
    S = _sym(n, rng.integers(0, n, 3000), rng.integers(0, n, 3000))
    A = _matrix(g, S, F)
    want = _ref(S)
    for k in (None, 3):
        dense = g.Vector(n, I)
        assert dense.build(np.full(n, 9, I), n) == 0
        sparse = g.Vector(n, I)
        assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
        for name, v in (("dense", dense), ("sparse", sparse), ("fresh", g.Vector(n, I))):
            _check(hb, S, A, k=k, name=name, want=want, v=v)


def test_output_on_caller_owned_storage(hb):
    """the output adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(15)
    n = 1003
    S = _sym(n, rng.integers(0, n, 9000), rng.integers(0, n, 9000))
    A = _matrix(g, S, F)
    want = _ref(S)
    for k in ad.KS:
        for kk in (None, 4):
            v, t, check = ad.adopt_dense(g, np.full(n, 77, I), k)
            assert v.device_ptrs()[2] % 16 == 4 * k
            got, _ = _check(hb, S, A, k=kk, name=("adopted", k), want=want, v=v)
            assert np.array_equal(ad.payload(t, k, n, I), got)
            check(("kcore", k, kk))


# ---- determinism, relabelling ------------------------------------------------------------------------------------------
def test_determinism_and_relabelling(hb):
    g = hb.g
    S = _rmat(13, 6)
    n = S.shape[0]
    want = _ref(S)
    A = _matrix(g, S, F)
    kk = want[1]["kmax"] // 2
    outs = []
    for _ in range(2):
        got, res = _check(hb, S, A, name="rmat13", want=want)
        got2, res2 = _check(hb, S, A, k=kk, name="rmat13", want=want)
        outs.append((got.tobytes(), got2.tobytes(), [res[x] for x in REC], [res2[x] for x in REC]))
    assert outs[0] == outs[1]
    perm = np.random.default_rng(16).permutation(n)         # vertex v becomes perm[v]
    co = S.tocoo()
    Sp = _pattern(n, perm[co.row], perm[co.col])
    gotp, resp = _check(hb, Sp, name="relabelled")
    assert np.array_equal(gotp[perm], got) and [resp[x] for x in REC] == outs[0][2]
    gotp2, resp2 = _check(hb, Sp, k=kk, name="relabelled")
    assert np.array_equal(gotp2[perm], got2) and [resp2[x] for x in REC] == outs[0][3]


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def test_cpp_frontend(tmp_path):
    """tests/tools/kcore.cpp: two triangles, a bridge and a pendant vertex; a K5 with a tail; a NULL descriptor.  It checks
    its own expected values"""
    exe = str(tmp_path / "kcore")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "kcore.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    assert lines[-1] == "ok" and "bridge core 2 2 2 2 2 2 1 0" in lines and "k5 core 4 4 4 4 4 1 1 1" in lines
    S = _sym(8, [0, 0, 1, 3, 3, 4, 2, 5], [1, 2, 2, 4, 5, 5, 3, 6])
    assert _ref(S)[0].tolist() == [2, 2, 2, 2, 2, 2, 1, 0] and _ref_kcore(S, _ref(S)[0], 2)[0].tolist() == [2, 2, 3, 3, 2, 2, 0, 0]
