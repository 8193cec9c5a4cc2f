"""Betweenness centrality on the device (csrc/bc.hip: batched Brandes, 64 sources per sweep) against a scipy restatement
of the definition in include/grb_hip.h: level-synchronous on dense n x B f64 arrays, St @ F forwards and S @ W backwards,
masked by depth.

Tolerance (derived, not measured): every quantity is a sum, product or quotient of non-negative f64 numbers, so two
evaluation orders differ by far less than 2^-24 relative at these sizes; after the single rounding to f32 they can differ by
one f32 ulp.  Asserted: |got - f32(ref)| <= 2^-22 * f32(ref) elementwise (two ulps: one for the rounding boundary, one of
margin), exactly 0 wherever the reference is exactly 0, and exact equality where the reference is integer-valued and
representable (trees, closed forms).

The fixture, random directed graphs in both element types with values that must not matter, source counts across the batch
edges, unreachable parts, path counts beyond f32, high diameter, closed forms, rows and level lists around every constant of
the kernels, runs of empty rows, degenerate sizes, identities through the library, determinism, every error code with bc
unchanged, and the C++ frontend."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp

from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# csrc/bc.hip
BATCH = 64           # kBcBatch: sources of one sweep, a lane each
UNROLL = 4           # kBcUnroll: neighbour rows a wave keeps in flight: a wave's share of a workgroup step
STEP = 16            # kBcUnroll x the 4 waves of a workgroup: the neighbours of one step; a longer row takes several
LONG = 256           # kBcLong: a row longer than this is walked 16 neighbours a wave, 64 a workgroup, per step (LONG_STEP)
LONG_STEP = 64
GRID = 2048          # kBcGrid: workgroups of a level's launch; a longer level list is walked grid-stride
CHUNK = 8            # kBcChunk: levels of the sweep between two host reads of the list offsets


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs and the reference ------------------------------------------------------------------------------------------
def _dir(n, r, c):
    """the directed graph of the draws (r, c): edge r -> c, loops dropped, no duplicates; int64 ones"""
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    keep = r != c
    S = sp.csr_matrix((np.ones(int(keep.sum()), np.int64), (r[keep], c[keep])), shape=(n, n))
    S.data[:] = 1
    S.sort_indices()
    return S


def _sym(n, r, c):
    r, c = np.asarray(r, np.int64), np.asarray(c, np.int64)
    return _dir(n, np.concatenate([r, c]), np.concatenate([c, r]))


def _ref(S, sources):
    """-> (bc in f64, vertices reached summed over the sources, largest depth + 1, the depths as an n x len(sources)
    array, -1 where unreached).  S: a 0 / 1 pattern without a diagonal, S[i, j] = the edge i -> j."""
    n = S.shape[0]
    S = sp.csr_matrix(S, dtype=np.float64)
    St = sp.csr_matrix(S.T)
    sources = np.arange(n) if sources is None else np.asarray(sources, np.int64)
    bc = np.zeros(n)
    reached, levels, depths = 0, 0, []
    for b0 in range(0, sources.size, BATCH):
        src = sources[b0:b0 + BATCH]
        B = src.size
        col = np.arange(B)
        depth = np.full((n, B), -1, np.int64)
        sigma = np.zeros((n, B))
        depth[src, col] = 0
        sigma[src, col] = 1.0
        d = 0
        while True:
            d += 1
            N = St @ (sigma * (depth == d - 1))          # N[w, s] = the paths that arrive at w from depth d - 1
            new = (N > 0) & (depth < 0)
            if not new.any():
                break
            depth[new] = d
            sigma[new] = N[new]
        last = d - 1
        delta = np.zeros((n, B))
        for d in range(last - 1, -1, -1):
            W = np.zeros((n, B))
            m = depth == d + 1
            W[m] = (1.0 + delta[m]) / sigma[m]
            G = S @ W                                    # G[v, s] = the sum over v's children
            m = depth == d
            delta[m] = (sigma * G)[m]
        delta[src, col] = 0.0
        bc += delta.sum(axis=1)
        reached += int((depth >= 0).sum())
        levels = max(levels, last + 1)
        depths.append(depth)
    return bc, reached, levels, np.concatenate(depths, axis=1)


def _matrix(g, S, dt=F, rng=None, diag=None):
    """A with S's structure; values that must not matter (zeros and negatives among them); diag: rows that also store
    their diagonal entry"""
    n = S.shape[0]
    P = S
    if diag is not None:
        P = sp.csr_matrix(S + sp.csr_matrix((np.ones(len(diag), np.int64), (diag, diag)), shape=(n, n)))
        P.sort_indices()
    vals = np.ones(P.nnz, dt) if rng is None else rng.integers(-3, 4, P.nnz).astype(dt)
    A = g.Matrix(n, n, dt)
    assert A.build_csr(P.indptr.astype(I), P.indices.astype(I), vals) == 0
    return A


def _bc(g, A, n, sources, desc=None):
    v = g.Vector(n, F)
    info, res = g.bc(v, A, sources, desc)
    assert info == 0, info
    i2, vals = v.extractTuples()
    assert i2 == 0 and vals.dtype == F and vals.size == n
    return vals, res


def _close(got, ref, name=""):
    want = ref.astype(F).astype(np.float64)
    assert np.all(np.isfinite(got)), name
    err = np.abs(got.astype(np.float64) - want)
    rel = float((err[want > 0] / want[want > 0]).max()) if (want > 0).any() else 0.0
    print(name, "largest relative difference to f32(ref): %.3g" % rel)
    assert np.all(got[ref == 0] == 0), (name, "exact zeros")
    assert np.all(err <= 2.0 ** -22 * want), (name, rel)


def _exact(got, ref, name=""):
    assert np.array_equal(ref, np.round(ref)) and np.array_equal(ref.astype(F).astype(np.float64), ref), name
    assert np.array_equal(got, ref.astype(F)), name


def _check(hb, S, sources, dt=F, rng=None, diag=None, name="", ref=None, exact=False):
    g = hb.g
    n = S.shape[0]
    want, reached, levels, _ = _ref(S, sources) if ref is None else ref
    got, res = _bc(g, _matrix(g, S, dt, rng, diag), n, sources)
    _close(got, want, name)
    if exact:
        _exact(got, want, name)
    ns = n if sources is None else len(sources)
    assert res["sources"] == ns and res["batches"] == (ns + BATCH - 1) // BATCH, (name, res)
    assert res["reached"] == reached and res["levels"] == levels, (name, res, reached, levels)
    return got, res


# ---- the fixture -------------------------------------------------------------------------------------------------------
def _fixture():
    with open(os.path.join(ROOT, "tests", "golden", "data", "test_bc.mtx")) as f:
        rows = [[int(x) for x in ln.split()] for ln in f if ln.strip() and not ln.startswith("%")]
    assert rows[0] == [7, 7, 15]
    e = np.array(rows[1:], np.int64)
    return _dir(7, e[:, 0] - 1, e[:, 1] - 1)                # the entry "r c" is the edge r - 1 -> c - 1


FIXTURE_BC = np.array([0.5, 0.5, 3.0, 11.0 / 6.0, 11.0 / 6.0, 1.0 / 3.0, 0.0])


def test_fixture(hb):
    S = _fixture()
    assert S.nnz == 15
    want = _ref(S, None)
    assert np.allclose(want[0], FIXTURE_BC, rtol=1e-14, atol=0)
    got, _ = _check(hb, S, None, name="fixture", ref=want)
    _close(got, FIXTURE_BC, "fixture, the stated values")
    got2, _ = _check(hb, S, list(range(7)), I, np.random.default_rng(1), name="fixture, explicit list", ref=want)
    assert got.tobytes() == got2.tobytes()
    _check(hb, _dir(7, S.nonzero()[1], S.nonzero()[0]), None, name="fixture transposed")


# ---- random directed graphs --------------------------------------------------------------------------------------------
_cache = {}


def _random_graph(n, draws):
    if (n, draws) not in _cache:
        rng = np.random.default_rng(7)
        S = _dir(n, rng.integers(0, n, draws), rng.integers(0, n, draws))
        diag = np.sort(rng.choice(n, n // 10, replace=False))
        lists = {}
        for ns in (1, 63, 64, 65, 130):
            lists[ns] = rng.choice(n, ns, replace=False)
        dup = rng.choice(n, 40, replace=False)
        lists["dup"] = np.concatenate([dup, dup[:30], dup[:5]])      # 75 sources, 40 distinct: duplicates across a batch edge
        if n <= 300:
            lists["all"] = None
        _cache[(n, draws)] = (S, diag, lists, {})
    return _cache[(n, draws)]


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("n, draws", [(300, 3000), (2000, 30000)])
def test_random_directed_graphs(hb, dt, n, draws):
    """A's values include zeros and negatives; a tenth of the rows store their diagonal entry; 1, 63, 64, 65 and 130 sources
    cross the batch edges and leave a ragged last batch; one list has duplicates; all sources on the small graph"""
    S, diag, lists, refs = _random_graph(n, draws)
    assert (S != S.T).nnz > 0
    rng = np.random.default_rng(8)
    for key, src in lists.items():
        if key not in refs:
            refs[key] = _ref(S, src)
        got, res = _check(hb, S, src, dt, rng, diag, (n, draws, key), ref=refs[key])
        assert got.max() > 0 or key == 1


# ---- unreachable parts -------------------------------------------------------------------------------------------------
def test_unreachable_parts(hb):
    """two components, isolated vertices, sources that are isolated, sources that are sinks, a source whose component is a
    single edge"""
    rng = np.random.default_rng(9)
    a, b = 150, 90                                       # component sizes; then 20 isolated vertices, then one edge
    r = np.concatenate([rng.integers(0, a, 900), a + rng.integers(0, b, 400), [a + b + 20]])
    c = np.concatenate([rng.integers(0, a, 900), a + rng.integers(0, b, 400), [a + b + 21]])
    n = a + b + 22
    keep = r % 17 != 3                                   # sinks: vertices without out-edges
    S = _dir(n, r[keep], c[keep])
    outdeg, indeg = np.diff(S.indptr), np.diff(S.T.tocsr().indptr)
    sinks = np.flatnonzero((outdeg == 0) & (indeg > 0))
    isolated = np.flatnonzero((outdeg == 0) & (indeg == 0))
    assert sinks.size >= 3 and isolated.size >= 20
    src = np.concatenate([[0, 5, a + 1, a + 7], sinks[:3], isolated[:3], [a + b + 20, a + b + 21]])
    want = _ref(S, src)
    assert want[1] < src.size * n
    _check(hb, S, src, F, rng, None, "unreachable", ref=want)
    _check(hb, S, None, I, rng, None, "unreachable, all sources")
    got, res = _check(hb, S, isolated[:2], name="isolated sources only")
    assert not got.any() and res["reached"] == 2 and res["levels"] == 1


# ---- path counts beyond f32 --------------------------------------------------------------------------------------------
def _grid(side):
    idx = np.arange(side * side).reshape(side, side)
    return _sym(side * side, np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]),
                np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))


def test_path_counts_beyond_f32(hb):
    """a 72 x 72 grid from a corner: the largest path count is C(142, 71) = 3.7e41, above f32's 3.4e38"""
    S = _grid(72)
    n = S.shape[0]
    St = sp.csr_matrix(S.T, dtype=np.float64)
    depth = np.add.outer(np.arange(72), np.arange(72)).ravel()
    sigma = np.zeros(n)
    sigma[0] = 1.0
    for d in range(1, 143):
        sigma[depth == d] = (St @ (sigma * (depth == d - 1)))[depth == d]
    assert 3.6e41 < sigma.max() < 3.8e41 and sigma.max() > float(np.finfo(F).max)
    want = _ref(S, [0])
    assert abs(want[0].max() - 2590.5) < 1e-6
    got, res = _check(hb, S, [0], name="grid 72", ref=want)
    assert np.all(np.isfinite(got)) and res["levels"] == 143


# ---- high diameter -----------------------------------------------------------------------------------------------------
def test_undirected_path_all_sources(hb):
    n = 3000
    S = _sym(n, np.arange(n - 1), np.arange(1, n))
    i = np.arange(n, dtype=np.float64)
    want = 2.0 * i * (n - 1 - i)
    got, res = _bc(hb.g, _matrix(hb.g, S), n, None)
    _exact(got, want, "path")
    assert res["levels"] == n and res["reached"] == n * n and res["batches"] == (n + BATCH - 1) // BATCH


def test_path_few_sources_and_directed_path(hb):
    n = 3000
    S = _sym(n, np.arange(n - 1), np.arange(1, n))
    _check(hb, S, [0, n - 1, n // 2], name="path ends and middle", exact=True)
    D = _dir(n, np.arange(n - 1), np.arange(1, n))
    got, res = _check(hb, D, [n - 1], name="directed path from its tail", exact=True)
    assert not got.any() and res["reached"] == 1 and res["levels"] == 1
    got, res = _check(hb, D, [0, 10], name="directed path", exact=True)
    assert got[1] == n - 2 and got[11] == 2 * (n - 12) and res["levels"] == n


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, CHUNK + 2, 2 * CHUNK, 2 * CHUNK + 1, 2 * CHUNK + 2])
def test_depths_around_the_host_reads(hb, n):
    """a path whose last level is one below, at and one above the levels the sweep launches between two host reads"""
    S = _sym(n, np.arange(n - 1), np.arange(1, n))
    got, res = _check(hb, S, [0], name=("chunk", n), exact=True)
    assert res["levels"] == n and np.array_equal(got[1:], np.arange(n - 2, -1, -1))
    _check(hb, S, None, name=("chunk, all", n), exact=True)


# ---- closed forms ------------------------------------------------------------------------------------------------------
def test_star(hb):
    """all sources: the centre lies between every ordered pair of leaves; the hub's row is longer than any threshold"""
    n = 5000
    S = _sym(n, np.zeros(n - 1, np.int64), np.arange(1, n))
    assert S.indptr[1] == n - 1 > GRID
    got, res = _bc(hb.g, _matrix(hb.g, S), n, None)
    want = np.zeros(n)
    want[0] = (n - 1) * (n - 2)
    _exact(got, want, "star")
    assert res["levels"] == 3 and res["reached"] == n * n


def test_complete_graph(hb):
    m = 70
    S = _sym(m, *np.triu_indices(m, 1))
    got, res = _check(hb, S, None, I, name="K70", exact=True)
    assert not got.any() and res["levels"] == 2


def test_complete_binary_tree(hb):
    n = 2 ** 11 - 1                                      # depth 10
    child = np.arange(1, n)
    S = _sym(n, (child - 1) // 2, child)
    got, _ = _check(hb, S, None, name="tree", exact=True)
    assert got[0] == 2 * (2 ** 10 - 1) ** 2 and not got[n // 2:].any()


@pytest.mark.parametrize("n, each", [(101, 100 * 98 / 4.0), (100, 98 * 98 / 4.0)])
def test_cycles(hb, n, each):
    """an even cycle has two shortest paths between opposite vertices: halves on the way"""
    S = _sym(n, np.arange(n), (np.arange(n) + 1) % n)
    want = _ref(S, None)
    assert np.allclose(want[0], each, rtol=1e-13)
    got, _ = _check(hb, S, None, name=("cycle", n), ref=want)
    _close(got, np.full(n, each), ("cycle, closed form", n))


# ---- thresholds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("length", [1, UNROLL - 1, UNROLL, UNROLL + 1, STEP - 1, STEP, STEP + 1, 2 * STEP - 1, 2 * STEP, 2 * STEP + 1,
                                    BATCH - 1, BATCH, BATCH + 1, LONG - 1, LONG, LONG + 1, LONG + LONG_STEP - 1, LONG + LONG_STEP,
                                    LONG + LONG_STEP + 1, LONG + 2 * LONG_STEP + 15, LONG + 2 * LONG_STEP + 17])
def test_row_lengths_around_the_step(hb, length):
    """one vertex with exactly that many in-neighbours and that many out-neighbours over a sparse random directed graph"""
    rng = np.random.default_rng(12)
    n = 600
    hub = 17
    others = np.setdiff1d(np.arange(n), [hub])
    ins, outs = rng.choice(others, length, replace=False), rng.choice(others, length, replace=False)
    r, c = rng.integers(0, n, 3 * n), rng.integers(0, n, 3 * n)
    keep = (r != hub) & (c != hub)
    S = _dir(n, np.concatenate([r[keep], ins, np.full(length, hub)]), np.concatenate([c[keep], np.full(length, hub), outs]))
    assert S.indptr[hub + 1] - S.indptr[hub] == length and np.diff(S.T.tocsr().indptr)[hub] == length
    src = np.concatenate([[hub], rng.choice(n, 70, replace=False)])
    got, _ = _check(hb, S, src, F, rng, None, ("row", length))
    assert got[hub] > 0


@pytest.mark.parametrize("m", [UNROLL - 1, UNROLL, UNROLL + 1, STEP - 1, STEP, STEP + 1, GRID - 1, GRID, GRID + 1, 2 * GRID + 1])
def test_level_lists_around_the_grid(hb, m):
    """a level list of exactly m vertices: 0 -> 1 .. m -> m + 1, and the same with two sources that see the middle at
    different depths (m + 2 -> 0)"""
    n = m + 3
    mid = np.arange(1, m + 1)
    S = _dir(n, np.concatenate([np.zeros(m, np.int64), mid, [m + 2]]), np.concatenate([mid, np.full(m, m + 1), [0]]))
    want = _ref(S, [0])
    assert (want[3][:, 0] == 1).sum() == m
    got, res = _check(hb, S, [0], name=("list", m), ref=want)
    assert res["levels"] == 3 and res["reached"] == m + 2
    _check(hb, S, [0, m + 2, 1], I, name=("list, two depths", m))


def test_runs_of_empty_rows(hb):
    """thousands of empty rows before, between and after the populated ones"""
    rng = np.random.default_rng(13)
    gap, blk = 5000, 40
    r, c, at, src = [], [], gap, []
    for i in range(4):
        r.append(at + rng.integers(0, blk, 160))
        c.append(at + rng.integers(0, blk, 160))
        src += [at, at + 3, at + blk - 1]
        at += blk + (gap if i in (0, 2) else 0)
    n = at + gap
    S = _dir(n, np.concatenate(r), np.concatenate(c))
    got, _ = _check(hb, S, src + [0, n - 1], F, rng, None, "empty rows")
    assert got.max() > 0
    _check(hb, S[:gap + 2 * blk, :gap + 2 * blk], None, I, None, None, "empty rows, all sources")


def test_degenerate(hb):
    """n = 1, n = 2, a matrix with no entries, a matrix with only diagonal entries"""
    for n, S, diag in ((1, _dir(1, [], []), None), (2, _dir(2, [0], [1]), None), (2, _sym(2, [0], [1]), None),
                       (2, _dir(2, [], []), None), (50, _dir(50, [], []), None), (50, _dir(50, [], []), np.arange(0, 50, 3)),
                       (1, _dir(1, [], []), np.array([0]))):
        for src in (None, [0], [n - 1, 0, 0]):
            got, res = _check(hb, S, src, F, None, diag, (n, "degenerate"), exact=True)
            assert not got.any()


# ---- identities through the library ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def graph():
    rng = np.random.default_rng(21)
    n = 500
    S = _dir(n, rng.integers(0, n, 4000), rng.integers(0, n, 4000))
    return S, rng.choice(n, 70, replace=False)


def test_sum_of_single_source_calls(hb, graph):
    g = hb.g
    S, src = graph
    n = S.shape[0]
    A = _matrix(g, S)
    whole, _ = _bc(g, A, n, src)
    total = np.zeros(n)
    for s in src:
        total += _bc(g, A, n, [int(s)])[0].astype(np.float64)
    # every term is within 2^-24 of its own f64 value, so their f64 sum is within 2^-24 of the f64 total; the one call
    # rounds that total once: 2^-23 between the two, inside the tolerance
    err = np.abs(whole.astype(np.float64) - total)
    assert np.all(err <= 2.0 ** -22 * total), float((err / np.maximum(total, 1e-300)).max())
    assert np.all(whole[total == 0] == 0)
    _close(whole, _ref(S, src)[0], "70 sources")


def test_relabelling_permutes_the_result(hb, graph):
    g = hb.g
    S, src = graph
    n = S.shape[0]
    perm = np.random.default_rng(22).permutation(n)      # old -> new
    r, c = S.nonzero()
    S2 = _dir(n, perm[r], perm[c])
    a, _ = _bc(g, _matrix(g, S), n, src)
    b, _ = _bc(g, _matrix(g, S2), n, perm[src])
    want = a.astype(np.float64)
    assert np.all(np.abs(b[perm].astype(np.float64) - want) <= 2.0 ** -22 * want)
    assert np.all(b[perm][a == 0] == 0)


def test_depths_agree_with_bfs_batch(hb, graph):
    g = hb.g
    S, src = graph
    n = S.shape[0]
    src = src[:BATCH]
    A = _matrix(g, S)
    vs = [g.Vector(n, F) for _ in src]
    info, rec = g.bfs_batch(vs, A, src, hb.descriptor())
    assert info == 0
    labels = np.stack([v.extractTuples()[1] for v in vs], axis=1).astype(np.int64)     # depth + 1, 0 where unreached
    _, reached, levels, depth = _ref(S, src)
    assert np.array_equal(labels - 1, depth)
    _, res = _bc(g, A, n, src)
    assert res["reached"] == rec["reached"] == reached == int(np.count_nonzero(labels))
    assert res["levels"] == int(labels.max()) == levels


def test_determinism(hb):
    from graphblast_amd.graphgen import rmat_edges
    g = hb.g
    s, dd, n = rmat_edges(10, 8, seed=5)
    S = _sym(n, np.asarray(s), np.asarray(dd))
    A = _matrix(g, S)
    src = np.random.default_rng(23).choice(n, BATCH, replace=False)
    a, _ = _bc(g, A, n, src)
    b, _ = _bc(g, A, n, src)
    assert a.max() > 0 and a.tobytes() == b.tobytes()
    _close(a, _ref(S, src)[0], "rmat10")


def test_csr_only_format(hb, monkeypatch):
    """GRB_SPARSE_MATRIX_FORMAT=1: the CSC is the CSR; on a symmetric structure the result is the same"""
    g = hb.g
    rng = np.random.default_rng(24)
    n = 400
    S = _sym(n, rng.integers(0, n, 2000), rng.integers(0, n, 2000))
    src = rng.choice(n, 65, replace=False)
    a, _ = _bc(g, _matrix(g, S), n, src)
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A1 = _matrix(g, S)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    b, _ = _bc(g, A1, n, src)
    assert a.tobytes() == b.tobytes()
    _close(b, _ref(S, src)[0], "CSR only")


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_bc_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(31)
    n = 60
    S = _dir(n, rng.integers(0, n, 600), rng.integers(0, n, 600))
    A = _matrix(g, S, F, rng)
    held = rng.random(n).astype(F)
    v = g.Vector(n, F)
    assert v.build(held, n) == 0
    sparse = g.Vector(n, F)
    assert sparse.build(np.array([3, 9], I), np.array([2.5, -1.0], F), 2, None) == 0

    def unchanged():
        ok = np.array_equal(v.extractTuples()[1], held)
        i, idx, val = sparse.extractTuples(sparse=True)
        return ok and i == 0 and np.array_equal(idx, [3, 9]) and np.array_equal(val, np.array([2.5, -1.0], F))

    src = np.array([1, 2, 3], I)
    call = lambda v_, A_, s_=src, ns=3: lib.grb_bc(v_, A_, None if s_ is None else s_.ctypes.data, ns, None, None)
    assert unchanged()
    for vec in (v, sparse):
        assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                        # null handles
        assert call(vec._h, None) == g.GrB_UNINITIALIZED_OBJECT
        assert call(vec._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT      # an unbuilt A
        R = g.Matrix(n, n + 1, F)                                                    # A not square
        assert R.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, F)) == 0
        assert call(vec._h, R._h) == g.GrB_DIMENSION_MISMATCH
        assert call(vec._h, R._h, None, 0) == g.GrB_DIMENSION_MISMATCH
        for ns in (0, -1, -70):                                                      # a list without sources
            assert call(vec._h, A._h, src, ns) == g.GrB_INVALID_VALUE
        assert g.bc(vec, A, [], None)[0] == g.GrB_INVALID_VALUE
        for bad in ([-1], [n], [1, 2, n + 5], [0] * 64 + [n], [2 ** 31 - 1]):          # a source outside 0 .. n - 1
            assert g.bc(vec, A, bad, None)[0] == g.GrB_INVALID_INDEX
        assert unchanged()
    for m in (n - 1, n + 1):                                                         # size(bc) != n
        assert call(g.Vector(m, F)._h, A._h) == g.GrB_DIMENSION_MISMATCH
    vi = g.Vector(n, I)                                                              # bc not f32
    assert vi.build(np.arange(n, dtype=I), n) == 0
    assert call(vi._h, A._h) == g.GrB_NOT_IMPLEMENTED and call(vi._h, A._h, None, 0) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(vi.extractTuples()[1], np.arange(n))
    # A without a CSC of its own: a product result; its transpose under INP0 = TRAN has one
    One = _matrix(g, S, F)
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", One, One, hb.descriptor()) == 0
    assert call(v._h, P._h) == g.GrB_INVALID_OBJECT and call(sparse._h, P._h, None, 0) == g.GrB_INVALID_OBJECT
    assert unchanged()
    dt = hb.descriptor()
    assert dt.toggle(g.GrB_INP0) == 0
    P2 = g.Matrix(n, n, F)
    assert g.transpose(P2, None, None, P, dt) == 0
    pp, pi, _ = P2.host_csr()
    S2 = sp.csr_matrix((np.ones(pi.size, np.int64), pi, pp), shape=(n, n))
    S2.setdiag(0)
    S2.eliminate_zeros()
    S2.sort_indices()
    got, _ = _bc(g, P2, n, None)
    _close(got, _ref(S2, None)[0], "the product with a CSC")
    # a null descriptor and a descriptor give the same bits; a null record is accepted; a sparse bc becomes dense
    want = _ref(S, src)[0]
    a, _ = _bc(g, A, n, src)
    b, _ = _bc(g, A, n, src, hb.descriptor())
    assert a.tobytes() == b.tobytes()
    assert call(sparse._h, A._h) == 0
    assert sparse.extractTuples()[1].tobytes() == a.tobytes()
    _close(a, want, "errors, the good call")


def test_cpp_frontend(tmp_path):
    """tests/tools/bc.cpp: the fixture's graph through algorithm::bc"""
    exe = str(tmp_path / "bc")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "bc.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    lines = {ln.split(" ")[0]: ln.split(" ")[1:] for ln in subprocess.check_output([exe]).decode().split("\n")
             if ln.split(" ")[0] in ("all", "list", "two", "rec")}
    S = _fixture()
    want, reached, levels, _ = _ref(S, None)
    _close(np.array(lines["all"], np.float64).astype(F), want, "cpp all")
    assert lines["list"] == lines["all"]
    _close(np.array(lines["two"], np.float64).astype(F), _ref(S, [2, 2])[0], "cpp two")
    assert [int(x) for x in lines["rec"]] == [7, 1, levels, reached]
