"""The minimum spanning forest on the device (csrc/msf.hip: grb_msf) against a Kruskal in numpy under the key of the definition
in include/grb_hip.h: the edges sorted by np.lexsort((max, min, w)) and a union-find with path halving, cross-checked once
against scipy (total weight, n - components edges).  Every comparison of C (pointers, indices, value BITS), of comp and of
edges / forest_edges / components / isolated / launches is EXACT.  weight is exact wherever the weights are integers below
2^24; for general floats it is compared with math.fsum within forest_edges x 2^-53 x sum |w|, the bound of an f64 summation
in any order: derived, not tuned.  Ties, distinct weights in both element types with every special value, hook chains and
mutual pairs, every row-length class of the kernel, components and diagonals, degenerate shapes, the outputs' state
beforehand, in place, the CSR-only format, caller-owned storage, determinism, a relabelling, every error code that can be
asked for (a failed allocation and a barrier that gives up cannot) with C and comp unchanged, an asymmetric input taken on
the caller's word, and the C++ frontend."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
import scipy.sparse.csgraph as csgraph

from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
LANE_LEN = 8       # kMsLaneLen: a vertex whose CSR row has up to this many entries is walked by one lane
WAVE_LEN = 2048    # kMsWaveLen: ... up to this many by a wave, a longer one by the workgroup
LAUNCHES = 1
REC = ("edges", "forest_edges", "components", "isolated", "launches")


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs and the reference ------------------------------------------------------------------------------------------
class Graph:
    """n vertices; the edges {u, v} (u < v, each once) with the value w stored at (u, v) and w_rev at (v, u) (the same
    weight; a zero may differ in sign); diag: (vertex, value) pairs stored on the diagonal"""

    def __init__(self, n, u, v, w, dt, w_rev=None, diag=None):
        u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        assert (lo < hi).all() and np.unique(lo * n + hi).size == lo.size
        self.n, self.u, self.v, self.dt = n, lo, hi, dt
        self.w = np.asarray(w, dt)
        self.w_rev = self.w if w_rev is None else np.asarray(w_rev, dt)
        self.diag = (np.zeros(0, np.int64), np.zeros(0, dt)) if diag is None else (np.asarray(diag[0], np.int64), np.asarray(diag[1], dt))

    def csr(self, u=None, v=None, w=None, w_rev=None, diag=True):
        """-> pointers, indices, values of the matrix with both directions (of the given edges) and the diagonal"""
        u = self.u if u is None else u
        v = self.v if v is None else v
        w = self.w if w is None else w
        w_rev = self.w_rev if w_rev is None else w_rev
        d = self.diag if diag else (np.zeros(0, np.int64), np.zeros(0, self.dt))
        r = np.concatenate([u, v, d[0]])
        c = np.concatenate([v, u, d[0]])
        x = np.concatenate([w, w_rev, d[1]]).astype(self.dt)
        o = np.lexsort((c, r))
        ptr = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=self.n), out=ptr[1:])
        return ptr.astype(I), c[o].astype(I), x[o]


def _kruskal(gr):
    """-> the indices of the forest's edges (in key order), comp (the smallest member), components"""
    n = gr.n
    order = np.lexsort((gr.v, gr.u, gr.w))                # -0.0 and +0.0 compare equal; the key's order
    parent = list(range(n))
    uu, vv = gr.u[order].tolist(), gr.v[order].tolist()
    keep = []
    for k in range(len(uu)):
        a, b = uu[k], vv[k]
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        while parent[b] != b:
            parent[b] = parent[parent[b]]
            b = parent[b]
        if a != b:
            parent[b if a < b else a] = a if a < b else b    # the smaller number stays root
            keep.append(k)
    root = np.arange(n)
    for x in range(n):
        a = x
        while parent[a] != a:
            a = parent[a]
        root[x] = a
    return order[np.asarray(keep, np.int64)], root.astype(I), int((root == np.arange(n)).sum())


def _ref(gr):
    """-> (C's pointers, indices, values), comp, the record, the forest's edge indices"""
    forest, comp, comps = _kruskal(gr)
    fw = gr.w[forest]
    ptr, ind, val = gr.csr(gr.u[forest], gr.v[forest], fw, fw, diag=False)   # both directions hold the bits of the row of min(u, v)
    deg = np.bincount(np.concatenate([gr.u, gr.v]), minlength=gr.n) if gr.n else np.zeros(0, np.int64)
    rec = dict(edges=int(gr.u.size), forest_edges=int(forest.size), components=comps, isolated=int((deg == 0).sum()), launches=LAUNCHES)
    assert rec["forest_edges"] == gr.n - comps
    return (ptr, ind, val), comp, rec, forest


def _matrix(g, gr, csr_only=False, monkeypatch=None):
    if csr_only:
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(gr.n, gr.n, gr.dt)
    if csr_only:
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    ptr, ind, val = gr.csr()
    assert A.build_csr(ptr, ind, val) == 0
    return A


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check_weight(gr, forest, got, name):
    w = gr.w[forest]
    if gr.dt is I:
        assert got == float(int(w.astype(np.int64).sum())), (name, got)
        return
    w64 = w.astype(np.float64)
    if not np.isfinite(w64).all():
        want = float(np.sum(w64))
        assert (math.isnan(want) and math.isnan(got)) or want == got, (name, got, want)
        return
    want = math.fsum(w64.tolist())
    if (np.abs(w64) < 2.0 ** 24).all() and (w64 == np.round(w64)).all():
        assert got == want, (name, got, want)
    else:
        bound = forest.size * 2.0 ** -53 * math.fsum(np.abs(w64).tolist())
        print(name, "weight", got, "fsum", want, "difference", abs(got - want), "bound", bound)
        assert abs(got - want) <= bound, (name, got, want, bound)


def _check(hb, gr, A=None, Cm=None, comp="new", name="", want=None):
    """grb_msf on gr against the reference, exactly; -> (C's arrays, comp's values, the record)"""
    g = hb.g
    n = gr.n
    if want is None:
        want = _ref(gr)
    (wp, wi, wv), wcomp, rec, forest = want
    if A is None:
        A = _matrix(g, gr)
    if Cm is None:
        Cm = g.Matrix(n, n, gr.dt)
    if isinstance(comp, str):
        comp = g.Vector(n, I)
    info, res = g.msf(Cm, comp, A, None)
    assert info == 0, (name, info)
    print(name, {x: res[x] for x in REC}, "weight", res["weight"], "rounds", res["rounds"], "passes", res["passes"], "loop_ms", res["loop_ms"])
    for x in REC:
        assert res[x] == rec[x], (name, x, res, rec)
    assert Cm.nvals() == 2 * rec["forest_edges"]
    cp, ci, cv = Cm.host_csr()
    assert np.array_equal(cp, wp), (name, "pointers", np.flatnonzero(cp != wp)[:10])
    assert np.array_equal(ci, wi), (name, "indices", np.flatnonzero(ci != wi)[:10])
    assert cv.dtype == np.dtype(gr.dt) and np.array_equal(_bits(cv), _bits(wv)), (name, "values", np.flatnonzero(_bits(cv) != _bits(wv))[:10])
    got_comp = None
    if comp is not None:
        assert comp.getStorage() == g.GrB_DENSE and comp.nvals() == n
        info, got_comp = comp.extractTuples()
        assert info == 0 and got_comp.dtype == I
        bad = np.flatnonzero(got_comp != wcomp)
        assert bad.size == 0, (name, "comp", bad[:10], got_comp[bad[:10]], wcomp[bad[:10]])
    _check_weight(gr, forest, res["weight"], name)
    assert res["loop_ms"] >= 0 and res["passes"] >= 1 and res["rounds"] >= 0
    return (cp, ci, cv), got_comp, res


def _random_edges(rng, n, m):
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = u != v
    lo, hi = np.minimum(u, v)[keep], np.maximum(u, v)[keep]
    key = np.unique(lo.astype(np.int64) * n + hi)
    return key // n, key % n


def _distinct_f32(rng, m, shift=0.0):
    """m distinct finite f32 values of both signs, no zeros"""
    x = np.unique((rng.standard_normal(2 * m + 100) * 100 + shift).astype(F))
    x = x[x != 0]
    assert x.size >= m
    return rng.permutation(x)[:m]


# ---- the reference itself ----------------------------------------------------------------------------------------------
def test_reference_agrees_with_scipy():
    rng = np.random.default_rng(1)
    n = 3000
    u, v = _random_edges(rng, n, 5000)
    gr = Graph(n, u, v, rng.integers(1, 50, u.size), F)
    _, comp, rec, forest = _ref(gr)
    S = sp.csr_matrix((gr.w.astype(np.float64), (gr.u, gr.v)), shape=(n, n))
    assert csgraph.minimum_spanning_tree(S).sum() == gr.w[forest].astype(np.float64).sum()
    ncomp, lab = csgraph.connected_components(S, directed=False)
    assert ncomp == rec["components"] > 1 and forest.size == n - ncomp
    assert np.array_equal(np.unique(lab, return_inverse=True)[1], np.unique(comp, return_inverse=True)[1])
    assert (comp <= np.arange(n)).all() and (comp[comp] == comp).all()


# ---- ties --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
def test_all_equal_weights_on_a_complete_graph(hb, dt):
    """K_64 with one weight: the forest is the star of vertex 0"""
    u, v = np.triu_indices(64, 1)
    gr = Graph(64, u, v, np.full(u.size, 7), dt)
    want = _ref(gr)
    assert np.array_equal(gr.u[want[3]], np.zeros(63, np.int64)) and np.array_equal(np.sort(gr.v[want[3]]), np.arange(1, 64))
    (cp, ci, _), comp, res = _check(hb, gr, name=("K64", dt.__name__), want=want)
    assert cp[1] == 63 and np.array_equal(ci[:63], np.arange(1, 64)) and not comp.any() and res["weight"] == 7 * 63


def _grid_edges(side):
    idx = np.arange(side * side).reshape(side, side)
    return np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])


def test_unit_weight_grid(hb):
    u, v = _grid_edges(100)
    _, comp, res = _check(hb, Graph(10000, u, v, np.ones(u.size), F), name="grid")
    assert res["forest_edges"] == 9999 and res["weight"] == 9999.0 and not comp.any()


@pytest.mark.parametrize("dt", [F, I])
def test_few_distinct_weights_on_a_random_graph(hb, dt):
    """weights from {1, 2, 3, 4}, n = 20 000 and about 200 000 edges: without the tie-break by the endpoints the hooks form
    cycles or take a wrong edge"""
    rng = np.random.default_rng(2)
    n = 20000
    u, v = _random_edges(rng, n, 201000)
    assert u.size > 195000
    _check(hb, Graph(n, u, v, rng.integers(1, 5, u.size), dt), name=("ties", dt.__name__))


# ---- distinct weights, every special value -----------------------------------------------------------------------------
def test_distinct_i32_weights(hb):
    rng = np.random.default_rng(3)
    n = 10000
    u, v = _random_edges(rng, n, 40200)
    w = rng.choice(np.arange(-2 ** 31 + 1, 2 ** 31 - 1, 9973, dtype=np.int64), u.size, replace=False)
    w[5], w[77] = -2 ** 31, 2 ** 31 - 1
    assert np.unique(w).size == w.size and (w < 0).sum() > 1000
    gr = Graph(n, u, v, w, I)
    want = _ref(gr)
    assert 5 in want[3]                                   # INT32_MIN is the lightest edge of all
    _check(hb, gr, name="distinct i32", want=want)


def test_distinct_f32_weights_with_every_special_value(hb):
    """negatives, -0.0 beside +0.0 (one weight: the endpoints decide), +-inf, subnormals.  The edge stored as -0.0 in the row
    of its smaller end and as +0.0 in the other comes back as -0.0 both ways"""
    rng = np.random.default_rng(4)
    n = 10000
    u, v = _random_edges(rng, n, 40200)
    w = _distinct_f32(rng, u.size, 150.0)                 # about one in fifteen is negative: the zeros are light edges
    assert np.unique(w).size == w.size and 1000 < (w < 0).sum() < 5000 and not (w == 0).any()
    w_rev = w.copy()
    at = rng.choice(u.size, 47, replace=False)
    special = [np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, np.inf] + [-0.0, 0.0] * 20
    for k, x in zip(at, special):
        w[k] = w_rev[k] = x
    mixed = at[7::4]                                      # every other -0.0: +0.0 the other way round
    w_rev[mixed] = 0.0
    mixed2 = at[8::4]                                     # ... and every other +0.0: -0.0 the other way round
    w_rev[mixed2] = -0.0
    gr = Graph(n, u, v, w, F, w_rev=w_rev)
    want = _ref(gr)
    forest = set(want[3].tolist())
    zeros = [int(k) for k in at[7:] if int(k) in forest]
    assert int(at[1]) in forest and len(zeros) > 20 and set(mixed.tolist()) & forest and set(mixed2.tolist()) & forest
    assert {True, False} == set(bool(np.signbit(w[k])) for k in zeros)
    (cp, ci, cv), _, _ = _check(hb, gr, name="distinct f32", want=want)
    for k in zeros:                                       # the bits of the row of the smaller end, both ways
        a, b = int(gr.u[k]), int(gr.v[k])
        fwd = cv[cp[a]:cp[a + 1]][ci[cp[a]:cp[a + 1]] == b]
        back = cv[cp[b]:cp[b + 1]][ci[cp[b]:cp[b + 1]] == a]
        assert _bits(fwd)[0] == _bits(back)[0] == _bits(np.array([w[k]], F))[0]


# ---- hook chains and rounds --------------------------------------------------------------------------------------------
def test_path_with_ascending_weights_is_one_hook_chain(hb):
    """every vertex but 0 chooses the edge to its left: one chain of 4 095 hooks in round one, flat after log2 n jumps"""
    n = 4096
    a = np.arange(n - 1)
    for dt in (F, I):
        _, comp, res = _check(hb, Graph(n, a, a + 1, a, dt), name=("path up", dt.__name__))
        assert res["forest_edges"] == n - 1 and not comp.any() and res["weight"] == float(a.sum())


def test_path_that_pairs_neighbours_every_round(hb):
    """the edge {i, i + 1} weighs the number of trailing zeros of i + 1: every round joins neighbouring blocks in mutual pairs
    and halves the components, log2 n rounds at the least"""
    n = 4096
    a = np.arange(n - 1)
    w = np.array([((x + 1) & -(x + 1)).bit_length() - 1 for x in a.tolist()])
    _, _, res = _check(hb, Graph(n, a, a + 1, w, I), name="path pairs")
    assert res["rounds"] >= 12 and res["forest_edges"] == n - 1


def test_cycle_leaves_its_heaviest_edge_out(hb):
    rng = np.random.default_rng(5)
    n = 1000
    a = np.arange(n)
    u, v = np.minimum(a, (a + 1) % n), np.maximum(a, (a + 1) % n)
    w = rng.permutation(n) + 1
    gr = Graph(n, u, v, w, F)
    heavy = int(np.argmax(w))
    (cp, ci, _), _, res = _check(hb, gr, name="cycle")
    lo, hi = int(gr.u[heavy]), int(gr.v[heavy])
    assert res["forest_edges"] == n - 1 and hi not in ci[cp[lo]:cp[lo + 1]] and res["weight"] == float(w.sum() - w.max())


# ---- the row-length classes --------------------------------------------------------------------------------------------
def test_row_length_classes(hb):
    """hubs whose rows have 7, 8, 9 (a lane / a wave) and 2 047, 2 048, 2 049 (a wave / the workgroup) entries, as spokes to one
    shared set of leaves, so that the hubs compete for the leaves over several rounds; distinct weights in both types"""
    rng = np.random.default_rng(6)
    lengths = (LANE_LEN - 1, LANE_LEN, LANE_LEN + 1, WAVE_LEN - 1, WAVE_LEN, WAVE_LEN + 1)
    leaves = WAVE_LEN + 1
    n = leaves + len(lengths)
    perm = rng.permutation(n)                             # the hubs anywhere among the leaves
    us, vs = [], []
    for h, length in enumerate(lengths):
        us.append(np.full(length, leaves + h))
        vs.append(rng.choice(leaves, length, replace=False))
    u, v = perm[np.concatenate(us)], perm[np.concatenate(vs)]
    for dt in (F, I):
        gr = Graph(n, u, v, rng.permutation(u.size) - 3000, dt)
        ptr = gr.csr()[0]
        assert sorted(np.diff(ptr)[perm[leaves:]].tolist()) == sorted(lengths)
        _check(hb, gr, name=("classes", dt.__name__))


def test_star_takes_the_workgroup_walk(hb):
    """5 000 leaves: the centre's row is the workgroup's, its forest row is the whole star"""
    n = 5001
    rng = np.random.default_rng(7)
    leaves = np.arange(1, n)
    (cp, ci, _), comp, res = _check(hb, Graph(n, np.full(n - 1, 2500), np.where(leaves <= 2500, leaves - 1, leaves), rng.permutation(n - 1), F),
                                    name="star")
    assert res["forest_edges"] == n - 1 and cp[2501] - cp[2500] == n - 1 and not comp.any()


@pytest.mark.parametrize("length", [1000, 3000])
@pytest.mark.parametrize("where", ["first", "last"])
def test_candidate_at_the_end_of_a_long_row(hb, length, where):
    """a wave's and a workgroup's row whose lightest entry sits in its first or its last position; every other neighbour of
    the hub is tied to a second hub by a lighter edge, so only that one entry of the first hub's row joins the forest"""
    n = length + 2
    x, y = (n - 1, n - 2)                                 # two hubs numbered past their neighbours: positions = neighbour numbers
    nb = np.arange(length)
    pick = 0 if where == "first" else length - 1
    wx = 10000.0 + (np.arange(length)[::-1] if where == "last" else np.arange(length))
    wx[pick] = 5000.0
    u = np.concatenate([np.full(length, x), np.full(length, y)])
    v = np.concatenate([nb, nb])
    w = np.concatenate([wx, 1.0 + np.arange(length)])     # the second hub's edges: all lighter than the first one's
    gr = Graph(n, u, v, w, F)
    (cp, ci, _), _, res = _check(hb, gr, name=("long row", length, where))
    assert ci[cp[x]:cp[x + 1]].tolist() == [pick] and res["forest_edges"] == n - 1


# ---- components --------------------------------------------------------------------------------------------------------
def _components_graph(dt, seed=8):
    """300 components of random size, 500 isolated vertices of which every third stores its diagonal, diagonal entries on a
    tenth of the others: all with weights below every edge's, which must be ignored"""
    rng = np.random.default_rng(seed)
    n = 6000
    label = np.concatenate([rng.integers(0, 300, n - 500), np.full(500, -1)])
    label = rng.permutation(label)
    us, vs = [], []
    for c in range(300):
        mem = np.flatnonzero(label == c)
        if mem.size > 1:
            a, b = _random_edges(rng, mem.size, 3 * mem.size)
            t = np.arange(1, mem.size)                    # ... and a random tree, so that the component is one
            a = np.concatenate([a, (rng.random(mem.size - 1) * t).astype(np.int64)])
            b = np.concatenate([b, t])
            us.append(mem[a])
            vs.append(mem[b])
    u, v = np.concatenate(us), np.concatenate(vs)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    key = np.unique(lo * n + hi)
    u, v = key // n, key % n
    iso = np.flatnonzero(label == -1)
    dg = np.concatenate([iso[::3], np.flatnonzero(label >= 0)[::10]])
    dv = np.full(dg.size, -np.inf if dt is F else -2 ** 31)
    return Graph(n, u, v, rng.integers(-50, 50, u.size), dt, diag=(dg, dv)), iso


@pytest.mark.parametrize("dt", [F, I])
def test_many_components_isolated_vertices_and_diagonals(hb, dt):
    gr, iso = _components_graph(dt)
    want = _ref(gr)
    assert want[2]["isolated"] == 500 and 700 < want[2]["components"] <= 800
    (cp, _, _), comp, _ = _check(hb, gr, name=("components", dt.__name__), want=want)
    assert (np.diff(cp)[iso] == 0).all() and np.array_equal(comp[iso], iso)


def test_comp_is_what_scc_returns(hb):
    g = hb.g
    gr, _ = _components_graph(F, seed=9)
    A = _matrix(g, gr)
    _, comp, _ = _check(hb, gr, A=A, name="against scc")
    v = g.Vector(gr.n, I)
    info, res = g.scc(v, A, None)
    assert info == 0 and np.array_equal(v.extractTuples()[1], comp)


# ---- degenerate shapes, the outputs' state beforehand, aliasing, formats ------------------------------------------------
def test_degenerate(hb):
    g = hb.g
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    C0, v0 = g.Matrix(0, 0, F), g.Vector(0, I)
    info, res = g.msf(C0, v0, A0, None)
    assert info == 0 and all(res[x] == 0 for x in REC) and res["weight"] == 0 and res["rounds"] == 0 and C0.nvals() == 0
    none = np.zeros(0, np.int64)
    for n, diag in ((1, None), (1, ([0], [5])), (50, None), (50, (np.arange(0, 50, 3), np.full(17, -4)))):
        for dt in (F, I):
            gr = Graph(n, none, none, none, dt, diag=diag)
            _, comp, res = _check(hb, gr, name=("no edges", n))
            assert res["components"] == res["isolated"] == n and res["weight"] == 0 and res["edges"] == 0
            assert np.array_equal(comp, np.arange(n))
    _, comp, res = _check(hb, Graph(300, [3, 5, 3, 7], [5, 7, 7, 200], [2, 1, 3, 0], I), name="one triangle and a stored zero")
    assert res["forest_edges"] == 3 and res["weight"] == 3.0 and comp[200] == 3 and comp[0] == 0


def test_outputs_prefilled_null_in_place_and_csr_only(hb, monkeypatch):
    g = hb.g
    rng = np.random.default_rng(10)
    n = 700
    u, v = _random_edges(rng, n, 2500)
    gr = Graph(n, u, v, _distinct_f32(rng, u.size), F)
    want = _ref(gr)
    A = _matrix(g, gr)
    ou, ov = _random_edges(rng, n, 4000)
    Cfull = _matrix(g, Graph(n, ou, ov, np.ones(ou.size), F))   # a C that holds something else
    dense = g.Vector(n, I)
    assert dense.build(np.full(n, 9, I), n) == 0
    _check(hb, gr, A=A, Cm=Cfull, comp=dense, name="prefilled", want=want)
    sparse = g.Vector(n, I)
    assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
    _check(hb, gr, A=A, comp=sparse, name="sparse comp", want=want)
    _check(hb, gr, A=A, comp=None, name="null comp", want=want)
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Conly = g.Matrix(n, n, F)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    _check(hb, gr, A=A, Cm=Conly, name="C CSR only", want=want)
    Aonly = _matrix(g, gr, csr_only=True, monkeypatch=monkeypatch)
    (cp, ci, cv), _, _ = _check(hb, gr, A=Aonly, name="A CSR only", want=want)
    C = g.Matrix(n, n, F)                                 # both orientations: the CSC is the CSR
    assert g.msf(C, None, A, None)[0] == 0
    for got, ref in zip(C.host_csc(), (cp, ci, cv)):
        assert np.array_equal(_bits(got) if got.dtype == F else got, _bits(ref) if ref.dtype == F else ref)
    _check(hb, gr, A=A, Cm=A, name="in place", want=want)   # last: A is its own forest now
    _check(hb, Graph(n, gr.u[want[3]], gr.v[want[3]], gr.w[want[3]], F), A=A, name="the forest's forest")


def test_comp_on_caller_owned_storage(hb):
    """comp adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(11)
    n = 1003
    u, v = _random_edges(rng, n, 1500)
    gr = Graph(n, u, v, rng.integers(1, 9, u.size), I)
    want = _ref(gr)
    A = _matrix(g, gr)
    for k in ad.KS:
        comp, t, check = ad.adopt_dense(g, np.full(n, 77, I), k)
        assert comp.device_ptrs()[2] % 16 == 4 * k
        _, got, _ = _check(hb, gr, A=A, comp=comp, name=("adopted", k), want=want)
        assert np.array_equal(ad.payload(t, k, n, I), got)
        check(("msf", k))


# ---- determinism, relabelling ------------------------------------------------------------------------------------------
def test_three_runs_give_the_same_bits(hb):
    g = hb.g
    rng = np.random.default_rng(12)
    n = 30000
    u, v = _random_edges(rng, n, 150000)
    gr = Graph(n, u, v, (rng.random(u.size) * 10 + 0.001).astype(F), F)     # non-integer weights, ties among them
    want = _ref(gr)
    A = _matrix(g, gr)
    outs = []
    for _ in range(3):
        (cp, ci, cv), comp, res = _check(hb, gr, A=A, name="determinism", want=want)
        outs.append((cp.tobytes(), ci.tobytes(), cv.tobytes(), comp.tobytes(), [res[x] for x in REC], np.float64(res["weight"]).tobytes()))
    assert outs[0] == outs[1] == outs[2]


def test_relabelling_with_distinct_weights(hb):
    rng = np.random.default_rng(13)
    n = 5000
    u, v = _random_edges(rng, n, 20000)
    w = _distinct_f32(rng, u.size)
    gr = Graph(n, u, v, w, F)
    (cp, ci, cv), _, res = _check(hb, gr, name="as drawn")
    perm = rng.permutation(n)                             # vertex x becomes perm[x]
    pu, pv = perm[gr.u], perm[gr.v]
    swap = pu > pv
    grp = Graph(n, pu, pv, w, F)
    assert np.array_equal(grp.w, w) and swap.any()
    (pp, pi, pw), _, resp = _check(hb, grp, name="relabelled")
    rows = np.repeat(np.arange(n), np.diff(cp))
    prow = np.repeat(np.arange(n), np.diff(pp))
    a = sorted(zip(perm[rows].tolist(), perm[ci].tolist(), _bits(cv).tolist()))
    b = sorted(zip(prow.tolist(), pi.tolist(), _bits(pw).tolist()))
    assert a == b and [res[x] for x in REC] == [resp[x] for x in REC]


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_c_and_comp_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(14)
    n = 80
    u, v = _random_edges(rng, n, 300)
    gr = Graph(n, u, v, rng.integers(1, 9, u.size), F)
    A = _matrix(g, gr)
    ptr, ind, val = gr.csr()
    Cm = _matrix(g, Graph(n, u[:50], v[:50], np.arange(50) + 1, F))
    cbefore = Cm.host_csr()
    before = rng.integers(5, 1000, n).astype(I)
    comp = g.Vector(n, I)
    assert comp.build(before, n) == 0
    sv = g.Vector(n, I)                                   # a sparse comp stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0

    def unchanged():
        now = Cm.host_csr()
        assert Cm.nvals() == 100 and all(np.array_equal(x, y) for x, y in zip(now, cbefore))
        assert comp.getStorage() == g.GrB_DENSE and np.array_equal(comp.extractTuples()[1], before)
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
        info, si, sx = sv.extractTuples(sparse=True)
        return info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]

    def call(c, v_, a):
        return lib.grb_msf(c, v_, a, None, None)

    assert call(None, comp._h, A._h) == g.GrB_UNINITIALIZED_OBJECT                   # null handles
    assert call(Cm._h, comp._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(Cm._h, comp._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT  # an unbuilt A
    R = g.Matrix(n, n + 1, F)                                                        # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(Cm._h, comp._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Matrix(n, n + 1, F)._h, comp._h, A._h) == g.GrB_DIMENSION_MISMATCH   # C not n x n
    assert call(g.Matrix(n + 1, n, F)._h, comp._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert call(Cm._h, g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH      # size(comp) != n
    assert unchanged()
    fv = g.Vector(n, F)                                                              # a comp that is not i32
    fbefore = rng.random(n).astype(F) + 2
    assert fv.build(fbefore, n) == 0
    assert call(Cm._h, fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(_bits(fv.extractTuples()[1]), _bits(fbefore))
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                         # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(Cm._h, comp._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    Ci = _matrix(g, Graph(n, u[:50], v[:50], np.arange(50) + 1, I))                  # C not of A's type
    cibefore = Ci.host_csr()
    assert call(Ci._h, comp._h, A._h) == g.GrB_DOMAIN_MISMATCH
    assert all(np.array_equal(x, y) for x, y in zip(Ci.host_csr(), cibefore))
    assert unchanged()
    # an asymmetric structure (with a CSC of its own)
    D = sp.csr_matrix((np.ones(300, F), (rng.integers(0, n, 300), rng.integers(0, n, 300))), shape=(n, n))
    D.sum_duplicates()
    D.sort_indices()
    assert (D != D.T).nnz > 0
    Dm = g.Matrix(n, n, F)
    assert Dm.build_csr(D.indptr.astype(I), D.indices.astype(I), np.ones(D.nnz, F)) == 0
    # asymmetric values on a symmetric structure: one entry of one direction differs
    bad = val.copy()
    bad[int(ptr[int(gr.v[0])])] += 1
    Vm = g.Matrix(n, n, F)
    assert Vm.build_csr(ptr, ind, bad) == 0
    # a NaN off the diagonal, in both directions, so that the matrix is symmetric bit for bit
    wn = gr.w.copy()
    wn[7] = np.nan
    Nm = _matrix(g, Graph(n, gr.u, gr.v, wn, F))
    for M in (Dm, Vm, Nm):
        for c_ in (comp, sv, None):
            assert call(Cm._h, c_._h if c_ is not None else None, M._h) == g.GrB_INVALID_VALUE
            assert unchanged()
    # a NaN on the diagonal is no weight; -0.0 against +0.0 is no asymmetry
    wz = gr.w.copy()
    wz[3] = -0.0
    wr = wz.copy()
    wr[3] = 0.0
    ok = Graph(n, gr.u, gr.v, wz, F, w_rev=wr, diag=([4, 9], [np.nan, np.nan]))
    _check(hb, ok, name="NaN on the diagonal")
    # a descriptor and a null descriptor give the same result; the record is optional
    C1, C2 = g.Matrix(n, n, F), g.Matrix(n, n, F)
    assert lib.grb_msf(C1._h, None, A._h, hb.descriptor()._h, None) == 0 and lib.grb_msf(C2._h, comp._h, A._h, None, None) == 0
    assert all(np.array_equal(x, y) for x, y in zip(C1.host_csr(), C2.host_csr()))
    assert np.array_equal(comp.extractTuples()[1], _ref(gr)[1])


def test_csr_only_input_with_asymmetric_values_returns(hb, monkeypatch):
    """an A without a CSC of its own is taken on the caller's word.  With values that differ between the two directions the
    result is unspecified, but the call returns and C's arrays are well-formed.  Every loop of the kernel is bounded, so
    this is an ordinary test of those bounds"""
    g = hb.g
    rng = np.random.default_rng(15)
    n = 2000
    u, v = _random_edges(rng, n, 8000)
    gr = Graph(n, u, v, rng.integers(1, 4, u.size), F, w_rev=rng.integers(1, 4, u.size))
    A = _matrix(g, gr, csr_only=True, monkeypatch=monkeypatch)
    Cm, comp = g.Matrix(n, n, F), g.Vector(n, I)
    info, res = g.msf(Cm, comp, A, None)
    print("asymmetric values, CSR only:", info, res)
    assert isinstance(info, int)
    if info == 0:
        cp, ci, _ = Cm.host_csr()
        assert cp[0] == 0 and (np.diff(cp) >= 0).all() and cp[-1] == Cm.nvals() == ci.size <= 2 * (n - 1)
        assert ci.size == 0 or (ci.min() >= 0 and ci.max() < n)
        assert res["launches"] == LAUNCHES and res["rounds"] <= 32


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def test_cpp_frontend(tmp_path):
    """tests/tools/msf.cpp on chesapeake.mtx with unit weights: the record, C's structure and comp against the Kruskal"""
    exe = str(tmp_path / "msf")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "msf.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    path = os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    co = sp.coo_matrix(scipy.io.mmread(path))
    keep = co.row != co.col
    lo, hi = np.minimum(co.row, co.col)[keep].astype(np.int64), np.maximum(co.row, co.col)[keep].astype(np.int64)
    n = co.shape[0]
    key = np.unique(lo * n + hi)
    gr = Graph(n, key // n, key % n, np.ones(key.size), F)
    (wp, wi, _), comp, rec, forest = _ref(gr)
    assert rec["edges"] == 170 and rec["forest_edges"] == 38
    assert lines[-1] == "ok"
    assert "float edges 170 forest 38 weight 38 components 1 isolated 0 launches 1" in lines
    assert "csr | " + " ".join(map(str, wp.tolist())) + " | " + " ".join(map(str, wi.tolist())) in lines
    assert "comp " + " ".join(map(str, comp.tolist())) in lines
    assert "int forest 38 nvals 76" in lines
