"""Biconnected components, articulation points and bridges on the device (csrc/bcc.hip: grb_bcc) against networkx under the
definition in include/grb_hip.h: the edge sets of nx.biconnected_component_edges, every edge normalised to (min, max), the
blocks sorted by their smallest edge; art(v) = the number of blocks that contain v.  The reference is first checked against
itself (nx.articulation_points, nx.bridges).  Every comparison is EXACT: C's pointers, indices and values in both modes, its
CSC, art, and edges / largest / blocks / bridges / articulation / components / isolated / levels / launches.  Literal
graphs, random graphs in both element types with diagonals, isolated vertices and stored zeros, every row-length class of the
kernel with the hub as a root and not, deep forests, many interleaved components, a permuted numbering, degenerate shapes, the
outputs' state beforehand, null outputs, in place, the CSR-only format, caller-owned storage, determinism (also on four CUs in
a child process), every error code that can be asked for (a failed allocation and a barrier that gives up cannot) with C and
art unchanged, an asymmetric input taken on the caller's word, RMAT-12 and the C++ frontend."""
import ctypes
import os
import subprocess
import sys

import networkx as nx
import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp

from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
LANE_LEN = 8       # kBcLaneLen: a vertex whose CSR row has up to this many entries is walked by one lane
WAVE_LEN = 2048    # kBcWaveLen: ... up to this many by a wave, a longer one by the workgroup
BLOCKS, BRIDGES = 0, 1
EXACT = ("edges", "largest", "blocks", "bridges", "articulation", "components", "isolated", "levels", "launches")


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs and the reference ------------------------------------------------------------------------------------------
class Graph:
    """n vertices; the edges {u, v} (each once); diag: the vertices with a stored diagonal entry; the stored values are
    `fill` everywhere (they are never read: a zero is as good as any)"""

    def __init__(self, n, u, v, dt=F, diag=None, fill=0):
        u, v = np.asarray(u, np.int64).ravel(), np.asarray(v, np.int64).ravel()
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        assert (lo < hi).all() and np.unique(lo * max(n, 1) + hi).size == lo.size and (hi.size == 0 or hi.max() < n)
        o = np.lexsort((hi, lo))
        self.n, self.u, self.v, self.dt, self.fill = n, lo[o], hi[o], dt, fill
        self.diag = np.zeros(0, np.int64) if diag is None else np.asarray(diag, np.int64)

    def csr(self):
        r = np.concatenate([self.u, self.v, self.diag])
        c = np.concatenate([self.v, self.u, self.diag])
        o = np.lexsort((c, r))
        ptr = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.bincount(r, minlength=self.n), out=ptr[1:])
        return ptr.astype(I), c[o].astype(I), np.full(r.size, self.fill, self.dt)

    def nx(self):
        G = nx.Graph()
        G.add_nodes_from(range(self.n))
        G.add_edges_from(zip(self.u.tolist(), self.v.tolist()))
        return G


def from_nx(G, dt=F, **kw):
    """a networkx graph whose nodes are 0 .. n-1 (or anything sortable: numbered in sorted order)"""
    nodes = sorted(G.nodes())
    at = {x: k for k, x in enumerate(nodes)}
    e = [(at[a], at[b]) for a, b in G.edges() if a != b]
    return Graph(len(nodes), [a for a, _ in e], [b for _, b in e], dt, **kw)


def _levels(gr):
    """the depth of the BFS forest rooted at every component's smallest vertex, + 1"""
    if gr.n == 0:
        return 0
    ptr, ind, _ = gr.csr()
    A = sp.csr_matrix((np.ones(ind.size, np.int8), ind, ptr), shape=(gr.n, gr.n))
    ncomp, lab = sp.csgraph.connected_components(A, directed=False)
    roots = np.full(ncomp, gr.n, np.int64)
    np.minimum.at(roots, lab, np.arange(gr.n))
    seen = np.zeros(gr.n, bool)
    seen[roots] = True
    front, levels = roots, 0
    while front.size:
        levels += 1
        nb = np.unique(A[front].indices)
        front = nb[~seen[nb]]
        seen[front] = True
    return levels


def _block_csr(n, lo, hi, num):
    """both directions of the edges (lo, hi) with the value num -> pointers, indices, values"""
    r, c, x = np.concatenate([lo, hi]), np.concatenate([hi, lo]), np.concatenate([num, num])
    o = np.lexsort((c, r))
    ptr = np.zeros(n + 1, np.int64)
    if r.size:
        np.cumsum(np.bincount(r, minlength=n), out=ptr[1:])
    return ptr.astype(I), c[o].astype(I), x[o].astype(I)


def _ref(gr):
    """-> dict(blocks = C's arrays in GRB_BCC_BLOCKS mode, bridges = ... in GRB_BCC_BRIDGES mode, art, rec, family = the
    blocks as sorted tuples of edges in the order of their numbers)"""
    n = gr.n
    G = gr.nx()
    family = [tuple(sorted((min(a, b), max(a, b)) for a, b in es)) for es in nx.biconnected_component_edges(G)]
    family.sort(key=lambda b: b[0])
    m = gr.u.size
    assert sum(len(b) for b in family) == m
    num = {}
    art = np.zeros(n, np.int64)
    for k, b in enumerate(family):
        for e in b:
            num[e] = k
        art[sorted(set(x for e in b for x in e))] += 1
    lab = np.array([num[e] for e in zip(gr.u.tolist(), gr.v.tolist())], np.int64)
    sizes = np.array([len(b) for b in family], np.int64)
    single = sizes[lab] == 1 if m else np.zeros(0, bool)
    deg = np.bincount(np.concatenate([gr.u, gr.v]), minlength=n) if n else np.zeros(0, np.int64)
    rec = dict(edges=int(m), largest=int(sizes.max()) if m else 0, blocks=len(family), bridges=int((sizes == 1).sum()),
               articulation=int((art >= 2).sum()), components=nx.number_connected_components(G), isolated=int((deg == 0).sum()),
               levels=_levels(gr), launches=1 if n else 0)
    return dict(blocks=_block_csr(n, gr.u, gr.v, lab), bridges=_block_csr(n, gr.u[single], gr.v[single], lab[single]), art=art.astype(I),
                rec=rec, family=family)


def _matrix(g, gr, csr_only=False, monkeypatch=None):
    if csr_only:
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(gr.n, gr.n, gr.dt)
    if csr_only:
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    ptr, ind, val = gr.csr()
    assert A.build_csr(ptr, ind, val) == 0
    return A


def _run(hb, gr, mode, want, A, Cm="new", art="new", name="", csc=True):
    """one call against the reference, exactly; -> (C's arrays or None, art's values or None, the record)"""
    g = hb.g
    n = gr.n
    if isinstance(Cm, str):
        Cm = g.Matrix(n, n, I)
    if isinstance(art, str):
        art = g.Vector(n, I)
    info, res = g.bcc(Cm, art, A, mode, None)
    assert info == 0, (name, mode, info)
    print(name, "mode", mode, {x: res[x] for x in EXACT}, "rounds", res["rounds"], "passes", res["passes"], "loop_ms", res["loop_ms"])
    for x in EXACT:
        assert res[x] == want["rec"][x], (name, mode, x, res, want["rec"])
    got_c = got_art = None
    if Cm is not None:
        wp, wi, wv = want["blocks" if mode == BLOCKS else "bridges"]
        assert Cm.nvals() == wi.size, (name, mode, Cm.nvals(), wi.size)
        cp, ci, cv = Cm.host_csr()
        assert np.array_equal(cp, wp), (name, mode, "pointers", np.flatnonzero(cp != wp)[:10])
        assert np.array_equal(ci, wi), (name, mode, "indices", np.flatnonzero(ci != wi)[:10])
        assert cv.dtype == np.dtype(I) and np.array_equal(cv, wv), (name, mode, "values", np.flatnonzero(cv != wv)[:10], cv[:20], wv[:20])
        if csc:                                           # an edge has one block both ways: the CSC is the transposed CSR = the CSR
            tp, ti, tv = Cm.host_csc()
            assert np.array_equal(tp, wp) and np.array_equal(ti, wi) and np.array_equal(tv, wv), (name, mode, "CSC")
        got_c = (cp, ci, cv)
    if art is not None:
        assert art.getStorage() == g.GrB_DENSE and art.nvals() == n
        info, got_art = art.extractTuples()
        assert info == 0 and got_art.dtype == I
        bad = np.flatnonzero(got_art != want["art"])
        assert bad.size == 0, (name, mode, "art", bad[:10], got_art[bad[:10]], want["art"][bad[:10]])
    assert res["loop_ms"] >= 0 and (n == 0 or res["passes"] >= 1) and res["rounds"] >= 0
    return got_c, got_art, res


def _check(hb, gr, name="", want=None, A=None):
    """both modes on gr; -> the reference"""
    if want is None:
        want = _ref(gr)
    if A is None:
        A = _matrix(hb.g, gr)
    _run(hb, gr, BLOCKS, want, A, name=name)
    _run(hb, gr, BRIDGES, want, A, name=name)
    return want


def _random_edges(rng, n, m):
    u, v = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = u != v
    lo, hi = np.minimum(u, v)[keep], np.maximum(u, v)[keep]
    key = np.unique(lo.astype(np.int64) * n + hi)
    return key // n, key % n


_CACHE = {}


def _rmat12():
    """RMAT-12 ef16, symmetrised, and its reference: computed once"""
    if "rmat" not in _CACHE:
        from graphblast_amd import graphgen
        src, dst, n = graphgen.rmat_edges(12, 16, seed=1)
        keep = src != dst
        lo, hi = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
        key = np.unique(lo * n + hi)
        gr = Graph(n, key // n, key % n, F, fill=1)
        _CACHE["rmat"] = (gr, _ref(gr))
    return _CACHE["rmat"]


def _path(n):
    a = np.arange(n - 1)
    return Graph(n, a, a + 1)


# ---- the reference itself ----------------------------------------------------------------------------------------------
def test_reference_agrees_with_itself():
    """no GPU work: {v : art(v) >= 2} = nx.articulation_points, the blocks of one edge = nx.bridges"""
    rng = np.random.default_rng(1)
    u, v = _random_edges(rng, 2000, 2200)
    for gr, want in (_rmat12(), (_path(3000), None), (Graph(2000, u, v), None)):
        want = want or _ref(gr)
        G = gr.nx()
        assert set(np.flatnonzero(want["art"] >= 2).tolist()) == set(nx.articulation_points(G))
        singles = set(b[0] for b in want["family"] if len(b) == 1)
        assert singles == set((min(a, b), max(a, b)) for a, b in nx.bridges(G))
        assert want["rec"]["bridges"] == len(singles) and want["rec"]["articulation"] == int((want["art"] >= 2).sum())
        assert [b[0] for b in want["family"]] == sorted(b[0] for b in want["family"])
    rec = _rmat12()[1]["rec"]
    assert rec["blocks"] > 100 and rec["bridges"] > 100 and rec["articulation"] > 50 and rec["largest"] > 40000


# ---- literals ----------------------------------------------------------------------------------------------------------
def _grid(side):
    return from_nx(nx.convert_node_labels_to_integers(nx.grid_2d_graph(side, side), ordering="sorted"))


def _grid_with_pendants(side):
    G = nx.convert_node_labels_to_integers(nx.grid_2d_graph(side, side), ordering="sorted")
    n = side * side
    for at, first in ((0, n), (side * (side // 2) + side // 2, n + 3)):    # a corner, an interior vertex
        nx.add_path(G, [at, first, first + 1, first + 2])
    return from_nx(G)


def _two_cycles_and_a_bridge():
    G = nx.cycle_graph(5)
    G.add_edges_from([(5, 6), (6, 7), (7, 8), (8, 5), (2, 7)])
    return from_nx(G)


def _theta():
    G = nx.Graph()
    for p in ([0, 2, 3, 1], [0, 4, 1], [0, 5, 6, 7, 1]):
        nx.add_path(G, p)
    return from_nx(G)


def _cactus():
    G = nx.Graph()
    nx.add_path(G, [0, 1, 2, 3, 4, 5])
    nx.add_cycle(G, [1, 6, 7])
    nx.add_cycle(G, [3, 8, 9, 10])
    nx.add_cycle(G, [5, 11, 12, 13, 14])
    return from_nx(G)


def _out_of_order():
    """the blocks' smallest edges against the order of discovery from vertex 0: {0,9} | {1,2,3} | {1,4} | {4,5,9}"""
    return Graph(10, [0, 9, 4, 5, 4, 1, 2, 1], [9, 4, 5, 9, 1, 2, 3, 3])


LITERALS = {
    "edge": lambda: Graph(2, [0], [1]),
    "triangle": lambda: from_nx(nx.cycle_graph(3)),
    "path5": lambda: _path(5),
    "cycle6": lambda: from_nx(nx.cycle_graph(6)),
    "cycle7": lambda: from_nx(nx.cycle_graph(7)),
    "bowtie": lambda: Graph(5, [0, 0, 1, 0, 0, 3], [1, 2, 2, 3, 4, 4]),
    "two cycles and a bridge": _two_cycles_and_a_bridge,
    "K4": lambda: from_nx(nx.complete_graph(4)),
    "K5": lambda: from_nx(nx.complete_graph(5)),
    "barbell": lambda: from_nx(nx.barbell_graph(4, 3)),
    "theta": _theta,
    "cactus": _cactus,
    "petersen": lambda: from_nx(nx.petersen_graph()),
    "grid30": lambda: _grid(30),
    "grid30 with pendants": lambda: _grid_with_pendants(30),
    "star5": lambda: from_nx(nx.star_graph(5)),
    "binary tree": lambda: from_nx(nx.balanced_tree(2, 6)),
    "out of order": _out_of_order,
}


@pytest.mark.parametrize("which", sorted(LITERALS))
def test_literals(hb, which):
    gr = LITERALS[which]()
    want = _check(hb, gr, name=which)
    rec = want["rec"]
    if which in ("triangle", "cycle6", "cycle7", "K4", "K5", "petersen", "grid30", "theta"):
        assert rec["blocks"] == 1 and rec["bridges"] == 0 and rec["articulation"] == 0 and rec["largest"] == rec["edges"]
    if which == "grid30 with pendants":
        assert rec["blocks"] == 7 and rec["bridges"] == 6 and rec["articulation"] == 6
    if which == "binary tree":
        assert rec["bridges"] == rec["blocks"] == 126 and rec["articulation"] == 63 and rec["levels"] == 7
    if which == "bowtie":
        assert want["art"].tolist() == [2, 1, 1, 1, 1]
    if which == "out of order":
        assert [len(b) for b in want["family"]] == [1, 3, 1, 3] and want["family"][1][0] == (1, 2)


# ---- random graphs -----------------------------------------------------------------------------------------------------
def test_two_hundred_small_random_graphs(hb):
    """n in 1 .. 60, m between 0.3 n and 2.2 n: many blocks, several components, isolated vertices, stored diagonals; both
    element types, the stored values zeros (an edge all the same) or anything else"""
    rng = np.random.default_rng(2)
    seen = dict(blocks=0, art=0, comps=0, iso=0)
    for k in range(200):
        n = int(rng.integers(1, 61))
        m = int(rng.uniform(0.3, 2.2) * n)
        u, v = _random_edges(rng, n, m) if n > 1 else (np.zeros(0, np.int64), np.zeros(0, np.int64))
        diag = np.flatnonzero(rng.random(n) < 0.2)
        gr = Graph(n, u, v, (F, I)[k % 2], diag=diag, fill=(0, 0, 3, -1)[k % 4])
        rec = _check(hb, gr, name=("random", k, n, m))["rec"]
        seen["blocks"] += rec["blocks"]
        seen["art"] += rec["articulation"]
        seen["comps"] += rec["components"] > 1
        seen["iso"] += rec["isolated"] > 0
    assert seen["blocks"] > 1500 and seen["art"] > 500 and seen["comps"] > 100 and seen["iso"] > 100


@pytest.mark.parametrize("seed", range(5))
def test_sparse_random_graph_of_two_thousand_vertices(hb, seed):
    rng = np.random.default_rng(100 + seed)
    u, v = _random_edges(rng, 2000, 2200)
    rec = _check(hb, Graph(2000, u, v, (F, I)[seed % 2], fill=seed), name=("random 2000", seed))["rec"]
    assert rec["blocks"] > 300 and rec["articulation"] > 250


# ---- the row-length classes --------------------------------------------------------------------------------------------
RIMS = (LANE_LEN, LANE_LEN + 1, WAVE_LEN, WAVE_LEN + 1, 2100)


def _hub_graph(kind, size, hub_last):
    """a hub and `size` rim vertices (wheel: the rim is a cycle; star: no rim edges) or `size` triangles on the hub"""
    if kind == "triangles":
        n = 2 * size + 1
        a = np.arange(size)
        u = np.concatenate([np.zeros(2 * size, np.int64), 1 + 2 * a])
        v = np.concatenate([1 + np.arange(2 * size), 2 + 2 * a])
    else:
        n = size + 1
        rim = 1 + np.arange(size)
        u, v = np.zeros(size, np.int64), rim
        if kind == "wheel":
            u, v = np.concatenate([u, rim]), np.concatenate([v, 1 + (rim % size)])
    if hub_last:                                          # the hub becomes vertex n - 1, the others move down: vertex 0 is the root
        u, v = (u - 1) % n, (v - 1) % n
    return Graph(n, u, v), (n - 1 if hub_last else 0)


@pytest.mark.parametrize("hub_last", [False, True])
@pytest.mark.parametrize("size", RIMS)
def test_wheel_is_one_block(hb, size, hub_last):
    gr, hub = _hub_graph("wheel", size, hub_last)
    assert np.diff(gr.csr()[0])[hub] == size
    want = _check(hb, gr, name=("wheel", size, hub_last))
    assert want["rec"]["blocks"] == 1 and want["rec"]["largest"] == 2 * size and (want["art"] == 1).all()


@pytest.mark.parametrize("hub_last", [False, True])
@pytest.mark.parametrize("size", RIMS)
def test_star_is_all_bridges(hb, size, hub_last):
    gr, hub = _hub_graph("star", size, hub_last)
    want = _check(hb, gr, name=("star", size, hub_last))
    assert want["rec"]["bridges"] == size and want["art"][hub] == size and want["rec"]["articulation"] == 1


@pytest.mark.parametrize("hub_last", [False, True])
def test_hub_of_three_thousand_triangles(hb, hub_last):
    """6 000 children of one vertex, 3 000 of them representatives: more than a wave's LDS stage and a workgroup's threads"""
    gr, hub = _hub_graph("triangles", 3000, hub_last)
    want = _check(hb, gr, name=("triangles", hub_last))
    assert want["art"][hub] == 3000 and want["rec"]["blocks"] == 3000 and want["rec"]["largest"] == 3 and want["rec"]["articulation"] == 1


# ---- depth -------------------------------------------------------------------------------------------------------------
def test_path_of_three_thousand(hb):
    want = _check(hb, _path(3000), name="path")
    assert want["rec"]["levels"] == 3000 and want["rec"]["bridges"] == 2999 and want["rec"]["articulation"] == 2998


def test_cycle_of_three_thousand_and_one(hb):
    want = _check(hb, from_nx(nx.cycle_graph(3001)), name="cycle")
    assert want["rec"]["blocks"] == 1 and want["rec"]["levels"] == 1501


def test_comb(hb):
    a = np.arange(500)
    gr = Graph(1000, np.concatenate([a[:-1], a]), np.concatenate([a[1:], a + 500]))
    want = _check(hb, gr, name="comb")
    assert want["rec"]["bridges"] == 999 and want["rec"]["articulation"] == 500 and want["rec"]["levels"] == 501


# ---- many components ---------------------------------------------------------------------------------------------------
def test_many_interleaved_components(hb):
    """1 000 triangles, 500 single edges, 300 isolated vertices of which 100 store their diagonal: under one permutation"""
    rng = np.random.default_rng(3)
    n = 3000 + 1000 + 300
    t = 3 * np.arange(1000)
    e = 3000 + 2 * np.arange(500)
    u = np.concatenate([t, t, t + 1, e])
    v = np.concatenate([t + 1, t + 2, t + 2, e + 1])
    perm = rng.permutation(n)
    gr = Graph(n, perm[u], perm[v], I, diag=perm[np.concatenate([np.arange(4000, 4100), t[:50]])], fill=5)
    want = _check(hb, gr, name="components")
    rec = want["rec"]
    assert rec["components"] == 1800 and rec["isolated"] == 300 and rec["blocks"] == 1500 and rec["bridges"] == 500
    assert rec["articulation"] == 0 and rec["levels"] == 2 and (want["art"][perm[4000:]] == 0).all()


# ---- a permuted numbering ----------------------------------------------------------------------------------------------
def test_permuted_numbering_gives_the_same_family(hb):
    g = hb.g
    rng = np.random.default_rng(4)
    n = 400
    u, v = _random_edges(rng, n, 520)
    gr = Graph(n, u, v)
    perm = rng.permutation(n)                             # vertex x becomes perm[x]
    grp = Graph(n, perm[gr.u], perm[gr.v])
    inv = np.argsort(perm)
    fams = []
    for x, back in ((gr, np.arange(n)), (grp, inv)):
        want = _ref(x)
        (cp, ci, cv), _, _ = _run(hb, x, BLOCKS, want, _matrix(g, x), name="permuted")
        rows = np.repeat(np.arange(n), np.diff(cp))
        fam = {}
        for a, b, k in zip(back[rows].tolist(), back[ci].tolist(), cv.tolist()):
            if a < b:
                fam.setdefault(k, set()).add((a, b))
        fams.append(set(frozenset(s) for s in fam.values()))
    assert fams[0] == fams[1] and len(fams[0]) > 50


# ---- degenerate shapes -------------------------------------------------------------------------------------------------
def test_degenerate(hb):
    g = hb.g
    none = np.zeros(0, np.int64)
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    C0, v0 = g.Matrix(0, 0, I), g.Vector(0, I)
    info, res = g.bcc(C0, v0, A0, BLOCKS, None)
    assert info == 0 and all(res[x] == 0 for x in EXACT) and res["rounds"] == 0 and res["passes"] == 0 and C0.nvals() == 0
    for n, diag in ((1, None), (1, [0]), (50, None), (50, np.arange(0, 50, 3))):
        for dt in (F, I):
            want = _check(hb, Graph(n, none, none, dt, diag=diag), name=("no edges", n))
            rec = want["rec"]
            assert rec["components"] == rec["isolated"] == n and rec["blocks"] == 0 and rec["levels"] == 1 and not want["art"].any()
    want = _check(hb, Graph(300, [7], [200], I, diag=[7, 9]), name="one pair")
    assert want["rec"]["blocks"] == want["rec"]["bridges"] == 1 and want["art"][7] == want["art"][200] == 1 and want["rec"]["components"] == 299


# ---- the outputs' state beforehand, null outputs, aliasing, formats ----------------------------------------------------
def test_outputs_prefilled_null_in_place_and_csr_only(hb, monkeypatch):
    g = hb.g
    rng = np.random.default_rng(5)
    n = 700
    u, v = _random_edges(rng, n, 900)
    gr = Graph(n, u, v, I, diag=[3, 500], fill=9)
    want = _ref(gr)
    assert want["rec"]["blocks"] > 100 and want["rec"]["bridges"] > 50
    A = _matrix(g, gr)
    for mode in (BLOCKS, BRIDGES):
        ou, ov = _random_edges(rng, n, 4000)
        Cfull = _matrix(g, Graph(n, ou, ov, I, fill=1))   # a C that holds something else
        dense = g.Vector(n, I)
        assert dense.build(np.full(n, 9, I), n) == 0
        _run(hb, gr, mode, want, A, Cm=Cfull, art=dense, name="prefilled")
        sparse = g.Vector(n, I)
        assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
        _run(hb, gr, mode, want, A, art=sparse, name="sparse art")
        _run(hb, gr, mode, want, A, art=None, name="null art")
        _run(hb, gr, mode, want, A, Cm=None, name="null C")
        _run(hb, gr, mode, want, A, Cm=None, art=None, name="both null")
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
        Conly = g.Matrix(n, n, I)
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
        _run(hb, gr, mode, want, A, Cm=Conly, name="C CSR only", csc=False)
        Aonly = _matrix(g, gr, csr_only=True, monkeypatch=monkeypatch)
        _run(hb, gr, mode, want, Aonly, name="A CSR only")
        Af = _matrix(g, Graph(n, gr.u, gr.v, F, diag=[3, 500]))   # a float A, an int C
        _run(hb, gr, mode, want, Af, name="float A")
    for mode in (BLOCKS, BRIDGES):                        # in place: A becomes its blocks / its bridges
        Ain = _matrix(g, gr)
        _run(hb, gr, mode, want, Ain, Cm=Ain, name="in place")
        wp, wi, _ = want["blocks" if mode == BLOCKS else "bridges"]
        rows = np.repeat(np.arange(n), np.diff(wp))
        up = wi > rows
        sub = Graph(n, rows[up], wi[up], I)               # what A holds now; its values (block numbers) are never read
        _run(hb, sub, BLOCKS, _ref(sub), Ain, name="the result's blocks")


def test_art_on_caller_owned_storage(hb):
    """art adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(6)
    n = 1003
    u, v = _random_edges(rng, n, 1300)
    gr = Graph(n, u, v, I, fill=2)
    want = _ref(gr)
    A = _matrix(g, gr)
    for k in ad.KS:
        art, t, check = ad.adopt_dense(g, np.full(n, 77, I), k)
        assert art.device_ptrs()[2] % 16 == 4 * k
        _, got, _ = _run(hb, gr, BLOCKS, want, A, art=art, name=("adopted", k))
        assert np.array_equal(ad.payload(t, k, n, I), got)
        check(("bcc", k))


# ---- determinism -------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import graphblast_amd as g
d = np.load(sys.argv[2])
out = {}
ptr, ind, val = d["ptr"], d["ind"], d["val"]
n = ptr.size - 1
A = g.Matrix(n, n, val.dtype.type)
assert A.build_csr(ptr, ind, val) == 0
for mode in (0, 1):
    art, Cm = g.Vector(n, np.int32), g.Matrix(n, n, np.int32)
    info, res = g.bcc(Cm, art, A, mode, None)
    assert info == 0 and res["launches"] == 1, (info, res)
    out["art%d" % mode] = art.extractTuples()[1]
    out["cp%d" % mode], out["ci%d" % mode], out["cv%d" % mode] = Cm.host_csr()
    out["rec%d" % mode] = np.array([res[x] for x in sys.argv[4].split(",")], np.int64)
np.savez(sys.argv[3], **out)
"""


def test_three_runs_and_a_child_on_four_cus_give_the_same_bits(hb, tmp_path):
    g = hb.g
    rng = np.random.default_rng(7)
    n = 5000
    u, v = _random_edges(rng, n, 6500)
    gr = Graph(n, u, v, F, fill=1)
    want = _ref(gr)
    A = _matrix(g, gr)
    first = {}
    for mode in (BLOCKS, BRIDGES):
        outs = []
        for _ in range(3):
            (cp, ci, cv), art, res = _run(hb, gr, mode, want, A, name="determinism")
            outs.append((art.tobytes(), cp.tobytes(), ci.tobytes(), cv.tobytes(), [res[x] for x in EXACT]))
        assert outs[0] == outs[1] == outs[2]
        first[mode] = outs[0]
    ptr, ind, val = gr.csr()
    np.savez(tmp_path / "in.npz", ptr=ptr, ind=ind, val=val)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, GRB_NUM_CU="4")
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz"), ",".join(EXACT)], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    for mode in (BLOCKS, BRIDGES):
        got = (out["art%d" % mode].tobytes(), out["cp%d" % mode].tobytes(), out["ci%d" % mode].tobytes(), out["cv%d" % mode].tobytes(),
               out["rec%d" % mode].tolist())
        assert got == first[mode], mode


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_c_and_art_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(8)
    n = 80
    u, v = _random_edges(rng, n, 120)
    gr = Graph(n, u, v, F, fill=1)
    A = _matrix(g, gr)
    ptr, ind, val = gr.csr()
    Cm = _matrix(g, Graph(n, u[:50], v[:50], I, fill=4))
    cbefore = Cm.host_csr()
    before = rng.integers(5, 1000, n).astype(I)
    art = g.Vector(n, I)
    assert art.build(before, n) == 0
    sv = g.Vector(n, I)                                   # a sparse art stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0

    def unchanged():
        now = Cm.host_csr()
        assert Cm.nvals() == 100 and all(np.array_equal(x, y) for x, y in zip(now, cbefore))
        assert art.getStorage() == g.GrB_DENSE and np.array_equal(art.extractTuples()[1], before)
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
        info, si, sx = sv.extractTuples(sparse=True)
        return info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]

    def call(c, v_, a, mode=BLOCKS):
        return lib.grb_bcc(c, v_, a, mode, None, None)

    assert call(Cm._h, art._h, None) == g.GrB_UNINITIALIZED_OBJECT                   # a null A
    assert call(Cm._h, art._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT   # an unbuilt A
    R = g.Matrix(n, n + 1, F)                                                        # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(Cm._h, art._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Matrix(n, n + 1, I)._h, art._h, A._h) == g.GrB_DIMENSION_MISMATCH  # C not n x n
    assert call(g.Matrix(n + 1, n, I)._h, art._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert call(Cm._h, g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH      # size(art) != n
    assert unchanged()
    fv = g.Vector(n, F)                                                              # an art that is not i32
    fbefore = rng.random(n).astype(F) + 2
    assert fv.build(fbefore, n) == 0
    assert call(Cm._h, fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(fv.extractTuples()[1].view(np.uint32), fbefore.view(np.uint32))
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                         # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(Cm._h, art._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    Cf = _matrix(g, Graph(n, u[:50], v[:50], F, fill=4))                             # C not i32
    cfbefore = Cf.host_csr()
    assert call(Cf._h, art._h, A._h) == g.GrB_DOMAIN_MISMATCH
    assert all(np.array_equal(x, y) for x, y in zip(Cf.host_csr(), cfbefore))
    assert unchanged()
    for mode in (-1, 2, 7):                                                          # a mode outside {0, 1}
        assert call(Cm._h, art._h, A._h, mode) == g.GrB_INVALID_VALUE
    assert unchanged()
    # an asymmetric structure (with a CSC of its own)
    D = sp.csr_matrix((np.ones(300, F), (rng.integers(0, n, 300), rng.integers(0, n, 300))), shape=(n, n))
    D.sum_duplicates()
    D.sort_indices()
    assert (D != D.T).nnz > 0
    Dm = g.Matrix(n, n, F)
    assert Dm.build_csr(D.indptr.astype(I), D.indices.astype(I), np.ones(D.nnz, F)) == 0
    for mode in (BLOCKS, BRIDGES):
        for c_ in (Cm, None):
            for a_ in (art, sv, None):
                assert call(c_._h if c_ is not None else None, a_._h if a_ is not None else None, Dm._h, mode) == g.GrB_INVALID_VALUE
                assert unchanged()
    # asymmetric VALUES are no asymmetry: they are never read
    bad = val.copy()
    bad[::3] = 5
    Vm = g.Matrix(n, n, F)
    assert Vm.build_csr(ptr, ind, bad) == 0
    _check(hb, gr, name="asymmetric values", A=Vm)
    # a descriptor and a null descriptor give the same result; the record is optional
    C1, C2 = g.Matrix(n, n, I), g.Matrix(n, n, I)
    assert lib.grb_bcc(C1._h, None, A._h, BLOCKS, hb.descriptor()._h, None) == 0 and lib.grb_bcc(C2._h, art._h, A._h, BLOCKS, None, None) == 0
    assert all(np.array_equal(x, y) for x, y in zip(C1.host_csr(), C2.host_csr()))
    assert np.array_equal(art.extractTuples()[1], _ref(gr)["art"])


@pytest.mark.parametrize("which", ["literal", "random"])
def test_csr_only_input_with_asymmetric_structure_returns(hb, monkeypatch, which):
    """an A without a CSC of its own is taken on the caller's word.  With a structure that is not symmetric the result is
    unspecified, but the call returns and C's arrays are well-formed.  Every loop of the kernel is bounded, so this is an
    ordinary test of those bounds"""
    g = hb.g
    rng = np.random.default_rng(9)
    if which == "literal":
        n = 4
        D = sp.csr_matrix((np.ones(4, F), ([0, 1, 2, 3], [1, 2, 0, 0])), shape=(n, n))
    else:
        n = 50
        D = sp.csr_matrix((np.ones(120, F), (rng.integers(0, n, 120), rng.integers(0, n, 120))), shape=(n, n))
    D.sum_duplicates()
    D.sort_indices()
    assert (D != D.T).nnz > 0
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(n, n, F)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(D.indptr.astype(I), D.indices.astype(I), np.ones(D.nnz, F)) == 0
    for mode in (BLOCKS, BRIDGES):
        Cm, art = g.Matrix(n, n, I), g.Vector(n, I)
        info, res = g.bcc(Cm, art, A, mode, None)
        print("asymmetric structure, CSR only:", which, mode, info, res)
        assert isinstance(info, int)
        if info == 0:
            cp, ci, _ = Cm.host_csr()
            assert cp[0] == 0 and (np.diff(cp) >= 0).all() and cp[-1] == Cm.nvals() == ci.size <= D.nnz
            assert ci.size == 0 or (ci.min() >= 0 and ci.max() < n)
            assert res["launches"] == 1 and res["levels"] <= n


# ---- RMAT --------------------------------------------------------------------------------------------------------------
def test_rmat12(hb):
    gr, want = _rmat12()
    assert gr.n == 4096
    _check(hb, gr, name="RMAT-12", want=want)


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def test_cpp_frontend(tmp_path):
    """tests/tools/bcc.cpp on chesapeake.mtx: the record, C in both modes and art against networkx"""
    exe = str(tmp_path / "bcc")
    subprocess.run(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "bcc.cpp"),
                    "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip", "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe],
                   check=True, timeout=300)
    path = os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    co = sp.coo_matrix(scipy.io.mmread(path))
    keep = co.row != co.col
    lo, hi = np.minimum(co.row, co.col)[keep].astype(np.int64), np.maximum(co.row, co.col)[keep].astype(np.int64)
    n = co.shape[0]
    key = np.unique(lo * n + hi)
    want = _ref(Graph(n, key // n, key % n))
    rec = want["rec"]
    assert rec["edges"] == 170
    assert lines[-1] == "ok"
    assert ("blocks %d bridges %d articulation %d largest %d edges 170 components %d isolated %d levels %d launches 1"
            % (rec["blocks"], rec["bridges"], rec["articulation"], rec["largest"], rec["components"], rec["isolated"], rec["levels"])) in lines
    for tag, which in (("csr", "blocks"), ("bridges", "bridges")):
        wp, wi, wv = want[which]
        assert " ".join((tag + " | " + " ".join(map(str, wp.tolist())) + " | " + " ".join(map(str, wi.tolist())) + " | " +
                         " ".join(map(str, wv.tolist()))).split()) in lines
    assert "art " + " ".join(map(str, want["art"].tolist())) in lines
