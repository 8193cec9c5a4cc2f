"""Louvain community detection on the device (csrc/louvain.hip: grb_louvain) against tests/louvain_model.py, the host
restatement of the definition in include/grb_hip.h.  Every comparison is EXACT: labels, levels, rounds, moves, proposals,
communities, qn, w, and modularity as the same double.  The graphs are made here with numpy.  Structure (cliques, grid, path,
K3,3, a planted partition of two levels, components and isolated vertices, degenerate shapes), every row-length class of the
propose pass with the hub's neighbours over many communities and over few, the global-array route with two long rows in one
round, the acceptance rule (a star, rejected co-entrants, a winner that leaves), weights (i32 = f32, zeros, loops, -0.0, W
just below 2^31 - 1, weighted = 0), truncation, the state of labels beforehand, the CSR-only format, a product result,
caller-owned storage, determinism (also on four CUs in a child process), every error code that can be asked for with labels
unchanged, and the C++ frontend."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import louvain_model as lm
from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
BIG = 1 << 30
LANE_LEN, WAVE_LEN, SMALL_LEN, BLOCK_LEN = 8, 64, 256, 2048   # kLvLaneLen, kLvWaveLen, kLvSmallLen, kLvBlockLen
EXACT = ("levels", "rounds", "moves", "proposals", "communities", "qn", "w")


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- graphs ------------------------------------------------------------------------------------------------------------
class Graph:
    """n vertices; the undirected edges {u, v} with integer weights (each once); loops: {vertex: weight}.  The stored entries
    are both directions of every edge and every loop once, in CSR order"""

    def __init__(self, n, u, v, w=None, loops=None):
        u, v = np.asarray(u, np.int64).ravel(), np.asarray(v, np.int64).ravel()
        w = np.ones(u.size, np.int64) if w is None else np.asarray(w, np.int64).ravel()
        assert (u != v).all() and u.size == v.size == w.size
        lo, hi = np.minimum(u, v), np.maximum(u, v)
        assert np.unique(lo * max(n, 1) + hi).size == lo.size and (hi.size == 0 or hi.max() < n)
        loops = loops or {}
        lv = np.array(sorted(loops), np.int64)
        lw = np.array([loops[x] for x in sorted(loops)], np.int64)
        r = np.concatenate([lo, hi, lv])
        c = np.concatenate([hi, lo, lv])
        x = np.concatenate([w, w, lw])
        o = np.lexsort((c, r))
        self.n, self.rows, self.cols, self.w = n, r[o], c[o], x[o]
        self.ptr = np.zeros(n + 1, np.int64)
        if r.size:
            np.cumsum(np.bincount(r, minlength=n), out=self.ptr[1:])

    def csr(self, dt=I, values=None):
        return self.ptr.astype(I), self.cols.astype(I), (self.w if values is None else values).astype(dt)


def _matrix(g, gr, dt=I, values=None, csr_only=False, monkeypatch=None):
    if csr_only:
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(gr.n, gr.n, dt)
    if csr_only:
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(*gr.csr(dt, values)) == 0
    return A


def _model(gr, weighted=1, max_levels=BIG, max_rounds=BIG):
    return lm.run(gr.n, gr.rows, gr.cols, gr.w if weighted else np.ones(gr.w.size, np.int64), max_levels, max_rounds)


def _compare(name, info, res, got, want):
    assert info == 0, (name, info)
    print(name, {x: res[x] for x in EXACT}, "Q %.4f" % res["modularity"], "passes", res["passes"], "launches", res["launches"],
          "loop_ms", res["loop_ms"])
    for x in EXACT:
        assert res[x] == getattr(want, x), (name, x, res[x], getattr(want, x), [t for t in want.trace])
    assert res["modularity"] == want.modularity, (name, res["modularity"], want.modularity)
    assert got.dtype == I
    bad = np.flatnonzero(got != want.labels)
    assert bad.size == 0, (name, "labels", bad[:10], got[bad[:10]], want.labels[bad[:10]])
    assert res["loop_ms"] >= 0 and res["passes"] >= 0
    assert res["launches"] == (res["levels"] if res["w"] > 0 else 0), (name, "one launch a level", res)


def _run(hb, gr, A, want, weighted=1, max_levels=BIG, max_rounds=BIG, labels=None, name=""):
    g = hb.g
    if labels is None:
        labels = g.Vector(gr.n, I)
    info, res = g.louvain(labels, A, weighted, max_levels, max_rounds, None)
    assert info == 0, (name, info)
    assert labels.getStorage() == g.GrB_DENSE and labels.nvals() == gr.n
    info2, got = labels.extractTuples()
    assert info2 == 0
    _compare(name, info, res, got, want)
    return got, res


def _check(hb, gr, name="", dt=I, weighted=1, **kw):
    want = _model(gr, weighted, **kw)
    _run(hb, gr, _matrix(hb.g, gr, dt), want, weighted, name=name, **kw)
    return want


def _ring_of_cliques(cliques, size):
    u, v = [], []
    for q in range(cliques):
        base = q * size
        for i in range(size):
            for j in range(i + 1, size):
                u.append(base + i)
                v.append(base + j)
        u.append(base + size - 1)
        v.append(((q + 1) % cliques) * size)
    return Graph(cliques * size, u, v)


def _grid(h, w):
    idx = np.arange(h * w).reshape(h, w)
    return Graph(h * w, np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()]), np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()]))


def _path(n):
    a = np.arange(n - 1)
    return Graph(n, a, a + 1)


def _planted(rng, groups, size, p_in, p_out, weights=False):
    n = groups * size
    b = np.arange(n) // size
    m = np.triu(rng.random((n, n)) < np.where(b[:, None] == b[None, :], p_in, p_out), 1)
    u, v = np.nonzero(m)
    return Graph(n, u, v, rng.integers(1, 9, u.size) if weights else None)


# ---- structure ---------------------------------------------------------------------------------------------------------
def test_ring_of_cliques(hb):
    want = _check(hb, _ring_of_cliques(8, 5), "ring of cliques")
    assert want.communities == 8 and (want.labels == 5 * (np.arange(40) // 5)).all()


def test_grid(hb):
    want = _check(hb, _grid(30, 31), "grid")
    assert want.levels >= 2 and 1 < want.communities < 200


def test_path_all_gains_tie(hb):
    """every gain ties with its mirror image: the smallest-x and the smallest-v rules decide everything"""
    want = _check(hb, _path(500), "path")
    assert want.levels >= 3 and want.modularity > 0.8


def test_k33(hb):
    _check(hb, Graph(6, [0, 0, 0, 1, 1, 1, 2, 2, 2], [3, 4, 5, 3, 4, 5, 3, 4, 5]), "K3,3")


def test_planted_partition_of_two_levels(hb):
    rng = np.random.default_rng(1)
    want = _check(hb, _planted(rng, 8, 60, 0.25, 0.01), "planted")
    assert want.levels >= 3 and want.communities == 8 and want.modularity > 0.6


def test_two_components_and_isolated_vertices(hb):
    """a clique ring on 5 .. 44, a path on 50 .. 79, everything else isolated; vertex 2 stores only its diagonal"""
    ring = _ring_of_cliques(8, 5)
    half = ring.rows < ring.cols
    a = np.arange(29)
    gr = Graph(90, np.concatenate([ring.rows[half] + 5, 50 + a]), np.concatenate([ring.cols[half] + 5, 51 + a]), loops={2: 4})
    want = _check(hb, gr, "components")
    alone = np.r_[0:5, 45:50, 80:90]
    assert (want.labels[alone] == alone).all() and want.communities > 8 + alone.size


def test_degenerate(hb):
    g = hb.g
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    info, res = g.louvain(g.Vector(0, I), A0, 1, 3, 3, None)
    assert info == 0 and (res["levels"], res["rounds"], res["moves"], res["proposals"], res["communities"], res["qn"], res["w"]) == (1, 1, 0, 0, 0, 0, 0)
    assert res["modularity"] == 0.0
    none = np.zeros(0, np.int64)
    for dt in (F, I):
        for weighted in (0, 1):
            for gr in (Graph(1, none, none), Graph(1, none, none, loops={0: 3}), Graph(7, none, none),       # n = 1, no entries
                       Graph(7, none, none, loops={0: 2, 3: 0, 6: 5}),                                     # only a diagonal
                       Graph(5, [0, 1], [1, 2], [0, 0])):                                                  # W = 0 with entries
                want = _check(hb, gr, ("degenerate", gr.n, dt, weighted), dt=dt, weighted=weighted)
                if gr.rows.size == 0 or (weighted and gr.w.sum() == 0):
                    assert (want.levels, want.rounds, want.qn) == (1, 1, 0)
                if (gr.rows == gr.cols).all():
                    assert (want.labels == np.arange(gr.n)).all() and want.moves == 0


# ---- every row-length class of the propose pass ------------------------------------------------------------------------
def _hub_many(size):
    """a hub with `size` neighbours that pair up among themselves: at level 0 the hub's row sees `size` communities, then
    about size / 2.  Vertex 0 is a pendant of the first rim vertex, so the hub is not the smallest vertex"""
    rim = 2 + np.arange(size)
    even = rim[: size - size % 2: 2]
    u = np.concatenate([np.full(size, 1), even, [0]])
    v = np.concatenate([rim, even + 1, [2]])
    return Graph(size + 2, u, v), 1


def _hub_few(size):
    """the hub's neighbours hang on four heavy centres: after two rounds the hub's row sees four communities"""
    rim = 5 + np.arange(size)
    u = np.concatenate([np.zeros(size, np.int64), 1 + (rim % 4)])
    v = np.concatenate([rim, rim])
    w = np.concatenate([np.ones(size, np.int64), np.full(size, 6)])
    return Graph(size + 5, u, v, w), 0


SIZES = (LANE_LEN, LANE_LEN + 1, WAVE_LEN, WAVE_LEN + 1, SMALL_LEN, SMALL_LEN + 1, 512, 513, BLOCK_LEN, BLOCK_LEN + 1)


@pytest.mark.parametrize("size", SIZES)
def test_hub_over_many_communities(hb, size):
    gr, hub = _hub_many(size)
    assert np.diff(gr.ptr)[hub] == size
    _check(hb, gr, ("hub, many", size))


@pytest.mark.parametrize("size", SIZES)
def test_hub_over_few_communities(hb, size):
    gr, hub = _hub_few(size)
    assert np.diff(gr.ptr)[hub] == size and np.diff(gr.ptr)[1:5].min() >= size // 4
    want = _check(hb, gr, ("hub, few", size))
    assert len(want.trace[0]) >= 3


def test_two_long_rows_in_one_round(hb):
    """two hubs over the same 2100 rim vertices, a third of them with a stored zero to the second hub: both rows take the
    global-array route in every round, and the rim rows are lane rows"""
    size = 2100
    rim = 2 + np.arange(size)
    u = np.concatenate([np.zeros(size, np.int64), np.ones(size, np.int64), rim[:-1:2]])
    v = np.concatenate([rim, rim, rim[1::2]])
    w = np.concatenate([1 + rim % 3, np.where(rim % 3 == 0, 0, 2), np.full(size // 2, 3)])
    gr = Graph(size + 2, u, v, w, loops={0: 7})
    assert np.diff(gr.ptr)[0] == size + 1 and np.diff(gr.ptr)[1] == size
    _check(hb, gr, "two long rows")


# ---- the acceptance rule -----------------------------------------------------------------------------------------------
def test_star_of_2100_leaves_enters_in_one_round(hb):
    size = 2100
    gr = Graph(size + 1, np.zeros(size, np.int64), 1 + np.arange(size))
    want = _check(hb, gr, "star")
    assert [t[:2] for t in want.trace[0]] == [(size + 1, 1), (size - 1, size - 1), (0, 0)]
    assert want.communities == 1 and want.qn == 0


def test_heavy_leaves_some_entrants_rejected(hb):
    """leaves with heavy loops: g > k(v) (K(d) - k(v)) fails for some of those who enter the hub's community together"""
    rng = np.random.default_rng(3)
    m = 40
    ew = rng.integers(1, 6, m)
    lw = rng.integers(0, 40, m) * (rng.random(m) < 0.5)
    gr = Graph(m + 1, np.zeros(m, np.int64), 1 + np.arange(m), ew, loops={int(i + 1): int(x) for i, x in enumerate(lw) if x > 0})
    want = _check(hb, gr, "heavy leaves")
    assert any(1 < moves < proposals for proposals, moves, _ in want.trace[0])


def test_winner_that_leaves_bars_the_entrants(hb):
    """0 - 1 heavy, 0 - 2 light: 0 wins its own community as a leaver (to 1), so 2 may not enter it in that round"""
    gr = Graph(3, [0, 0], [1, 2], [5, 1])
    want = _check(hb, gr, "leaver")
    assert want.trace[0][0][:2] == (3, 1) and (want.labels == 0).all()


# ---- weights -----------------------------------------------------------------------------------------------------------
def test_weights_i32_f32_zeros_loops_and_unweighted(hb):
    g = hb.g
    rng = np.random.default_rng(4)
    base = _planted(rng, 6, 40, 0.3, 0.03, weights=True)
    half = base.rows < base.cols
    w = base.w[half].copy()
    w[rng.random(w.size) < 0.15] = 0                       # stored zeros
    gr = Graph(base.n, base.rows[half], base.cols[half], w, loops={int(x): int(rng.integers(0, 12)) for x in range(0, base.n, 9)})
    want = _model(gr)
    assert want.levels >= 2 and (gr.w == 0).sum() > 50
    outs = []
    for dt in (I, F):
        got, res = _run(hb, gr, _matrix(g, gr, dt), want, name=("weights", dt))
        outs.append((got.tobytes(), [res[x] for x in EXACT], res["modularity"]))
    assert outs[0] == outs[1]
    # -0.0 is +0.0, also when the two directions of an edge differ in the sign of their zero
    vals = gr.w.astype(F)
    zeros = np.flatnonzero(gr.w == 0)
    vals[zeros[::2]] = -0.0
    assert np.signbit(vals).sum() > 10
    _run(hb, gr, _matrix(g, gr, F, values=vals), want, name="negative zeros")
    # weighted = 0 on the same matrices never reads the values: a NaN, a negative and a fraction are fine
    unw = _model(gr, weighted=0)
    assert unw.w == gr.w.size and unw.qn != want.qn
    bad = vals.copy()
    bad[:3] = (np.nan, -2.0, 0.5)
    for A in (_matrix(g, gr, I), _matrix(g, gr, F, values=bad)):
        _run(hb, gr, A, unw, weighted=0, name="unweighted")


def test_triangle_with_w_just_below_two_to_the_31(hb):
    x = (2 ** 31 - 1) // 6
    gr = Graph(3, [0, 0, 1], [1, 2, 2], [x, x, x - 1])
    want = _check(hb, gr, "big triangle")
    assert want.w == 6 * x - 2 and 2 ** 31 - 8 < want.w <= 2 ** 31 - 1 and want.communities == 1
    gr = Graph(4, [0, 0, 1, 2], [1, 2, 2, 3], [x - 1, x - 2, x - 3, 5], loops={3: 1})
    want = _check(hb, gr, "big triangle and a tail")
    assert want.w > 2 ** 31 - 16


# ---- truncation ----------------------------------------------------------------------------------------------------------
def test_truncation(hb):
    rng = np.random.default_rng(5)
    gr = _planted(rng, 12, 30, 0.3, 0.01)
    A = _matrix(hb.g, gr)
    full = _model(gr)
    assert full.levels >= 3 and len(full.trace[0]) >= 3
    for kw in (dict(max_levels=1), dict(max_rounds=1), dict(max_levels=2, max_rounds=2), dict(max_levels=2)):
        want = _model(gr, **kw)
        assert want.levels <= kw.get("max_levels", BIG) and all(len(t) <= kw.get("max_rounds", BIG) for t in want.trace)
        _run(hb, gr, A, want, name=("truncated", kw), **kw)
    _run(hb, gr, A, full, name="full")


# ---- the state of labels beforehand, formats, storage --------------------------------------------------------------------
def test_labels_beforehand_csr_only_product_and_adopted(hb, monkeypatch):
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(6)
    gr = _planted(rng, 5, 50, 0.3, 0.02, weights=True)
    n = gr.n
    want = _model(gr)
    A = _matrix(g, gr)
    dense = g.Vector(n, I)
    assert dense.build(np.full(n, 9, I), n) == 0
    _run(hb, gr, A, want, labels=dense, name="dense labels")
    sparse = g.Vector(n, I)
    assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
    _run(hb, gr, A, want, labels=sparse, name="sparse labels")
    _run(hb, gr, A, want, labels=g.Vector(n, I), name="empty labels")
    for dt in (I, F):
        _run(hb, gr, _matrix(g, gr, dt, csr_only=True, monkeypatch=monkeypatch), want, name=("CSR only", dt))
    # a product result: S * S of the 0/1 structure is symmetric with small integer values and a diagonal; no CSC of its own
    S = _matrix(g, gr, F, values=np.ones(gr.w.size))
    P = g.Matrix(n, n, F)
    assert g.mxm(P, None, None, "PlusMultiplies", S, S, hb.descriptor()) == 0
    pp, pi, pv = P.host_csr()
    prod = Graph(n, [], [])
    prod.rows, prod.cols, prod.w = np.repeat(np.arange(n), np.diff(pp)).astype(np.int64), pi.astype(np.int64), pv.astype(np.int64)
    prod.ptr = pp.astype(np.int64)
    assert (pv == np.round(pv)).all() and (prod.rows == prod.cols).sum() > n // 2
    _run(hb, prod, P, _model(prod), name="product result")
    # caller-owned storage: A's arrays and labels at every 4-byte offset past a 16-byte boundary
    ptr, ind, val = gr.csr(I)
    for k in ad.KS:
        ks = (k, (k + 1) % 4, (k + 2) % 4)
        Aad, checks = ad.adopt_csr(g, (n, n), I, ptr, ind, val, ks)
        lab, t, check = ad.adopt_dense(g, np.full(n, 77, I), (k + 3) % 4)
        got, _ = _run(hb, gr, Aad, want, labels=lab, name=("adopted", k))
        assert np.array_equal(ad.payload(t, (k + 3) % 4, n, I), got)
        check(("louvain labels", k))
        for c in checks:
            c(("louvain A", k))


# ---- determinism -------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import graphblast_amd as g
d = np.load(sys.argv[2])
ptr, ind, val = d["ptr"], d["ind"], d["val"]
n = ptr.size - 1
A = g.Matrix(n, n, val.dtype.type)
assert A.build_csr(ptr, ind, val) == 0
lab = g.Vector(n, np.int32)
info, res = g.louvain(lab, A, 1, 1 << 30, 1 << 30, None)
assert info == 0, (info, res)
np.savez(sys.argv[3], labels=lab.extractTuples()[1], rec=np.array([res[x] for x in sys.argv[4].split(",")], np.int64),
         modularity=np.array([res["modularity"]]))
"""


def test_two_runs_and_a_child_on_four_cus_give_the_same_bits(hb, tmp_path):
    g = hb.g
    rng = np.random.default_rng(7)
    base = _planted(rng, 10, 50, 0.2, 0.01, weights=True)
    half = base.rows < base.cols
    hub = np.arange(1, 2300, dtype=np.int64) % base.n      # vertex 0 joined to everybody, with growing weights: a workgroup row
    hub = np.unique(hub[hub != 0])
    extra = np.setdiff1d(hub, base.cols[base.rows == 0])
    gr = Graph(base.n, np.concatenate([base.rows[half], np.zeros(extra.size, np.int64)]), np.concatenate([base.cols[half], extra]),
               np.concatenate([base.w[half], 1 + extra % 2]))
    want = _model(gr)
    A = _matrix(g, gr)
    outs = []
    for _ in range(2):
        got, res = _run(hb, gr, A, want, name="determinism")
        outs.append((got.tobytes(), [res[x] for x in EXACT], res["modularity"]))
    assert outs[0] == outs[1]
    ptr, ind, val = gr.csr(I)
    np.savez(tmp_path / "in.npz", ptr=ptr, ind=ind, val=val)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz"), ",".join(EXACT)],
                       env=dict(os.environ, GRB_NUM_CU="4"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    assert (out["labels"].tobytes(), out["rec"].tolist(), float(out["modularity"][0])) == outs[0]


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_labels_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(8)
    gr = _planted(rng, 4, 20, 0.4, 0.05, weights=True)
    n = gr.n
    ptr, ind, val = gr.csr(I)
    A = _matrix(g, gr)
    before = rng.integers(5, 1000, n).astype(I)
    lab = g.Vector(n, I)
    assert lab.build(before, n) == 0
    sv = g.Vector(n, I)                                   # a sparse labels stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0

    def unchanged():
        assert lab.getStorage() == g.GrB_DENSE and np.array_equal(lab.extractTuples()[1], before)
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
        info, si, sx = sv.extractTuples(sparse=True)
        return info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]

    def call(l_, a_, weighted=1, max_levels=10, max_rounds=10):
        return lib.grb_louvain(l_, a_, weighted, max_levels, max_rounds, None, None)

    def with_values(vals, dt):
        M = g.Matrix(n, n, dt)
        assert M.build_csr(ptr, ind, np.asarray(vals, dt)) == 0
        return M

    assert call(None, A._h) == g.GrB_UNINITIALIZED_OBJECT                             # null handles
    assert call(lab._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(lab._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT          # an unbuilt A
    R = g.Matrix(n, n + 1, I)                                                        # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(lab._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH             # size(labels) != n
    assert unchanged()
    fv = g.Vector(n, F)                                                              # labels not i32
    fbefore = rng.random(n).astype(F) + 2
    assert fv.build(fbefore, n) == 0
    assert call(fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(fv.extractTuples()[1].view(np.uint32), fbefore.view(np.uint32))
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                         # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(lab._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    for kw in (dict(weighted=2), dict(weighted=-1), dict(max_levels=0), dict(max_rounds=0), dict(max_rounds=-5)):
        for l_ in (lab, sv):
            assert call(l_._h, A._h, **kw) == g.GrB_INVALID_VALUE, kw
    assert unchanged()
    # bad weights: a negative i32; a fractional, a NaN, a negative, an infinite and a too large f32 -- each mirrored, so the
    # matrix stays symmetric and only the weight is wrong
    at = int(np.flatnonzero(gr.rows != gr.cols)[5])
    twin = int(np.flatnonzero((gr.rows == gr.cols[at]) & (gr.cols == gr.rows[at]))[0])
    for dt, x in ((I, -1), (F, 0.5), (F, np.nan), (F, -3.0), (F, np.inf), (F, 2.0 ** 24 + 2)):
        vals = gr.w.astype(dt)
        vals[[at, twin]] = x
        M = with_values(vals, dt)
        for l_ in (lab, sv):
            assert call(l_._h, M._h) == g.GrB_INVALID_VALUE, (dt, x)
        assert call(g.Vector(n, I)._h, M._h, weighted=0) == 0                        # the values are never read
    vals = gr.w.astype(F)
    vals[[at, twin]] = 2.0 ** 24                                                     # exactly 2^24 is allowed
    assert call(g.Vector(n, I)._h, with_values(vals, F)._h) == 0
    assert unchanged()
    # W = 2^31: one too many
    two = Graph(2, [0], [1], [2 ** 30])
    T = _matrix(g, two)
    l2 = g.Vector(2, I)
    assert l2.build(np.array([7, 8], I), 2) == 0
    assert lib.grb_louvain(l2._h, T._h, 1, 10, 10, None, None) == g.GrB_INVALID_VALUE
    assert l2.extractTuples()[1].tolist() == [7, 8]
    almost = Graph(2, [0], [1], [2 ** 30 - 1], loops={1: 1})                         # W = 2^31 - 1
    _check(hb, almost, "W = 2^31 - 1")
    # asymmetric values, and an asymmetric structure (with a CSC of their own)
    vals = gr.w.astype(I)
    vals[at] += 1
    Va = with_values(vals, I)
    assert call(lab._h, Va._h) == g.GrB_INVALID_VALUE
    assert call(g.Vector(n, I)._h, Va._h, weighted=0) == 0                           # ... which weighted = 0 never reads
    keep = np.ones(ind.size, bool)
    keep[at] = False
    rows = gr.rows[keep]
    ap = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ap[1:])
    D = g.Matrix(n, n, I)
    assert D.build_csr(ap.astype(I), ind[keep], val[keep]) == 0
    for weighted in (0, 1):
        for l_ in (lab, sv):
            assert call(l_._h, D._h, weighted=weighted) == g.GrB_INVALID_VALUE
    assert unchanged()
    # a descriptor and a null descriptor give the same result; the record is optional
    l1, l3 = g.Vector(n, I), g.Vector(n, I)
    assert lib.grb_louvain(l1._h, A._h, 1, BIG, BIG, hb.descriptor()._h, None) == 0 and lib.grb_louvain(l3._h, A._h, 1, BIG, BIG, None, None) == 0
    assert np.array_equal(l1.extractTuples()[1], l3.extractTuples()[1]) and np.array_equal(l1.extractTuples()[1], _model(gr).labels)


def test_csr_only_input_with_asymmetric_structure_returns(hb, monkeypatch):
    """an A without a CSC of its own is taken on the caller's word.  With a structure that is not symmetric the result is
    unspecified, but the call returns within max_rounds rounds a level and the labels are vertex numbers.  Every loop of the
    kernel is bounded, so this is an ordinary test of those bounds"""
    g = hb.g
    rng = np.random.default_rng(9)
    n = 50
    key = np.unique(rng.integers(0, n, 160) * n + rng.integers(0, n, 160))
    rows, cols = key // n, key % n
    ptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=ptr[1:])
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(n, n, I)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(ptr.astype(I), cols.astype(I), np.ones(key.size, I)) == 0
    lab = g.Vector(n, I)
    info, res = g.louvain(lab, A, 1, 4, 20, None)
    print("asymmetric structure, CSR only:", info, res)
    assert info == 0 and res["levels"] <= 4 and res["rounds"] <= 80 and res["w"] == key.size
    got = lab.extractTuples()[1]
    assert got.min() >= 0 and got.max() < n


# ---- the C++ frontend --------------------------------------------------------------------------------------------------
def _read_pattern_mtx(path):
    with open(path) as f:
        lines = [ln for ln in f if not ln.startswith("%")]
    n = int(lines[0].split()[0])
    e = np.array([[int(x) for x in ln.split()[:2]] for ln in lines[1:] if ln.strip()], np.int64) - 1
    return n, e[:, 0], e[:, 1]


def test_cpp_frontend(tmp_path):
    """tests/tools/louvain.cpp on chesapeake.mtx: the records and the labels of the weighted and the unweighted run"""
    exe = str(tmp_path / "louvain")
    subprocess.run(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "tools", "louvain.cpp"),
                    "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip", "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe],
                   check=True, timeout=300)
    path = os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    n, a, b = _read_pattern_mtx(path)
    keep = a != b
    lo, hi = np.minimum(a, b)[keep], np.maximum(a, b)[keep]
    key = np.unique(lo * n + hi)
    lo, hi = key // n, key % n
    gr = Graph(n, lo, hi, 1 + (lo + hi) % 3)
    assert lo.size == 170 and lines[-1] == "ok"
    for tag, ltag, want in (("weighted", "labels", _model(gr)), ("unweighted", "ulabels", _model(gr, weighted=0))):
        assert ("%s levels %d rounds %d moves %d proposals %d communities %d qn %d w %d launches %d"
                % (tag, want.levels, want.rounds, want.moves, want.proposals, want.communities, want.qn, want.w, want.levels)) in lines
        assert ltag + " " + " ".join(map(str, want.labels.tolist())) in lines
