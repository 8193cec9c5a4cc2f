"""Greedy weighted and maximal matching on the device (csrc/matching.hip: grb_matching) against the greedy scan in numpy under
the key of the definition in include/grb_hip.h: the edges sorted by np.lexsort((max, min, p)) and one loop that keeps an
edge when both ends are free.  Every comparison of mate, of C (pointers, indices, value BITS) and of edges / matched /
exposed / isolated / launches is EXACT.  weight is exact wherever the weights are integers below 2^24; for general floats
it is compared with math.fsum within matched x 2^-53 x sum |w|, the bound of an f64 summation in any order: derived, not
tuned.  Every result is also checked to be a matching and maximal.  Literal cases, ties and distinct weights in all three
modes and both element types with every special value, every row-length class of the kernel, a hub that loses its
candidate four rounds running, long dependency chains, more appends than a wave's LDS stage holds, components and
diagonals, degenerate shapes, the outputs' state beforehand, in place, the CSR-only format, caller-owned storage,
determinism (also in a child process on four CUs), every error code that can be asked for (a failed allocation and a
barrier that gives up cannot) with mate and C unchanged, an asymmetric input taken on the caller's word, RMAT-12 and the C++
frontend."""
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
from test_gpu_msf import Graph, _bits, _distinct_f32, _grid_edges, _matrix, _random_edges

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, I = np.float32, np.int32
HEAVIEST, LIGHTEST, HASHED = 0, 1, 2
MODES = (HEAVIEST, LIGHTEST, HASHED)
LANE_LEN = 8       # kMtLaneLen: a vertex whose CSR row has up to this many entries is walked by one lane
WAVE_LEN = 2048    # kMtWaveLen: ... up to this many by a wave, a longer one by the workgroup
STAGE = 256        # kMtStage: appends a wave stages in LDS before it reserves room for them
LAUNCHES = 1
REC = ("edges", "matched", "exposed", "isolated", "launches")


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- the reference -----------------------------------------------------------------------------------------------------
def _mix(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x.astype(np.uint64) * np.uint64(0x85ebca6b)).astype(np.uint32)
    x = x ^ (x >> np.uint32(13))
    x = (x.astype(np.uint64) * np.uint64(0xc2b2ae35)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def _priority(gr, mode, seed):
    """p of every edge: the smaller goes first"""
    if mode == HASHED:
        lo = ((gr.u + (seed & 0xffffffff)) & 0xffffffff).astype(np.uint32)
        return _mix(_mix(lo) ^ gr.v.astype(np.uint32))
    w = gr.w.astype(np.float64) if gr.dt is F else gr.w.astype(np.int64)    # -0.0 and +0.0 compare equal
    return -w if mode == HEAVIEST else w


def _greedy(gr, mode, seed):
    """-> mate, the indices of the matched edges (in key order)"""
    order = np.lexsort((gr.v, gr.u, _priority(gr, mode, seed)))
    mate = [-1] * gr.n
    keep = []
    uu, vv = gr.u[order].tolist(), gr.v[order].tolist()
    for k in range(len(uu)):
        a, b = uu[k], vv[k]
        if mate[a] < 0 and mate[b] < 0:
            mate[a], mate[b] = b, a
            keep.append(k)
    return np.asarray(mate, I), order[np.asarray(keep, np.int64)]


def _ref(gr, mode, seed=0):
    """-> mate, (C's pointers, indices, values), the record, the matched edges' indices"""
    mate, m = _greedy(gr, mode, seed)
    mw = gr.w[m]
    csr = gr.csr(gr.u[m], gr.v[m], mw, mw, diag=False)    # both directions hold the bits of the row of min(u, v)
    deg = np.bincount(np.concatenate([gr.u, gr.v]), minlength=gr.n) if gr.n else np.zeros(0, np.int64)
    rec = dict(edges=int(gr.u.size), matched=int(m.size), exposed=int(((deg > 0) & (mate < 0)).sum()), isolated=int((deg == 0).sum()),
               launches=LAUNCHES)
    assert rec["exposed"] + rec["isolated"] + 2 * rec["matched"] == gr.n
    return mate, csr, rec, m


def _check_weight(gr, m, got, name):
    w = gr.w[m]
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
        bound = m.size * 2.0 ** -53 * math.fsum(np.abs(w64).tolist())
        print(name, "weight", got, "fsum", want, "difference", abs(got - want), "bound", bound)
        assert abs(got - want) <= bound, (name, got, want, bound)


def _is_maximal_matching(gr, mate):
    n = gr.n
    on = np.flatnonzero(mate >= 0)
    assert (mate[on] < n).all() and np.array_equal(mate[mate[on]], on) and (mate[on] != on).all()
    edges = set((gr.u * n + gr.v).tolist())
    lo, hi = np.minimum(on, mate[on]), np.maximum(on, mate[on])
    assert set((lo.astype(np.int64) * n + hi).tolist()) <= edges              # every pair is an edge
    assert not ((mate[gr.u] < 0) & (mate[gr.v] < 0)).any()                     # no edge with two free ends


def _check(hb, gr, mode, seed=0, A=None, Cm="new", mate=None, name="", want=None):
    """grb_matching on gr against the reference, exactly; -> (mate's values, C's arrays, the record)"""
    g = hb.g
    n = gr.n
    if want is None:
        want = _ref(gr, mode, seed)
    wmate, (wp, wi, wv), rec, m = want
    if A is None:
        A = _matrix(g, gr)
    if isinstance(Cm, str):
        Cm = g.Matrix(n, n, gr.dt)
    if mate is None:
        mate = g.Vector(n, I)
    info, res = g.matching(mate, Cm, A, mode, seed, None)
    assert info == 0, (name, info)
    print(name, {x: res[x] for x in REC}, "weight", res["weight"], "rounds", res["rounds"], "passes", res["passes"], "evaluations",
          res["evaluations"], "loop_ms", res["loop_ms"])
    assert mate.getStorage() == g.GrB_DENSE and mate.nvals() == n
    info, got = mate.extractTuples()
    assert info == 0 and got.dtype == I
    bad = np.flatnonzero(got != wmate)
    assert bad.size == 0, (name, "mate", bad[:10], got[bad[:10]], wmate[bad[:10]])
    _is_maximal_matching(gr, got)
    for x in REC:
        assert res[x] == rec[x], (name, x, res, rec)
    arrays = None
    if Cm is not None:
        assert Cm.nvals() == 2 * rec["matched"]
        cp, ci, cv = arrays = Cm.host_csr()
        assert np.array_equal(cp, wp), (name, "pointers", np.flatnonzero(cp != wp)[:10])
        assert np.array_equal(ci, wi), (name, "indices", np.flatnonzero(ci != wi)[:10])
        assert cv.dtype == np.dtype(gr.dt) and np.array_equal(_bits(cv), _bits(wv)), (name, "values", np.flatnonzero(_bits(cv) != _bits(wv))[:10])
        assert (np.diff(cp) <= 1).all()
    _check_weight(gr, m, res["weight"], name)
    assert res["loop_ms"] >= 0 and res["passes"] >= 1 and res["rounds"] >= 0 and res["evaluations"] >= 0
    return got, arrays, res


# ---- literal cases -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
def test_path_2_3_2_keeps_the_middle_edge(hb, dt):
    """greedy is not maximum: the middle edge alone, weight 3 against 4"""
    gr = Graph(4, [0, 1, 2], [1, 2, 3], [2, 3, 2], dt)
    mate, _, res = _check(hb, gr, HEAVIEST, name="2 3 2")
    assert mate.tolist() == [-1, 2, 1, -1] and res["matched"] == 1 and res["weight"] == 3.0 and res["exposed"] == 2
    mate, _, res = _check(hb, gr, LIGHTEST, name="2 3 2 lightest")
    assert mate.tolist() == [1, 0, 3, 2] and res["weight"] == 4.0 and res["exposed"] == 0


@pytest.mark.parametrize("dt", [F, I])
def test_triangle_with_ties(hb, dt):
    """equal weights: the key falls back to the vertex numbers, {0, 1} first"""
    gr = Graph(3, [0, 0, 1], [1, 2, 2], [5, 5, 5], dt)
    for mode in (HEAVIEST, LIGHTEST):
        mate, _, res = _check(hb, gr, mode, name="triangle")
        assert mate.tolist() == [1, 0, -1] and res["exposed"] == 1
    gr = Graph(3, [0, 0, 1], [1, 2, 2], [5, 6, 6], dt)    # two heaviest: {0, 2} before {1, 2}
    assert _check(hb, gr, HEAVIEST, name="triangle 2")[0].tolist() == [2, -1, 0]


def test_two_seeds_on_a_six_cycle(hb):
    a = np.arange(6)
    gr = Graph(6, np.minimum(a, (a + 1) % 6), np.maximum(a, (a + 1) % 6), np.full(6, np.nan), F)   # the values are not read
    refs = {}
    for seed in range(40):
        refs.setdefault(tuple(_greedy(gr, HASHED, seed)[0].tolist()), seed)
    assert len(refs) >= 2
    seeds = sorted(refs.values())[:2]
    got = [_check(hb, gr, HASHED, seed=s, Cm=None, name=("six cycle", s))[0].tolist() for s in seeds]
    assert got[0] != got[1]
    big = 0xfffffff0                                      # min + seed wraps in 32 bits
    _check(hb, gr, HASHED, seed=big, Cm=None, name="six cycle, a large seed")


# ---- random graphs: ties, distinct weights, every special value ---------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("mode", MODES)
def test_random_graphs(hb, mode, dt):
    rng = np.random.default_rng(20 + mode)
    for n, m in ((301, 900), (1237, 9000), (2999, 7000)):
        assert n % 64
        u, v = _random_edges(rng, n, m)
        _check(hb, Graph(n, u, v, rng.integers(1, 5, u.size), dt), mode, seed=n, name=("ties", n, mode, dt.__name__))
        if dt is F:
            w = _distinct_f32(rng, u.size, 50.0)
        else:
            w = rng.choice(np.arange(-2 ** 31 + 1, 2 ** 31 - 1, 9973, dtype=np.int64), u.size, replace=False)
        _check(hb, Graph(n, u, v, w, dt), mode, seed=n + 1, name=("distinct", n, mode, dt.__name__))


@pytest.mark.parametrize("mode", MODES)
def test_f32_special_values(hb, mode):
    """-0.0 and +0.0 stored at the two directions of an edge (one weight: the endpoints decide; C holds the bits of the row of
    the smaller end both ways), +-inf, negatives and denormals.  The other weights lie mostly on the side of zero that
    makes the zeros good edges in the mode, so that many of them are matched"""
    rng = np.random.default_rng(30)
    n = 1501
    u, v = _random_edges(rng, n, 6000)
    w = _distinct_f32(rng, u.size, {HEAVIEST: -150.0, LIGHTEST: 150.0, HASHED: 20.0}[mode])
    assert (w < 0).sum() > 100 and (w > 0).sum() > 100
    w_rev = w.copy()
    at = rng.choice(u.size, 607, replace=False)
    special = [np.inf, -np.inf, 1e-45, -1e-45, 1e-40, -1e-40, np.inf] + [-0.0, 0.0] * 300
    for k, x in zip(at, special):
        w[k] = w_rev[k] = x
    w_rev[at[7::4]] = 0.0                                 # every other -0.0: +0.0 the other way round
    w_rev[at[8::4]] = -0.0                                # ... and every other +0.0: -0.0 the other way round
    gr = Graph(n, u, v, w, F, w_rev=w_rev)
    want = _ref(gr, mode, 3)
    matched = set(want[3].tolist())
    zeros = [int(k) for k in at[7:] if int(k) in matched]
    assert len(zeros) > 20 and set(at[7::4].tolist()) & matched and set(at[8::4].tolist()) & matched
    _, (cp, ci, cv), _ = _check(hb, gr, mode, seed=3, name=("special f32", mode), want=want)
    for k in zeros:
        a, b = int(gr.u[k]), int(gr.v[k])
        assert ci[cp[a]] == b and ci[cp[b]] == a
        assert _bits(cv[cp[a]:cp[a] + 1])[0] == _bits(cv[cp[b]:cp[b] + 1])[0] == _bits(np.array([w[k]], F))[0]


@pytest.mark.parametrize("mode", MODES)
def test_i32_extremes(hb, mode):
    rng = np.random.default_rng(31)
    n = 1501
    u, v = _random_edges(rng, n, 6000)
    w = rng.integers(-1000, 1000, u.size)
    w[rng.choice(u.size, 40, replace=False)] = np.repeat([-2 ** 31, 2 ** 31 - 1], 20)
    gr = Graph(n, u, v, w, I)
    want = _ref(gr, mode, 4)
    if mode != HASHED:
        first = want[3][0]
        assert gr.w[first] == (2 ** 31 - 1 if mode == HEAVIEST else -2 ** 31)
    _check(hb, gr, mode, seed=4, name=("extreme i32", mode), want=want)


# ---- the row-length classes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
def test_every_row_class_and_position(hb, dt):
    """hubs whose rows have 8, 9 (a lane / a wave), 2 048, 2 049 (a wave / the workgroup) and 2 100 entries, the best entry the
    first, the last or the middle one of the row.  Each hub's neighbours are shared with a second hub whose edges to them
    are all worse, so that the neighbours all choose the first hub and only its best entry is matched in the first round"""
    rng = np.random.default_rng(32)
    us, vs, ws, hubs = [], [], [], []
    base = 0
    for d in (LANE_LEN, LANE_LEN + 1, WAVE_LEN, WAVE_LEN + 1, 2100):
        for where in ("first", "last", "middle"):
            nb = base + np.arange(d)
            x, y = base + d, base + d + 1                 # numbered past their neighbours: positions = neighbour numbers
            pick = {"first": 0, "last": d - 1, "middle": d // 2 + 1}[where]
            wx = 10000 + rng.permutation(d)
            wx[pick] = 50000
            us += [np.full(d, x), np.full(d, y)]
            vs += [nb, nb]
            ws += [wx, 1 + rng.permutation(d)]
            hubs.append((x, int(nb[pick])))
            base += d + 2
    u, v, w = np.concatenate(us), np.concatenate(vs), np.concatenate(ws)
    gr = Graph(base, u, v, w, dt)
    rows = np.diff(gr.csr()[0])
    assert sorted(set(rows[[h for h, _ in hubs]].tolist())) == [LANE_LEN, LANE_LEN + 1, WAVE_LEN, WAVE_LEN + 1, 2100]
    mate, _, _ = _check(hb, gr, HEAVIEST, name=("classes", dt.__name__))
    for h, best in hubs:
        assert mate[h] == best
    _check(hb, Graph(base, u, v, -w, dt), LIGHTEST, name=("classes, lightest", dt.__name__))
    _check(hb, gr, HASHED, seed=9, name=("classes, hashed", dt.__name__))


def test_hub_loses_its_candidate_four_rounds_running(hb):
    """hub h of degree 2 100; w(h, u_i) = 1000 - i for i = 1..4, and u_i heads a path of 2 i - 1 edges whose weights rise away
    from h, all above 2000: u_i is taken in round i, by its path.  The other neighbours of h are leaves of weight 1..10,
    and h ends with the heaviest leaf (the smallest number among those of weight 10)"""
    rng = np.random.default_rng(33)
    deg = 2100
    h = 0
    us, vs, ws = [], [], []
    nxt = 1
    heads = []
    for i in range(1, 5):
        ui = nxt
        nxt += 1
        heads.append(ui)
        us.append(h), vs.append(ui), ws.append(1000 - i)
        prev = ui
        for j in range(2 * i - 1):
            us.append(prev), vs.append(nxt), ws.append(2001 + 10 * i + j)
            prev = nxt
            nxt += 1
    leaves = np.arange(nxt, nxt + deg - 4)
    lw = rng.integers(1, 11, leaves.size)
    n = int(leaves[-1]) + 1
    perm = rng.permutation(n)                             # the hub anywhere
    u = perm[np.concatenate([np.asarray(us), np.full(leaves.size, h)])]
    v = perm[np.concatenate([np.asarray(vs), leaves])]
    w = np.concatenate([np.asarray(ws), lw])
    for dt in (F, I):
        gr = Graph(n, u, v, w, dt)
        assert np.diff(gr.csr()[0])[perm[h]] == deg
        mate, _, res = _check(hb, gr, HEAVIEST, name=("hub", dt.__name__))
        heavy = perm[leaves[lw == 10]]
        assert mate[perm[h]] == heavy.min() and all(mate[perm[x]] == perm[x + 1] for x in heads)
        assert res["rounds"] >= 5 and res["evaluations"] >= n - 1 + 4


# ---- long dependency chains --------------------------------------------------------------------------------------------
def test_equal_weight_path_and_grid(hb):
    """equal weights: the key falls back to vertex numbers, and a path is matched one edge a round from its low end"""
    n = 3001
    a = np.arange(n - 1)
    for dt, mode in ((F, HEAVIEST), (I, LIGHTEST)):
        mate, _, res = _check(hb, Graph(n, a, a + 1, np.full(n - 1, 7), dt), mode, name=("path", dt.__name__))
        assert np.array_equal(mate[0:n - 1:2], np.arange(1, n, 2)) and mate[n - 1] == -1
        assert res["matched"] == 1500 and res["weight"] == 7.0 * 1500 and res["rounds"] >= 1500
    u, v = _grid_edges(60)
    _, _, res = _check(hb, Graph(3600, u, v, np.ones(u.size), F), HEAVIEST, name="grid")
    assert res["rounds"] >= 30                            # its first row alone is such a path


def test_more_appends_than_the_lds_stage(hb):
    """n = 70 000: the pairs (2 i, 2 i + 1) with weight 100 and light edges between them.  Everything is matched in the first
    round: on four CUs every wave appends more than its stage holds"""
    gr = _stage_graph()
    mate, _, res = _check(hb, gr, HEAVIEST, name="stage")
    assert np.array_equal(mate, np.arange(gr.n) ^ 1) and res["matched"] == gr.n // 2 and res["rounds"] == 1
    assert gr.n / (4 * 16) > 2 * STAGE


def _stage_graph():
    n = 70000
    a = np.arange(n - 1)
    return Graph(n, a, a + 1, np.where(a % 2 == 0, 100, 1 + a % 7), I)


# ---- structure ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("mode", MODES)
def test_components_isolated_vertices_and_diagonals(hb, mode, dt):
    """200 components of random size, 300 isolated vertices of which every third stores its diagonal, diagonal entries on a
    tenth of the others with the best weight of all (a NaN for f32): all of which must be ignored"""
    rng = np.random.default_rng(34)
    n = 2500
    label = rng.permutation(np.concatenate([rng.integers(0, 200, n - 300), np.full(300, -1)]))
    us, vs = [], []
    for c in range(200):
        mem = np.flatnonzero(label == c)
        if mem.size > 1:
            a, b = _random_edges(rng, mem.size, 2 * mem.size)
            us.append(mem[a])
            vs.append(mem[b])
    u, v = np.concatenate(us), np.concatenate(vs)
    iso = np.flatnonzero(label == -1)
    dg = np.concatenate([iso[::3], np.flatnonzero(label >= 0)[::10]])
    dv = np.full(dg.size, np.nan if dt is F else (2 ** 31 - 1 if mode == HEAVIEST else -2 ** 31))
    gr = Graph(n, u, v, rng.integers(-50, 50, u.size), dt, diag=(dg, dv))
    want = _ref(gr, mode, 11)
    assert want[2]["isolated"] >= 300 and want[2]["exposed"] > 0
    mate, (cp, _, _), _ = _check(hb, gr, mode, seed=11, name=("components", mode, dt.__name__), want=want)
    assert (mate[iso] == -1).all() and (np.diff(cp)[iso] == 0).all()


def test_degenerate(hb):
    g = hb.g
    A0 = g.Matrix(0, 0, F)
    assert A0.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F)) == 0
    C0, v0 = g.Matrix(0, 0, F), g.Vector(0, I)
    info, res = g.matching(v0, C0, A0, HEAVIEST, 0, None)
    assert info == 0 and all(res[x] == 0 for x in REC) and res["weight"] == 0 and res["rounds"] == 0 and C0.nvals() == 0
    assert res["evaluations"] == 0 and res["passes"] == 0
    none = np.zeros(0, np.int64)
    for n, diag in ((1, None), (1, ([0], [5])), (50, None), (50, (np.arange(0, 50, 3), np.full(17, -4)))):
        for dt in (F, I):
            for mode in MODES:
                gr = Graph(n, none, none, none, dt, diag=diag)
                mate, (cp, ci, _), res = _check(hb, gr, mode, name=("no edges", n))
                assert (mate == -1).all() and res["isolated"] == n and res["weight"] == 0 and res["edges"] == 0 and ci.size == 0
    mate, _, res = _check(hb, Graph(300, [3, 5, 3, 7], [5, 7, 7, 200], [2, 1, 3, 0], I), LIGHTEST, name="a triangle, a tail and a stored zero")
    assert mate[7] == 200 and mate[3] == 5 and res["matched"] == 2 and res["weight"] == 2.0 and res["isolated"] == 296


# ---- the outputs' state beforehand, aliasing, formats -------------------------------------------------------------------
def test_outputs_prefilled_null_in_place_and_csr_only(hb, monkeypatch):
    g = hb.g
    rng = np.random.default_rng(35)
    n = 700
    u, v = _random_edges(rng, n, 2500)
    gr = Graph(n, u, v, _distinct_f32(rng, u.size), F)
    want = _ref(gr, HEAVIEST)
    A = _matrix(g, gr)
    ou, ov = _random_edges(rng, n, 4000)
    Cfull = _matrix(g, Graph(n, ou, ov, np.ones(ou.size), F))   # a C that holds something else
    dense = g.Vector(n, I)
    assert dense.build(np.full(n, 9, I), n) == 0
    _check(hb, gr, HEAVIEST, A=A, Cm=Cfull, mate=dense, name="prefilled", want=want)
    sparse = g.Vector(n, I)
    assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
    _check(hb, gr, HEAVIEST, A=A, mate=sparse, name="sparse mate", want=want)
    _check(hb, gr, HEAVIEST, A=A, Cm=None, name="null C", want=want)
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Conly = g.Matrix(n, n, F)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    _check(hb, gr, HEAVIEST, A=A, Cm=Conly, name="C CSR only", want=want)
    Aonly = _matrix(g, gr, csr_only=True, monkeypatch=monkeypatch)
    _, (cp, ci, cv), _ = _check(hb, gr, HEAVIEST, A=Aonly, name="A CSR only", want=want)
    C = g.Matrix(n, n, F)                                 # both orientations: the CSC is the CSR
    assert g.matching(g.Vector(n, I), C, A, HEAVIEST, 0, None)[0] == 0
    for got, ref in zip(C.host_csc(), (cp, ci, cv)):
        assert np.array_equal(_bits(got) if got.dtype == F else got, _bits(ref) if ref.dtype == F else ref)
    _check(hb, gr, HEAVIEST, A=A, Cm=A, name="in place", want=want)   # last: A is its own matching now
    m = want[3]
    _check(hb, Graph(n, gr.u[m], gr.v[m], gr.w[m], F), LIGHTEST, A=A, name="the matching's matching")


def test_mate_on_caller_owned_storage(hb):
    """mate adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(36)
    n = 1003
    u, v = _random_edges(rng, n, 1500)
    gr = Graph(n, u, v, rng.integers(1, 9, u.size), I)
    want = _ref(gr, HEAVIEST)
    A = _matrix(g, gr)
    for k in ad.KS:
        mate, t, check = ad.adopt_dense(g, np.full(n, 77, I), k)
        assert mate.device_ptrs()[2] % 16 == 4 * k
        got, _, _ = _check(hb, gr, HEAVIEST, A=A, mate=mate, Cm=None, name=("adopted", k), want=want)
        assert np.array_equal(ad.payload(t, k, n, I), got)
        check(("matching", k))


# ---- determinism -------------------------------------------------------------------------------------------------------
CHILD = r"""
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import graphblast_amd as g
d = np.load(sys.argv[2])
out = {}
for name in ("a", "b"):
    ptr, ind, val = d[name + "_ptr"], d[name + "_ind"], d[name + "_val"]
    n = ptr.size - 1
    A = g.Matrix(n, n, val.dtype.type)
    assert A.build_csr(ptr, ind, val) == 0
    mate = g.Vector(n, np.int32)
    info, res = g.matching(mate, None, A, int(d[name + "_mode"]), 5, None)
    assert info == 0 and res["launches"] == 1, (info, res)
    out[name] = mate.extractTuples()[1]
np.savez(sys.argv[3], **out)
"""


def test_three_runs_and_a_child_on_four_cus_give_the_same_bits(hb, tmp_path):
    g = hb.g
    rng = np.random.default_rng(37)
    n = 30001
    u, v = _random_edges(rng, n, 150000)
    gr = Graph(n, u, v, (rng.integers(1, 40, u.size) / 8 + 0.001).astype(F), F)     # non-integer weights, ties among them
    want = _ref(gr, HEAVIEST, 5)
    A = _matrix(g, gr)
    outs = []
    for _ in range(3):
        mate, (cp, ci, cv), res = _check(hb, gr, HEAVIEST, seed=5, A=A, name="determinism", want=want)
        outs.append((mate.tobytes(), cp.tobytes(), ci.tobytes(), cv.tobytes(), [res[x] for x in REC], np.float64(res["weight"]).tobytes()))
    assert outs[0] == outs[1] == outs[2]
    st = _stage_graph()
    data = {}
    for name, x, mode in (("a", gr, HEAVIEST), ("b", st, HEAVIEST)):
        data[name + "_ptr"], data[name + "_ind"], data[name + "_val"] = x.csr()
        data[name + "_mode"] = mode
    np.savez(tmp_path / "in.npz", **data)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, GRB_NUM_CU="4")
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    assert np.array_equal(out["a"], want[0])
    assert np.array_equal(out["b"], np.arange(st.n) ^ 1)


# ---- errors ------------------------------------------------------------------------------------------------------------
def test_errors_leave_mate_and_c_unchanged(hb):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(38)
    n = 80
    u, v = _random_edges(rng, n, 300)
    gr = Graph(n, u, v, rng.integers(1, 9, u.size), F)
    A = _matrix(g, gr)
    ptr, ind, val = gr.csr()
    Cm = _matrix(g, Graph(n, u[:50], v[:50], np.arange(50) + 1, F))
    cbefore = Cm.host_csr()
    before = rng.integers(5, 1000, n).astype(I)
    mate = g.Vector(n, I)
    assert mate.build(before, n) == 0
    sv = g.Vector(n, I)                                   # a sparse mate stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0

    def unchanged():
        now = Cm.host_csr()
        assert Cm.nvals() == 100 and all(np.array_equal(x, y) for x, y in zip(now, cbefore))
        assert mate.getStorage() == g.GrB_DENSE and np.array_equal(mate.extractTuples()[1], before)
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
        info, si, sx = sv.extractTuples(sparse=True)
        return info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]

    def call(m_, c, a, mode=0, seed=0):
        return lib.grb_matching(m_, c, a, mode, seed, None, None)

    assert call(None, Cm._h, A._h) == g.GrB_UNINITIALIZED_OBJECT                     # null handles
    assert call(mate._h, Cm._h, None) == g.GrB_UNINITIALIZED_OBJECT
    assert call(mate._h, Cm._h, g.Matrix(n, n, F)._h) == g.GrB_UNINITIALIZED_OBJECT  # an unbuilt A
    R = g.Matrix(n, n + 1, F)                                                        # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(mate._h, Cm._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(mate._h, g.Matrix(n, n + 1, F)._h, A._h) == g.GrB_DIMENSION_MISMATCH   # C not n x n
    assert call(mate._h, g.Matrix(n + 1, n, F)._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Vector(n + 1, I)._h, Cm._h, A._h) == g.GrB_DIMENSION_MISMATCH      # size(mate) != n
    assert unchanged()
    fv = g.Vector(n, F)                                                              # a mate that is not i32
    fbefore = rng.random(n).astype(F) + 2
    assert fv.build(fbefore, n) == 0
    assert call(fv._h, Cm._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(_bits(fv.extractTuples()[1]), _bits(fbefore))
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                         # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(mate._h, None, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    Ci = _matrix(g, Graph(n, u[:50], v[:50], np.arange(50) + 1, I))                  # C not of A's type
    cibefore = Ci.host_csr()
    assert call(mate._h, Ci._h, A._h) == g.GrB_DOMAIN_MISMATCH
    assert all(np.array_equal(x, y) for x, y in zip(Ci.host_csr(), cibefore))
    for mode in (-1, 3, 7):                                                          # a bad mode
        assert call(mate._h, Cm._h, A._h, mode) == g.GrB_INVALID_VALUE
    assert unchanged()
    # an asymmetric structure (with a CSC of its own): every mode
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
    grn = Graph(n, gr.u, gr.v, wn, F)
    Nm = _matrix(g, grn)
    for M, modes in ((Dm, MODES), (Vm, (HEAVIEST, LIGHTEST)), (Nm, (HEAVIEST, LIGHTEST))):
        for mode in modes:
            for m_ in (mate, sv):
                for c_ in (Cm, None):
                    assert call(m_._h, c_._h if c_ is not None else None, M._h, mode) == g.GrB_INVALID_VALUE
                    assert unchanged()
    # the hashed mode reads no value: asymmetric values and a NaN are accepted
    mh = g.Vector(n, I)
    info, res = g.matching(mh, None, Vm, HASHED, 2, None)
    assert info == 0 and np.array_equal(mh.extractTuples()[1], _greedy(gr, HASHED, 2)[0])
    _check(hb, grn, HASHED, seed=2, A=Nm, name="a NaN, hashed")
    # a NaN on the diagonal is no weight; -0.0 against +0.0 is no asymmetry
    wz = gr.w.copy()
    wz[3] = -0.0
    wr = wz.copy()
    wr[3] = 0.0
    ok = Graph(n, gr.u, gr.v, wz, F, w_rev=wr, diag=([4, 9], [np.nan, np.nan]))
    for mode in MODES:
        _check(hb, ok, mode, name="NaN on the diagonal")
    # a descriptor and a null descriptor give the same result; the record is optional
    C1, C2 = g.Matrix(n, n, F), g.Matrix(n, n, F)
    m1, m2 = g.Vector(n, I), g.Vector(n, I)
    assert lib.grb_matching(m1._h, C1._h, A._h, 0, 0, hb.descriptor()._h, None) == 0 and lib.grb_matching(m2._h, C2._h, A._h, 0, 9, None, None) == 0
    assert all(np.array_equal(x, y) for x, y in zip(C1.host_csr(), C2.host_csr()))
    assert np.array_equal(m1.extractTuples()[1], m2.extractTuples()[1])              # seed is ignored in mode 0


def test_csr_only_asymmetric_input_returns(hb, monkeypatch):
    """an A without a CSC of its own is taken on the caller's word.  With an asymmetric structure the result is unspecified,
    but the call returns with in-range mate values or -1.  Every loop of the kernel is bounded, so this is an ordinary test
    of those bounds"""
    g = hb.g
    rng = np.random.default_rng(39)
    n = 2000
    D = sp.csr_matrix((rng.integers(1, 4, 9000).astype(F), (rng.integers(0, n, 9000), rng.integers(0, n, 9000))), shape=(n, n))
    D.sum_duplicates()
    D.sort_indices()
    assert (D != D.T).nnz > 0
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(n, n, F)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(D.indptr.astype(I), D.indices.astype(I), D.data.astype(F)) == 0
    for mode in MODES:
        mate, Cm = g.Vector(n, I), g.Matrix(n, n, F)
        info, res = g.matching(mate, Cm, A, mode, 1, None)
        print("asymmetric, CSR only:", mode, info, res)
        assert isinstance(info, int)
        if info == 0:
            got = mate.extractTuples()[1]
            assert got.size == n and (got >= -1).all() and (got < n).all()
            assert res["launches"] == LAUNCHES and res["rounds"] <= n // 2 + 1


# ---- scale and the C++ frontend ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_rmat_12(hb, mode):
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(12, 16, seed=1)
    ptr, ind = finalize_edges(s, d, n, symmetrize=True)["csr"]
    rows = np.repeat(np.arange(n), np.diff(ptr))
    up = rows < ind
    rng = np.random.default_rng(40)
    for dt in (I, F):
        gr = Graph(n, rows[up], ind[up], rng.integers(1, 65, int(up.sum())), dt)
        _, _, res = _check(hb, gr, mode, seed=12, name=("RMAT-12", mode, dt.__name__))
        assert res["edges"] == int(up.sum())


def test_cpp_frontend(tmp_path):
    """tests/tools/matching.cpp on chesapeake.mtx with the weights 1 + (min + 3 max) % 7: the record, mate in all three modes and
    C against the greedy scan"""
    exe = str(tmp_path / "matching")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "matching.cpp"),
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
    u, v = key // n, key % n
    gr = Graph(n, u, v, 1 + (u + 3 * v) % 7, F)
    mate, (wp, wi, wv), rec, m = _ref(gr, HEAVIEST)
    assert rec["edges"] == 170
    assert lines[-1] == "ok"
    assert "heaviest edges 170 matched %d weight %d exposed %d isolated 0 launches 1" % (rec["matched"], int(gr.w[m].sum()), rec["exposed"]) in lines
    assert "mate " + " ".join(map(str, mate.tolist())) in lines
    assert "csr | " + " ".join(map(str, wp.tolist())) + " | " + " ".join(map(str, wi.tolist())) + " | " + " ".join("%g" % x for x in wv.tolist()) in lines
    assert "lightest mate " + " ".join(map(str, _greedy(gr, LIGHTEST, 0)[0].tolist())) in lines
    assert "hashed mate " + " ".join(map(str, _greedy(gr, HASHED, 5)[0].tolist())) in lines
