"""Maximum flow and minimum cut on the device (csrc/maxflow.hip: grb_maxflow) against scipy.sparse.csgraph.maximum_flow on the
host.  scipy's flow_value is the value; the reference side is a numpy backward reachability from the sink in the residual
graph of scipy's flow, a set that does not depend on which maximum flow scipy found.  Every comparison is EXACT, there is no
tolerance anywhere: value, side, sink_side, cut_arcs, arcs, cut_capacity == value and launches == 1 on every case.  F is not
compared with scipy's flow (a maximum flow is not unique) but checked by a numpy validity function: its structure is a
subset of A's off-diagonal structure with columns ascending, 0 < F <= capacity, never both directions, conservation at every
non-terminal, net outflow of the source = net inflow of the sink = value, no arc from side 0 to side 1 unsaturated, no arc
from side 1 to side 0 with flow, the CSC equal to the transposed CSR, flow_arcs == nvals(F).  Literal networks, 200 random
networks, every row-length class of the kernel's walkers as the source's, the sink's and a hub's row, a value past 2^32,
excess that must come back to the source, more appends than a wave's LDS stage holds, the unit mode against the maximum
bipartite matching, bad capacities, degenerate shapes, the outputs' state beforehand, in place, the CSR-only format,
caller-owned storage, determinism (also in a child process on four CUs), every error code that can be asked for (a failed
allocation and a barrier that gives up cannot) with F and side unchanged, RMAT-12 and the C++ frontend."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.io
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, maximum_bipartite_matching, maximum_flow

from backends import HipBackend

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, I = np.float32, np.int32
CAPACITY, UNIT = 0, 1
LANE_LEN = 8       # kMfLaneLen: a vertex whose residual row has up to this many slots is walked by one lane
WAVE_LEN = 2048    # kMfWaveLen: ... up to this many by a wave, a longer one by the workgroup
STAGE = 256        # kMfStage: appends a wave stages in LDS before it reserves room for them
EXACT = ("value", "arcs", "flow_arcs", "sink_side", "cut_arcs", "cut_capacity", "launches")


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


# ---- networks and the reference ------------------------------------------------------------------------------------------
class Net:
    """a network: the stored entries (i, j, c), diagonal and zeros included, at most one per (i, j); caps: what the mode
    makes of the off-diagonal ones, as int64"""

    def __init__(self, n, i, j, c, dt=I, unit=False):
        self.n, self.dt, self.unit = int(n), dt, unit
        i, j = np.asarray(i, np.int64), np.asarray(j, np.int64)
        order = np.lexsort((j, i))
        self.i, self.j, self.c = i[order], j[order], np.asarray(c)[order].astype(dt)
        assert np.unique(self.i * max(self.n, 1) + self.j).size == self.i.size
        self.ptr = np.zeros(self.n + 1, I)
        np.cumsum(np.bincount(self.i, minlength=self.n), out=self.ptr[1:])
        self.off = self.i != self.j
        with np.errstate(invalid="ignore"):               # (a bad capacity is never compared: the call is rejected)
            self.caps = np.ones(self.i.size, np.int64) if unit else self.c.astype(np.float64).astype(np.int64)

    def csr(self):
        return self.ptr, self.j.astype(I), self.c

    def capacity_matrix(self):
        keep = self.off & (self.caps > 0)
        return sp.csr_matrix((self.caps[keep], (self.i[keep], self.j[keep])), shape=(self.n, self.n))


def _matrix(g, net, csr_only=False, monkeypatch=None):
    if csr_only:
        monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    A = g.Matrix(net.n, net.n, net.dt)
    if csr_only:
        monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    assert A.build_csr(*net.csr()) == 0
    return A


def _reaches(R, t):
    """the vertices from which t is reached over the entries of R (a 0/1 vector)"""
    n = R.shape[0]
    side = np.zeros(n, I)
    side[breadth_first_order(sp.csr_matrix(R.T), t, directed=True, return_predecessors=False)] = 1
    return side


def _ref(net, s, t, value=None):
    """-> (value, side, the record's exact fields but flow_arcs).  value given: capacities past what scipy's int32 sums hold;
    the side then comes from the caller too (a tuple (value, side))"""
    Cm = net.capacity_matrix()
    if value is None:
        if Cm.nnz:
            res = maximum_flow(Cm.astype(I), s, t)
            value = int(res.flow_value)
            R = (Cm - res.flow).tocsr()                     # scipy's flow is antisymmetric: the reverse arcs' residuals are in it
            R.data = (R.data > 0).astype(np.int8)
            R.eliminate_zeros()
            side = _reaches(R, t)
        else:
            value, side = 0, np.zeros(net.n, I)
            side[t] = 1
    else:
        value, side = value
    assert side[t] == 1 and side[s] == 0
    cut = net.off & (side[net.i] == 0) & (side[net.j] == 1)
    rec = dict(value=value, arcs=int(net.off.sum()), sink_side=int(side.sum()), cut_arcs=int(cut.sum()), cut_capacity=int(net.caps[cut].sum()),
               launches=1)
    assert rec["cut_capacity"] == value
    return value, side, rec


def _valid_flow(net, s, t, value, side, Fm, res, name):
    """F is a maximum flow in cancelled form, and it agrees with the cut"""
    n = net.n
    fp, fi, fv = Fm.host_csr()
    assert fv.dtype == np.dtype(net.dt)
    assert res["flow_arcs"] == Fm.nvals() == fi.size == fp[-1], (name, res["flow_arcs"], Fm.nvals())
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(fp))
    key = rows * n + fi
    assert (np.diff(key) > 0).all(), (name, "columns ascending, no duplicates")
    akey = (net.i * n + net.j)[net.off]
    acap = net.caps[net.off]
    at = np.searchsorted(akey, key)
    assert (at < akey.size).all() and (akey[np.minimum(at, akey.size - 1)] == key).all(), (name, "structure within A's, off the diagonal")
    f = fv.astype(np.float64).astype(np.int64)
    assert (f.astype(net.dt) == fv).all() and (f > 0).all() and (f <= acap[at]).all(), (name, "0 < F <= capacity")
    assert not np.isin(fi.astype(np.int64) * n + rows, key).any(), (name, "both directions")
    net_out = np.bincount(rows, weights=f, minlength=n) - np.bincount(fi, weights=f, minlength=n)
    inner = np.ones(n, bool)
    inner[[s, t]] = False
    assert (net_out[inner] == 0).all(), (name, "conservation", np.flatnonzero(inner & (net_out != 0))[:10])
    assert net_out[s] == value and net_out[t] == -value, (name, net_out[s], net_out[t], value)
    flow_on = np.zeros(akey.size, np.int64)
    flow_on[at] = f
    ai, aj = net.i[net.off], net.j[net.off]
    fwd = (side[ai] == 0) & (side[aj] == 1)
    assert (flow_on[fwd] == acap[fwd]).all(), (name, "an unsaturated arc across the cut")
    assert (flow_on[(side[ai] == 1) & (side[aj] == 0)] == 0).all(), (name, "flow back across the cut")
    if not Fm_csr_only(Fm):
        cp, ci, cv = Fm.host_csc()
        T = sp.csr_matrix((f, fi, fp), shape=(n, n)).T.tocsr()
        T.sort_indices()
        assert np.array_equal(cp, T.indptr) and np.array_equal(ci, T.indices) and np.array_equal(cv.astype(np.float64).astype(np.int64), T.data), name
    return fp, fi, fv


def Fm_csr_only(Fm):
    return getattr(Fm, "_csr_only", False)


def _check(hb, net, s, t, A=None, Fm="new", side="new", name="", want=None, mode=None):
    """grb_maxflow on net against the reference, exactly; -> (side's values or None, F's arrays or None, the record)"""
    g = hb.g
    n = net.n
    if want is None:
        want = _ref(net, s, t)
    value, wside, rec = want
    if A is None:
        A = _matrix(g, net)
    if isinstance(Fm, str):
        Fm = g.Matrix(n, n, net.dt)
    if isinstance(side, str):
        side = g.Vector(n, I)
    if mode is None:
        mode = UNIT if net.unit else CAPACITY
    info, res = g.maxflow(Fm, side, A, s, t, mode, None)
    assert info == 0, (name, info)
    print(name, {x: res[x] for x in EXACT}, "rounds", res["rounds"], "global_relabels", res["global_relabels"], "passes", res["passes"],
          "loop_ms", res["loop_ms"])
    for x in rec:
        assert res[x] == rec[x], (name, x, res, rec)
    assert res["cut_capacity"] == res["value"] == value and res["launches"] == 1
    got = None
    if side is not None:
        assert side.getStorage() == g.GrB_DENSE and side.nvals() == n
        info, got = side.extractTuples()
        assert info == 0 and got.dtype == I
        bad = np.flatnonzero(got != wside)
        assert bad.size == 0, (name, "side", bad[:10], got[bad[:10]], wside[bad[:10]])
    arrays = None
    if Fm is not None:
        arrays = _valid_flow(net, s, t, value, wside, Fm, res, name)
    else:
        assert res["flow_arcs"] == -1
    assert res["loop_ms"] >= 0 and res["passes"] >= 1 and res["rounds"] >= 0 and res["global_relabels"] >= 1
    return got, arrays, res


def _both(hb, net, s, t, name="", want=None):
    """with F and without: value and side are identical either way"""
    if want is None:
        want = _ref(net, s, t)
    A = _matrix(hb.g, net)
    s1, arrays, r1 = _check(hb, net, s, t, A=A, name=(name, "F"), want=want)
    s2, _, r2 = _check(hb, net, s, t, A=A, Fm=None, name=(name, "no F"), want=want)
    assert np.array_equal(s1, s2) and all(r1[x] == r2[x] for x in EXACT if x != "flow_arcs")
    return arrays, r1, r2


# ---- literal networks ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, I])
def test_four_vertices_value_five(hb, dt):
    """0 -> 1 (3), 0 -> 2 (2), 1 -> 2 (5), 1 -> 3 (2), 2 -> 3 (3): value 5, every arc at a terminal saturated: the sink alone on its side"""
    net = Net(4, [0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [3, 2, 5, 2, 3], dt)
    want = _ref(net, 0, 3)
    assert want[0] == 5 and want[1].tolist() == [0, 0, 0, 1]
    _both(hb, net, 0, 3, "four", want)
    unit = Net(4, [0, 0, 1, 1, 2], [1, 2, 2, 3, 3], [3, 2, 5, 2, 3], dt, unit=True)
    assert _ref(unit, 0, 3)[0] == 2
    _both(hb, unit, 0, 3, "four, unit")


@pytest.mark.parametrize("dt", [F32, I])
def test_single_arc_antiparallel_arcs_and_a_reverse_only_arc(hb, dt):
    g = hb.g
    one = Net(2, [0], [1], [7], dt)
    (fp, fi, fv), r, _ = _both(hb, one, 0, 1, "one arc")
    assert r["value"] == 7 and fp.tolist() == [0, 1, 1] and fi.tolist() == [1] and fv.tolist() == [7]
    anti = Net(2, [0, 1], [1, 0], [3, 9], dt)             # two arcs: 0 -> 1 carries 3, 1 -> 0 nothing
    (fp, fi, fv), r, _ = _both(hb, anti, 0, 1, "antiparallel")
    assert r["value"] == 3 and r["arcs"] == 2 and fi.tolist() == [1] and fv.tolist() == [3]
    (fp, fi, fv), r, _ = _both(hb, anti, 1, 0, "antiparallel, the other way")
    assert r["value"] == 9 and fp.tolist() == [0, 0, 1] and fi.tolist() == [0] and fv.tolist() == [9]
    back = Net(3, [1, 1], [0, 2], [4, 6], dt)             # (1, 0) is stored only as such: 0 -> 1 has no entry in A
    (fp, fi, fv), r, _ = _both(hb, back, 0, 2, "reverse only")
    assert r["value"] == 0 and fi.size == 0 and r["sink_side"] == 2
    (fp, fi, fv), r, _ = _both(hb, back, 1, 0, "reverse only, along it")
    assert r["value"] == 4 and fi.tolist() == [0]
    _both(hb, Net(2, [0, 1], [1, 0], [3, 9], dt, unit=True), 0, 1, "antiparallel, unit")


# ---- random networks -----------------------------------------------------------------------------------------------------
def _random_net(rng, n, m, lo, hi, dt, diag=True):
    i, j = rng.integers(0, n, m), rng.integers(0, n, m)
    key = np.unique(i.astype(np.int64) * n + j)
    i, j = key // n, key % n
    if not diag:
        i, j = i[i != j], j[i != j]
    return Net(n, i, j, rng.integers(lo, hi, i.size), dt)


def test_200_random_networks(hb):
    """2 <= n < 40, up to 4 n entries, capacities 0 .. 8, diagonal entries included, random terminals"""
    rng = np.random.default_rng(51)
    for k in range(200):
        n = int(rng.integers(2, 40))
        net = _random_net(rng, n, int(rng.integers(0, 4 * n + 1)), 0, 9, (I, F32)[k & 1])
        s = int(rng.integers(n))
        t = int(rng.integers(n - 1))
        t += t >= s
        _both(hb, net, s, t, ("random", k))


# ---- the walkers' row-length classes -----------------------------------------------------------------------------------
def _fan(L, where, rng):
    """a row of exactly L residual slots as the source's, the sink's or a hub's in the middle"""
    if where == "source":      # 0 -> L mids -> a collector -> the sink
        mids = np.arange(L) + 1
        col, t, n = L + 1, L + 2, L + 3
        i = np.concatenate([np.zeros(L, np.int64), mids, [col]])
        j = np.concatenate([mids, np.full(L, col), [t]])
        c = np.concatenate([rng.integers(1, 9, L), rng.integers(1, 9, L), [3 * L]])
        return Net(n, i, j, c), 0, t, 0
    if where == "sink":        # the source -> a distributor -> L mids -> the sink
        mids = np.arange(L) + 2
        t, n = L + 2, L + 3
        i = np.concatenate([[0], np.ones(L, np.int64), mids])
        j = np.concatenate([[1], mids, np.full(L, t)])
        c = np.concatenate([[3 * L], rng.integers(1, 9, L), rng.integers(1, 9, L)])
        return Net(n, i, j, c), 0, t, t
    # the source -> the hub (less than the hub could pass on) -> L - 1 leaves -> the sink; the hub's row: L slots
    leaves = np.arange(L - 1) + 2
    t, n = L + 1, L + 2
    i = np.concatenate([[0], np.ones(L - 1, np.int64), leaves])
    j = np.concatenate([[1], leaves, np.full(L - 1, t)])
    out = 1 + np.arange(L - 1) % 8                        # (the hub's budget runs out part of the way through them)
    c = np.concatenate([[int(out.sum()) // 2 + 1], out, np.full(L - 1, 9)])
    return Net(n, i, j, c), 0, t, 1


@pytest.mark.parametrize("where", ["source", "sink", "hub"])
@pytest.mark.parametrize("L", [LANE_LEN, LANE_LEN + 1, WAVE_LEN, WAVE_LEN + 1])
def test_every_row_class(hb, L, where):
    rng = np.random.default_rng(52 + L)
    net, s, t, long_row = _fan(L, where, rng)
    both = np.concatenate([net.i[net.off] * net.n + net.j[net.off], net.j[net.off] * net.n + net.i[net.off]])
    assert np.bincount(np.unique(both) // net.n, minlength=net.n)[long_row] == L     # the residual row's slots
    (fp, fi, fv), r, _ = _both(hb, net, s, t, (where, L))
    if where == "hub":
        # the hub has less excess than its admissible arcs hold: the stored-order rule fills the leaves in order, the rest get nothing
        row = fv[fp[1]:fp[2]].astype(np.int64)
        out = net.caps[(net.i == 1)]
        budget = int(net.caps[0])
        want = np.minimum(out, np.maximum(0, budget - (np.cumsum(out) - out)))
        assert np.array_equal(fi[fp[1]:fp[2]], 2 + np.flatnonzero(want > 0)) and np.array_equal(row, want[want > 0])
        assert 0 < (want > 0).sum() < L - 1


# ---- 64-bit value --------------------------------------------------------------------------------------------------------
def test_value_past_two_to_the_32(hb):
    big = 2 ** 31 - 1
    net = Net(5, [0, 0, 0, 1, 2, 3], [1, 2, 3, 4, 4, 4], [big] * 6, I)
    side = np.array([0, 0, 0, 0, 1], I)                   # every arc is saturated: nothing but the sink reaches the sink
    want = _ref(net, 0, 4, value=(3 * big, side))
    assert want[0] == 3 * big > 2 ** 32
    (fp, fi, fv), r, _ = _both(hb, net, 0, 4, "3 (2^31 - 1)", want)
    assert r["value"] == 6442450941 and fv.tolist() == [big] * 6
    anti = Net(2, [0, 1], [1, 0], [big, big], I)          # the twin's residual reaches 2^32 - 2
    _both(hb, anti, 0, 1, "antiparallel 2^31 - 1", _ref(anti, 0, 1, value=(big, np.array([0, 1], I))))


# ---- excess that must come back ------------------------------------------------------------------------------------------
def _bottleneck_path():
    k = 256
    c = np.full(k - 1, 10)
    c[-1] = 1
    return Net(k, np.arange(k - 1), np.arange(k - 1) + 1, c, I)


def _grid(g, rng, lo=1, hi=8):
    v = np.arange(g * g).reshape(g, g)
    a = np.concatenate([v[:, :-1].ravel(), v[:-1, :].ravel()])
    b = np.concatenate([v[:, 1:].ravel(), v[1:, :].ravel()])
    i, j = np.concatenate([a, b]), np.concatenate([b, a])
    return Net(g * g, i, j, rng.integers(lo, hi, i.size), I)


def test_bottleneck_path(hb):
    net = _bottleneck_path()
    (fp, fi, fv), r1, r2 = _both(hb, net, 0, 255, "bottleneck path")
    assert r1["value"] == 1 and r1["sink_side"] == 1 and r1["cut_arcs"] == 1
    assert fi.tolist() == list(range(1, 256)) and (fv == 1).all()          # the flow on every arc is 1


def test_grid_24(hb):
    net = _grid(24, np.random.default_rng(53))
    _both(hb, net, 0, 24 * 24 - 1, "grid 24 x 24")


# ---- more appends than a wave's stage holds ------------------------------------------------------------------------------
def _stage_net():
    k = 600
    assert k > 2 * STAGE
    mids = np.arange(k) + 1
    return Net(k + 2, np.concatenate([np.zeros(k, np.int64), mids]), np.concatenate([mids, np.full(k, k + 1)]),
               np.concatenate([np.arange(k) % 5 + 1, np.arange(k) % 3 + 1]), I)


def test_more_appends_than_the_lds_stage(hb):
    net = _stage_net()
    _, r, _ = _both(hb, net, 0, 601, "600 middle vertices")
    assert r["value"] == int(np.minimum(np.arange(600) % 5 + 1, np.arange(600) % 3 + 1).sum())


# ---- the unit mode -------------------------------------------------------------------------------------------------------
def test_unit_mode_never_reads_the_values(hb):
    rng = np.random.default_rng(54)
    n = 30
    net = _random_net(rng, n, 100, 0, 9, F32)
    junk = np.array([np.nan, -1.0, 0.5, np.inf, -np.inf, 2.0 ** 30, 0.0, -0.0], F32)
    unit = Net(n, net.i, net.j, junk[rng.integers(0, junk.size, net.i.size)], F32, unit=True)
    assert np.isnan(unit.c).any() and (unit.c < 0).any()
    _both(hb, unit, 3, 17, "unit, junk values")


def test_unit_mode_is_the_maximum_bipartite_matching(hb):
    rng = np.random.default_rng(55)
    k = 40
    B = sp.random(k, k, density=0.06, random_state=np.random.RandomState(5), format="csr")
    B.data[:] = 1
    size = int((maximum_bipartite_matching(B, perm_type="column") >= 0).sum())
    bi, bj = B.nonzero()
    s, t = 2 * k, 2 * k + 1
    i = np.concatenate([np.full(k, s), bi, k + np.arange(k)])
    j = np.concatenate([np.arange(k), k + bj, np.full(k, t)])
    for dt in (I, F32):
        net = Net(2 * k + 2, i, j, rng.integers(1, 9, i.size), dt, unit=True)
        (fp, fi, fv), r, _ = _both(hb, net, s, t, ("bipartite", dt.__name__))
        assert r["value"] == size and 0 < size < k
        rows = np.repeat(np.arange(2 * k + 2), np.diff(fp))
        mid = (rows < k) & (fi >= k) & (fi < 2 * k)
        assert mid.sum() == size and np.unique(rows[mid]).size == size and np.unique(fi[mid]).size == size and (fv == 1).all()


# ---- bad capacities ------------------------------------------------------------------------------------------------------
def test_bad_capacities_are_rejected(hb):
    g = hb.g
    n = 6
    i, j = np.array([0, 1, 2, 3, 4, 2]), np.array([1, 2, 3, 4, 5, 2])       # a path and a diagonal entry
    fbefore, sbefore = Net(n, [0, 3], [5, 1], [2, 3], F32), np.arange(n, dtype=I) + 40
    for dt, bads in ((I, [-1]), (F32, [-1.0, 0.5, np.nan, np.inf, 2.0 ** 24 + 2])):
        Fm = _matrix(g, Net(n, fbefore.i, fbefore.j, fbefore.c, dt))
        side = g.Vector(n, I)
        assert side.build(sbefore, n) == 0
        for bad in bads:
            c = np.array([5, 5, bad, 5, 5, 1], dt)
            A = _matrix(g, Net(n, i, j, c, dt))
            for f_, s_ in ((Fm, side), (None, side), (Fm, None)):
                info, _ = g.maxflow(f_, s_, A, 0, 5, CAPACITY, None)
                assert info == g.GrB_INVALID_VALUE, (dt, bad, info)
                assert Fm.nvals() == 2 and Fm.host_csr()[1].tolist() == [5, 1] and Fm.host_csr()[2].tolist() == [2, 3]
                assert np.array_equal(side.extractTuples()[1], sbefore)
            _both(hb, Net(n, i, j, c, dt, unit=True), 0, 5, ("bad capacity, unit mode", dt.__name__, bad))
            diag = np.array([5, 5, 5, 5, 5, bad], dt)                         # on the diagonal it takes no part
            _both(hb, Net(n, i, j, diag, dt), 0, 5, ("bad capacity on the diagonal", dt.__name__, bad))
    top = Net(n, i, j, np.array([2.0 ** 24] * 5 + [1], F32), F32)            # 2^24 itself converts exactly
    _, r, _ = _both(hb, top, 0, 5, "2^24")
    assert r["value"] == 2 ** 24


# ---- other conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [F32, I])
def test_no_path_components_isolated_terminals_and_zero_capacities(hb, dt):
    rng = np.random.default_rng(56)
    two = Net(8, [0, 1, 2, 4, 5, 6], [1, 2, 3, 5, 6, 7], [3, 4, 5, 6, 7, 8], dt)    # two components
    (fp, fi, fv), r, _ = _both(hb, two, 0, 7, "different components")
    assert r["value"] == 0 and fi.size == 0 and r["sink_side"] == 4 and r["cut_arcs"] == 0
    (fp, fi, fv), r, _ = _both(hb, two, 3, 0, "against the arcs")
    assert r["value"] == 0 and r["sink_side"] == 1
    lone = Net(6, [1, 2, 3], [2, 3, 1], [1, 2, 3], dt)                              # both terminals isolated
    _, r, _ = _both(hb, lone, 0, 5, "isolated terminals")
    assert r["value"] == 0 and r["sink_side"] == 1
    _, r, _ = _both(hb, lone, 0, 2, "isolated source")
    assert r["value"] == 0 and r["sink_side"] == 3
    _both(hb, lone, 2, 5, "isolated sink")
    empty = Net(3, [], [], np.zeros(0), dt)
    _, r, _ = _both(hb, empty, 2, 0, "no entries")
    assert r["value"] == 0 and r["arcs"] == 0
    only_diag = Net(3, [0, 1, 2], [0, 1, 2], [4, 5, 6], dt)
    _, r, _ = _both(hb, only_diag, 0, 1, "only a diagonal")
    assert r["arcs"] == 0
    zeros = _random_net(rng, 25, 90, 0, 3, dt)                                       # a third of the arcs have capacity 0
    assert (zeros.caps[zeros.off] == 0).sum() > 10
    _both(hb, zeros, 1, 20, "stored zeros")
    allzero = Net(4, [0, 1, 2], [1, 2, 3], [0, 0, 0], dt)
    _, r, _ = _both(hb, allzero, 0, 3, "only zero capacities")
    assert r["value"] == 0 and r["arcs"] == 3 and r["sink_side"] == 1


def test_outputs_prefilled_null_in_place_and_csr_only(hb, monkeypatch):
    g = hb.g
    rng = np.random.default_rng(57)
    n = 300
    net = _random_net(rng, n, 1500, 0, 20, F32)
    s, t = 5, 250
    want = _ref(net, s, t)
    assert want[0] > 0
    A = _matrix(g, net)
    Ffull = _matrix(g, _random_net(rng, n, 2000, 1, 5, F32))    # an F that holds something else
    dense = g.Vector(n, I)
    assert dense.build(np.full(n, 9, I), n) == 0
    _check(hb, net, s, t, A=A, Fm=Ffull, side=dense, name="prefilled", want=want)
    sparse = g.Vector(n, I)
    assert sparse.build(np.array([1, 2, 77], I), np.array([4, 4, 4], I), 3, None) == 0
    _check(hb, net, s, t, A=A, side=sparse, name="sparse side", want=want)
    _check(hb, net, s, t, A=A, Fm=None, name="null F", want=want)
    _, arrays, _ = _check(hb, net, s, t, A=A, side=None, name="null side", want=want)
    _check(hb, net, s, t, A=A, Fm=None, side=None, name="both null", want=want)
    monkeypatch.setenv("GRB_SPARSE_MATRIX_FORMAT", "1")
    Fonly = g.Matrix(n, n, F32)
    monkeypatch.delenv("GRB_SPARSE_MATRIX_FORMAT")
    Fonly._csr_only = True
    _, only, _ = _check(hb, net, s, t, A=A, Fm=Fonly, name="F CSR only", want=want)
    assert all(np.array_equal(x, y) for x, y in zip(arrays, only))
    _, inplace, _ = _check(hb, net, s, t, A=A, Fm=A, name="in place", want=want)   # last: A is its own flow now
    assert all(np.array_equal(x, y) for x, y in zip(arrays, inplace))
    fp, fi, fv = arrays
    flow = Net(n, np.repeat(np.arange(n), np.diff(fp)), fi, fv, F32)
    _, again, r = _check(hb, flow, s, t, A=A, name="the flow's flow")
    assert r["value"] == want[0] and r["flow_arcs"] <= fi.size


def test_side_on_caller_owned_storage(hb):
    """side adopted at every 4-byte offset past a 16-byte boundary: the values, the caller's tensor, the guards"""
    import test_gpu_adopted_storage as ad
    g = hb.g
    rng = np.random.default_rng(58)
    n = 1003
    net = _random_net(rng, n, 4000, 1, 9, I)
    want = _ref(net, 2, 900)
    A = _matrix(g, net)
    for k in ad.KS:
        side, tt, check = ad.adopt_dense(g, np.full(n, 77, I), k)
        assert side.device_ptrs()[2] % 16 == 4 * k
        got, _, _ = _check(hb, net, 2, 900, A=A, side=side, Fm=None, name=("adopted", k), want=want)
        assert np.array_equal(ad.payload(tt, k, n, I), got)
        check(("maxflow", k))


# ---- determinism ---------------------------------------------------------------------------------------------------------
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
    side, Fm = g.Vector(n, np.int32), g.Matrix(n, n, val.dtype.type)
    info, res = g.maxflow(Fm, side, A, int(d[name + "_s"]), int(d[name + "_t"]), 0, None)
    assert info == 0 and res["launches"] == 1, (info, res)
    out[name + "_side"] = side.extractTuples()[1]
    out[name + "_fp"], out[name + "_fi"], out[name + "_fv"] = Fm.host_csr()
    out[name + "_rec"] = np.array([res[x] for x in ("value", "arcs", "flow_arcs", "sink_side", "cut_arcs", "cut_capacity", "launches")], np.int64)
np.savez(sys.argv[3], **out)
"""


def test_three_runs_and_a_child_on_four_cus_give_the_same_bits(hb, tmp_path):
    g = hb.g
    rng = np.random.default_rng(59)
    nets = {"a": (_grid(24, rng), 0, 575), "b": (_random_net(rng, 2000, 12000, 1, 30, I), 7, 1500)}
    first = {}
    data = {}
    for name, (net, s, t) in nets.items():
        want = _ref(net, s, t)
        A = _matrix(g, net)
        outs = []
        for _ in range(3):
            side, (fp, fi, fv), res = _check(hb, net, s, t, A=A, name=("determinism", name), want=want)
            outs.append((side.tobytes(), fp.tobytes(), fi.tobytes(), fv.tobytes(), [res[x] for x in EXACT]))
        assert outs[0] == outs[1] == outs[2]
        first[name] = outs[0]
        data[name + "_ptr"], data[name + "_ind"], data[name + "_val"] = net.csr()
        data[name + "_s"], data[name + "_t"] = s, t
    np.savez(tmp_path / "in.npz", **data)
    script = tmp_path / "child.py"
    script.write_text(CHILD)
    env = dict(os.environ, GRB_NUM_CU="4")
    r = subprocess.run([sys.executable, str(script), ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    out = np.load(tmp_path / "out.npz")
    for name in nets:
        got = (out[name + "_side"].tobytes(), out[name + "_fp"].tobytes(), out[name + "_fi"].tobytes(), out[name + "_fv"].tobytes(),
               out[name + "_rec"].tolist())
        assert got == first[name], name


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors_leave_f_and_side_unchanged(hb, monkeypatch):
    g = hb.g
    lib = g._lib.load()
    rng = np.random.default_rng(60)
    n = 80
    net = _random_net(rng, n, 300, 1, 9, F32)
    A = _matrix(g, net)
    ptr, ind, val = net.csr()
    fnet = _random_net(rng, n, 60, 1, 5, F32)
    Fm = _matrix(g, fnet)
    fbefore = Fm.host_csr()
    before = rng.integers(5, 1000, n).astype(I)
    side = g.Vector(n, I)
    assert side.build(before, n) == 0
    sv = g.Vector(n, I)                                   # a sparse side stays sparse
    assert sv.build(np.array([3, 9], I), np.array([5, 6], I), 2, None) == 0

    def unchanged():
        now = Fm.host_csr()
        assert Fm.nvals() == fbefore[1].size and all(np.array_equal(x, y) for x, y in zip(now, fbefore))
        assert side.getStorage() == g.GrB_DENSE and np.array_equal(side.extractTuples()[1], before)
        assert sv.getStorage() == g.GrB_SPARSE and sv.nvals() == 2
        info, si, sx = sv.extractTuples(sparse=True)
        return info == 0 and si.tolist() == [3, 9] and sx.tolist() == [5, 6]

    def call(f_, s_, a, source=0, sink=1, mode=0):
        return lib.grb_maxflow(f_, s_, a, source, sink, mode, None, None)

    assert call(Fm._h, side._h, None) == g.GrB_UNINITIALIZED_OBJECT                  # a null A
    assert call(Fm._h, side._h, g.Matrix(n, n, F32)._h) == g.GrB_UNINITIALIZED_OBJECT  # an unbuilt A
    R = g.Matrix(n, n + 1, F32)                                                      # A not square
    assert R.build_csr(ptr, ind, val) == 0
    assert call(Fm._h, side._h, R._h) == g.GrB_DIMENSION_MISMATCH
    assert call(g.Matrix(n, n + 1, F32)._h, side._h, A._h) == g.GrB_DIMENSION_MISMATCH   # F not n x n
    assert call(g.Matrix(n + 1, n, F32)._h, side._h, A._h) == g.GrB_DIMENSION_MISMATCH
    assert call(Fm._h, g.Vector(n + 1, I)._h, A._h) == g.GrB_DIMENSION_MISMATCH      # size(side) != n
    assert unchanged()
    for s_, t_ in ((-1, 1), (0, -1), (n, 1), (0, n), (2 ** 40, 1), (0, 2 ** 31)):     # a terminal outside 0 .. n - 1
        assert call(Fm._h, side._h, A._h, s_, t_) == g.GrB_INDEX_OUT_OF_BOUNDS
        assert call(None, sv._h, A._h, s_, t_) == g.GrB_INDEX_OUT_OF_BOUNDS
    Z = g.Matrix(0, 0, F32)                                                          # n = 0 cannot name two terminals
    assert Z.build_csr(np.zeros(1, I), np.zeros(0, I), np.zeros(0, F32)) == 0
    assert call(None, None, Z._h, 0, 0) == g.GrB_INDEX_OUT_OF_BOUNDS
    assert call(Fm._h, side._h, A._h, 4, 4) == g.GrB_INVALID_VALUE                   # source == sink
    for mode in (-1, 2, 7):                                                          # a bad mode
        assert call(Fm._h, side._h, A._h, 0, 1, mode) == g.GrB_INVALID_VALUE
        assert call(Fm._h, sv._h, A._h, 0, 1, mode) == g.GrB_INVALID_VALUE
    assert unchanged()
    fv = g.Vector(n, F32)                                                            # a side that is not i32
    fvbefore = rng.random(n).astype(F32) + 2
    assert fv.build(fvbefore, n) == 0
    assert call(Fm._h, fv._h, A._h) == g.GrB_NOT_IMPLEMENTED
    assert np.array_equal(fv.extractTuples()[1].view(np.uint32), fvbefore.view(np.uint32))
    h = ctypes.c_void_p()
    assert lib.grb_matrix_new(ctypes.byref(h), 2, n, n) == 0                         # an A of element type code 2
    assert lib.grb_matrix_build_csr(h, ptr.ctypes.data, ind.ctypes.data, val.ctypes.data, ind.size, None, None, None) == 0
    assert call(None, side._h, h) == g.GrB_NOT_IMPLEMENTED
    assert lib.grb_matrix_free(h) == 0
    Fi = _matrix(g, Net(n, fnet.i, fnet.j, fnet.c, I))                               # F not of A's type
    fibefore = Fi.host_csr()
    assert call(Fi._h, side._h, A._h) == g.GrB_DOMAIN_MISMATCH
    assert all(np.array_equal(x, y) for x, y in zip(Fi.host_csr(), fibefore))
    Aonly = _matrix(g, net, csr_only=True, monkeypatch=monkeypatch)                  # an A without a CSC of its own
    for f_, s_ in ((Fm, side), (None, sv), (None, None)):
        assert call(f_._h if f_ else None, s_._h if s_ else None, Aonly._h) == g.GrB_INVALID_OBJECT
    bad = val.copy()                                                                 # a bad capacity
    bad[np.flatnonzero(net.off)[5]] = -2
    B = g.Matrix(n, n, F32)
    assert B.build_csr(ptr, ind, bad) == 0
    for f_, s_ in ((Fm, side), (Fm, sv), (None, side)):
        assert call(f_._h if f_ else None, s_._h, B._h) == g.GrB_INVALID_VALUE
    assert unchanged()
    # a descriptor and a null descriptor give the same result; the record is optional
    F1, F2 = g.Matrix(n, n, F32), g.Matrix(n, n, F32)
    s1, s2 = g.Vector(n, I), g.Vector(n, I)
    assert lib.grb_maxflow(F1._h, s1._h, A._h, 0, 1, 0, hb.descriptor()._h, None) == 0 and lib.grb_maxflow(F2._h, s2._h, A._h, 0, 1, 0, None, None) == 0
    assert all(np.array_equal(x, y) for x, y in zip(F1.host_csr(), F2.host_csr()))
    assert np.array_equal(s1.extractTuples()[1], s2.extractTuples()[1])


# ---- scale and the C++ frontend ------------------------------------------------------------------------------------------
def test_rmat_12(hb):
    """RMAT-12 ef16 as drawn (directed) with capacities 1 .. 64, from the vertex of largest out-degree to one it reaches"""
    from graphblast_amd.graphgen import rmat_edges
    s, d, n = rmat_edges(12, 16, seed=1)
    key = np.unique(np.asarray(s, np.int64) * n + np.asarray(d, np.int64))
    i, j = key // n, key % n
    rng = np.random.default_rng(61)
    caps = rng.integers(1, 65, i.size)
    src = int(np.argmax(np.bincount(i[i != j], minlength=n)))
    order = breadth_first_order(sp.csr_matrix((np.ones(i.size), (i, j)), shape=(n, n)), src, directed=True, return_predecessors=False)
    snk = int(order[-1])
    assert snk != src
    for dt in (I, F32):
        net = Net(n, i, j, caps, dt)
        _, r, _ = _both(hb, net, src, snk, ("RMAT-12", dt.__name__))
        assert r["value"] > 0 and r["arcs"] == int((i != j).sum())
    hub2 = int(np.argsort(np.bincount(j[i != j], minlength=n))[-1])                   # into the vertex of largest in-degree
    if hub2 != src:
        _both(hb, Net(n, i, j, caps, I), src, hub2, "RMAT-12, hub to hub")


def test_cpp_frontend(tmp_path):
    """tests/tools/maxflow.cpp on chesapeake.mtx with the capacities 1 + (i + 3 j) % 7 in both directions, from vertex 0 to
    vertex n - 1: the record, side from the float and the int run, F a maximum flow, the unit value"""
    exe = str(tmp_path / "maxflow")
    subprocess.check_call(["g++", "-std=c++11", "-O1", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "tools", "maxflow.cpp"),
                           "-L" + os.path.join(ROOT, "graphblast_amd"), "-lgrb_hip",
                           "-Wl,-rpath," + os.path.join(ROOT, "graphblast_amd"), "-o", exe])
    path = os.path.join(ROOT, "tests", "golden", "data", "chesapeake.mtx")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    lines = [ln.strip() for ln in r.stdout.split("\n") if ln.strip()]
    assert r.returncode == 0, (r.returncode, lines, r.stderr[-2000:])
    co = sp.coo_matrix(scipy.io.mmread(path))
    keep = co.row != co.col
    n = co.shape[0]
    a, b = co.row[keep].astype(np.int64), co.col[keep].astype(np.int64)
    key = np.unique(np.concatenate([a * n + b, b * n + a]))
    i, j = key // n, key % n
    net = Net(n, i, j, 1 + (i + 3 * j) % 7, F32)
    value, side, rec = _ref(net, 0, n - 1)
    assert rec["arcs"] == 340 and value > 0
    assert lines[-1] == "ok"
    head = [ln for ln in lines if ln.startswith("capacity value")]
    assert len(head) == 1
    words = head[0].split()
    got = dict(zip(words[1::2], map(int, words[2::2])))
    for x in rec:
        assert got[x] == rec[x], (x, got, rec)
    assert got["cut_capacity"] == value
    assert "side " + " ".join(map(str, side.tolist())) in lines
    assert "int side " + " ".join(map(str, side.tolist())) in lines
    csr = [ln for ln in lines if ln.startswith("csr |")][0].split("|")
    fp, fi, fv = (np.array(x.split(), dtype=float).astype(np.int64) for x in csr[1:])

    class Shown:
        _csr_only = True                                  # (only the CSR is printed)

        def host_csr(self):
            return fp.astype(I), fi.astype(I), fv.astype(F32)

        def nvals(self):
            return fi.size

    _valid_flow(net, 0, n - 1, value, side, Shown(), dict(flow_arcs=got["flow_arcs"]), "C++ frontend")
    unit = _ref(Net(n, i, j, np.ones(i.size), I, unit=True), 0, n - 1)[0]
    assert any(ln.startswith("unit value %d flow_arcs " % unit) for ln in lines)
