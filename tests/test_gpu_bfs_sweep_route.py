"""GPU suite (-m gpu): under the default width rule a gathered group of k* or more plain queued traversals runs as ONE
bit-parallel sweep (bfs_batch.hip) instead of the co-scheduled launch (grb_bfs_set_sweep_from; docs/experiments.md R8.1).
Other test files leave a width set, so every case runs in a fresh child process.  Labels are compared with the oracle and
with the blocking call, result blocks (levels, reached, edges_traversed) with the blocking call, and
grb_bfs_coschedule_profile / grb_bfs_sweep_counts must show the expected launches, traversals and sweeps.

Graphs: RMAT-13 (ef 16, symmetrised); the same plus one vertex adjacent to every other (a row of 8192 entries: the slice
and owner kernels of both directions); a thinned 48 x 48 grid (more than 16 levels: past the stored level words into the
direct-label path); a directed RMAT-13 (the CSC differs from the CSR); the hub graph once more at RMAT-15 (owner ranges need 16 Ki vertices)."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import graphblast_amd as g
from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges, random_sources
from oracle import simple_reference as sr

graph, mode = sys.argv[1], sys.argv[2]
assert g.bfs_set_coschedule(-1) == 1                    # (what a query answers while the library picks the width)
KSTAR = g.bfs_set_sweep_from(-1)
assert 2 <= KSTAR <= 48, KSTAR
KEYS = ("levels", "reached", "edges_traversed")


def csr_of(name):
    if name == "grid":
        s, d, n = grid_edges(48, keep=0.6, seed=3)
        return [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=True)["csr"]]
    s, d, n = rmat_edges(15 if name == "hub15" else 13, 16, seed=3)
    s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
    if name in ("hub", "hub15"):                                   # vertex n, adjacent to every other
        s = np.concatenate([s, np.full(n, n, dtype=np.int64)])
        d = np.concatenate([d, np.arange(n, dtype=np.int64)])
        n += 1
    return [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=(name != "directed"))["csr"]]


def matrix(ptr, ind):
    A = g.Matrix(ptr.size - 1, ptr.size - 1)
    assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
    return A


ptr, ind = csr_of(graph)
n = ptr.size - 1
deg = np.diff(ptr)
A = matrix(ptr, ind)
desc = g.Descriptor()
assert desc.loadArgs(mxvmode=0, struconly=1, opreuse=1, edgeswitch=0.05) == 0
desc_plain = g.Descriptor()
assert desc_plain.loadArgs(mxvmode=0, struconly=1, opreuse=1) == 0
hub = int(np.argmax(deg))
lonely = int(np.nonzero(deg == 0)[0][0]) if (deg == 0).any() else None
if graph in ("hub", "hub15"):
    assert deg[hub] >= 4096
if graph == "grid":
    assert sr.bfs(ptr, ind, hub)[0].max() > 17          # more levels than the sweep stores words for
blocking = {}


def blocking_call(src, M=None, d=None, key=None):
    k_ = (src, key)
    if k_ not in blocking:
        vb = g.Vector(n)
        info, res = g.bfs(vb, M if M is not None else A, src, d if d is not None else desc, fused=True)
        assert info == 0, info
        blocking[k_] = (vb.extractTuples()[1], res)
    return blocking[k_]


def queue(vecs, srcs, mats=None, d=None):
    tickets = []
    for i, (v, s_) in enumerate(zip(vecs, srcs)):
        info, t = g.bfs_enqueue(v, mats[i] if mats else A, s_, d if d is not None else desc)
        assert info == 0 and t != 0, info
        tickets.append(t)
    out = []
    for t in tickets:
        info, res = g.bfs_wait(t)
        assert info == 0, info
        out.append(res)
    return out


def profiled(vecs, srcs, mats=None, d=None):
    c0 = g.bfs_sweep_counts()
    g.bfs_coschedule_profile(True)
    res = queue(vecs, srcs, mats, d)
    prof = g.bfs_coschedule_profile(False)
    c1 = g.bfs_sweep_counts()
    return res, (prof["launches"], prof["traversals"]), (c1["sweeps"] - c0["sweeps"], c1["traversals"] - c0["traversals"])


def check(vecs, res, srcs, oracle=True, M=None, d=None, key=None, csr=None):
    p_, i_ = csr if csr else (ptr, ind)
    for v, r, s_ in zip(vecs, res, srcs):
        got = v.extractTuples()[1]
        want, rb = blocking_call(s_, M, d, key)
        assert np.array_equal(got, want), ("labels differ from the blocking call", s_)
        if oracle:
            assert np.array_equal(got, sr.bfs(p_, i_, s_)[0]), ("labels differ from the oracle", s_)
        assert all(r[k] == rb[k] for k in KEYS), (s_, {k: (r[k], rb[k]) for k in KEYS})


def sources(count, seed=11):
    """the maximum-degree vertex, a vertex with no edges (where the graph has one), a repeated source, random ones"""
    out = [hub] + ([lonely] if lonely is not None else [])
    out += random_sources(ptr, max(count - len(out) - 1, 0), seed=seed)
    out.append(out[-1])                                     # the repeated source
    return out[:count]


if mode == "counts":
    for count in (KSTAR - 1, KSTAR, 48, 49):
        srcs = sources(count)
        vs = [g.Vector(n) for _ in srcs]
        res, launched, swept = profiled(vs, srcs)
        if count < KSTAR:
            assert swept == (0, 0), (count, swept)
            assert launched == ((1, count) if count >= 2 else (0, 0)), (count, launched)
        else:
            # 48 fill a group (swept when the 48th is queued); the 49th goes alone, to the one-traversal kernel
            assert swept == (1, min(count, 48)) and launched == (1, min(count, 48)), (count, launched, swept)
        check(vs, res, srcs)
        if lonely is not None and count >= 2:
            r = res[1]
            assert (r["reached"], r["levels"], r["edges_traversed"]) == (1, 1, 0), r
elif mode == "rules":
    srcs = sources(KSTAR + 2, seed=5)
    vs = [g.Vector(n) for _ in srcs]
    for d_, key in ((desc, None), (desc_plain, "plain")):   # edgeswitch set / not set: both swept, same results
        res, launched, swept = profiled(vs, srcs, d=d_)
        assert swept == (1, len(srcs)) and launched == (1, len(srcs)), (key, launched, swept)
        check(vs, res, srcs, d=d_, key=key)
    d_cut = g.Descriptor()                                  # an iteration cap: the co-scheduled launch, unchanged results
    assert d_cut.loadArgs(mxvmode=0, struconly=1, opreuse=1, max_niter=3) == 0
    res, launched, swept = profiled(vs, srcs, d=d_cut)
    assert swept == (0, 0) and launched == (1, len(srcs)), (launched, swept)
    check(vs, res, srcs, oracle=False, d=d_cut, key="cut")
    d_push = g.Descriptor()                                 # push-only: the same
    assert d_push.loadArgs(mxvmode=1, struconly=1, opreuse=1) == 0
    res, launched, swept = profiled(vs, srcs, d=d_push)
    assert swept == (0, 0) and launched == (1, len(srcs)), (launched, swept)
    check(vs, res, srcs, d=d_push, key="push")
    os.environ["GRB_SPARSE_MATRIX_FORMAT"] = "1"            # a CSR-only matrix: never gathered, never swept
    A1 = matrix(ptr, ind)
    del os.environ["GRB_SPARSE_MATRIX_FORMAT"]
    res, launched, swept = profiled(vs, srcs, mats=[A1] * len(srcs))
    assert swept == (0, 0) and launched == (0, 0), (launched, swept)
    check(vs, res, srcs, M=A1, key="csronly")
elif mode == "orderings":
    # v <- s0, v <- s1, w <- s2, v <- s3 behind KSTAR gathered: the last traversal into a vector wins
    srcs = sources(KSTAR, seed=7)
    vs = [g.Vector(n) for _ in srcs]
    s0, s1, s2, s3 = random_sources(ptr, 4, seed=5)
    v, w = g.Vector(n), g.Vector(n)
    res = queue(vs + [v, v, w, v], srcs + [s0, s1, s2, s3])
    check(vs, res[:KSTAR], srcs)
    assert np.array_equal(v.extractTuples()[1], blocking_call(s3)[0])
    assert np.array_equal(w.extractTuples()[1], blocking_call(s2)[0])
    for r, s_ in zip(res[KSTAR:], (s0, s1, s2, s3)):
        assert all(r[k] == blocking_call(s_)[1][k] for k in KEYS), s_
    # two matrices queued alternately: every change of matrix launches what has gathered (groups of one)
    B = matrix(ptr, ind)
    vs2 = [g.Vector(n) for _ in range(6)]
    srcs2 = sources(6, seed=9)
    res = queue(vs2, srcs2, mats=[A, B] * 3)
    check(vs2, res, srcs2)
    # ... and KSTAR on A, KSTAR on B, KSTAR on A: three swept groups
    vs3 = [g.Vector(n) for _ in range(3 * KSTAR)]
    srcs3 = sources(3 * KSTAR, seed=13)
    res, launched, swept = profiled(vs3, srcs3, mats=[A] * KSTAR + [B] * KSTAR + [A] * KSTAR)
    assert swept == (3, 3 * KSTAR) and launched == (3, 3 * KSTAR), (launched, swept)
    check(vs3, res, srcs3)
elif mode == "blocking_between":
    srcs = sources(2 * KSTAR, seed=17)
    vs = [g.Vector(n) for _ in srcs]
    res1, launched1, swept1 = profiled(vs[:KSTAR], srcs[:KSTAR])
    vb = g.Vector(n)
    info, rb = g.bfs(vb, A, hub, desc, fused=True)          # a blocking call between two swept groups
    assert info == 0
    assert np.array_equal(vb.extractTuples()[1], sr.bfs(ptr, ind, hub)[0])
    res2, launched2, swept2 = profiled(vs[KSTAR:], srcs[KSTAR:])
    assert swept1 == swept2 == (1, KSTAR) and launched1 == launched2 == (1, KSTAR)
    check(vs, res1 + res2, srcs)
elif mode == "explicit_width":
    srcs = sources(KSTAR + 5, seed=19)
    for width in (12, 1):                                   # an explicit width asks for per-traversal kernels: no sweep
        g.bfs_set_coschedule(width)
        vs = [g.Vector(n) for _ in srcs]
        res, launched, swept = profiled(vs, srcs)
        assert swept == (0, 0), (width, swept)
        assert launched == ((1, len(srcs)) if width == 12 else (0, 0)), (width, launched)
        check(vs, res, srcs)
elif mode == "opt_out":
    assert g.bfs_set_sweep_from(0) == KSTAR                 # the route off under the default width rule
    srcs = sources(KSTAR + 1, seed=23)
    vs = [g.Vector(n) for _ in srcs]
    res, launched, swept = profiled(vs, srcs)
    assert swept == (0, 0) and launched == (1, len(srcs)), (launched, swept)
    check(vs, res, srcs)
    assert g.bfs_set_sweep_from(KSTAR) == 0
    res, launched, swept = profiled(vs, srcs)
    assert swept == (1, len(srcs)), swept
    check(vs, res, srcs)
print("OK")
'''


def run_child(graph, mode):
    out = subprocess.run([sys.executable, "-c", CHILD, graph, mode], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2500:]
    assert "not published" not in out.stderr and "host-driven" not in out.stderr, out.stderr[-1500:]


@pytest.mark.parametrize("graph", ["rmat", "hub", "grid", "directed", "hub15"])
def test_counts_around_the_sweep_threshold(graph):
    """k* - 1 (not swept), k*, 48 and 49 (48 swept, one alone) traversals queued under the default; the sources include
    the maximum-degree vertex, a vertex with no edges (reached 1, levels 1, edges 0) and a repeated source.  (hub15: the
    hub graph at RMAT-15, the smallest size at which the matrix gets owner ranges for the heavy push levels.)"""
    run_child(graph, "counts")


@pytest.mark.parametrize("graph", ["rmat", "directed"])
def test_rules_that_are_swept_and_rules_that_are_not(graph):
    """A descriptor with edgeswitch and one without are both swept; a max_niter cut, a push-only mode and a CSR-only
    matrix stay on the per-traversal kernels with unchanged results."""
    run_child(graph, "rules")


@pytest.mark.parametrize("graph", ["rmat", "hub"])
def test_orderings(graph):
    """v <- s0, v <- s1, w <- s2, v <- s3 with k* reached: the last traversal into a vector wins; two matrices queued
    alternately; three swept groups on two matrices."""
    run_child(graph, "orderings")


@pytest.mark.parametrize("graph", ["rmat", "grid"])
def test_a_blocking_call_between_two_swept_groups(graph):
    run_child(graph, "blocking_between")


def test_an_explicit_width_keeps_the_per_traversal_kernels():
    """grb_bfs_set_coschedule(12) and (1): no sweep, launches and traversals as before the route existed."""
    run_child("rmat", "explicit_width")


def test_sweep_from_zero_turns_the_route_off():
    run_child("rmat", "opt_out")
