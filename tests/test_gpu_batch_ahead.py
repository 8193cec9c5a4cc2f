"""GPU suite (-m gpu): the bit-parallel sweep decides a level's directions on the device and launches the next level's pull
kernels ahead of the host (bfs_batch.hip, batch_decide.hpp; GRB_BATCH_AHEAD=0 waits first).  Small graphs never leave the
light-level launch at its default limit, so every case sets the limit to 0 (every level through the host loop) and to 64
(the launch entered again and again) and restores it.  Both entrances: grb_bfs_batch and the queue's routed sweep
(grb_bfs_set_sweep_from(2)), each case in a fresh child process, once more with GRB_BATCH_AHEAD=0.  Labels against the
oracle, totals against the labels, the routed sweep's result blocks against the blocking call.

Graphs: RMAT-13 symmetrised plus one vertex adjacent to all others (an 8192-entry row: the slice, list and owner kernels;
n + 1 vertices, no multiple of 64); the same plus a 3-vertex component holding a source (a big in-row that never gets
that source's bit: the slice kernels stay) and an isolated vertex; a thinned 48 x 48 grid (more than 16 levels: past the
kept slots, a planned rotating array) and a path of 40 vertices, each with an isolated vertex appended."""
import os
import re
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
KEYS = ("levels", "reached", "edges_traversed")
KS = (1, 2, 20, 33, 64)
LIMITS = (0, 64)


def csr_of(name):
    if name == "grid":
        s, d, n = grid_edges(48, keep=0.6, seed=3)
        s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
        extra = []
    elif name == "path":
        s, d, n = np.arange(39, dtype=np.int64), np.arange(1, 40, dtype=np.int64), 40
        extra = []
    else:
        s, d, n = rmat_edges(13, 16, seed=3)
        s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
        s = np.concatenate([s, np.full(n, n, dtype=np.int64)])      # vertex n, adjacent to every other
        d = np.concatenate([d, np.arange(n, dtype=np.int64)])
        n += 1
        extra = []
        if name == "hubsplit":                                      # a component of three, apart from everything
            s = np.concatenate([s, [n, n + 1]])
            d = np.concatenate([d, [n + 1, n + 2]])
            extra = [n + 1]
            n += 3
    if name != "hub":
        n += 1                                                      # an isolated vertex
        extra.append(n - 1)
    ptr, ind = [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=True)["csr"]]
    return ptr, ind, extra


ptr, ind, extra = csr_of(graph)
n = ptr.size - 1
deg = np.diff(ptr)
hub = int(np.argmax(deg))
if graph in ("hub", "hubsplit"):
    assert deg[hub] >= 8192 and n % 64 != 0
A = g.Matrix(n, n)
assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
oracle = {}


def want(s_):
    if s_ not in oracle:
        oracle[s_] = sr.bfs(ptr, ind, s_)[0]
    return oracle[s_]


def sources(count, seed=11):
    """the maximum-degree vertex, the component of three and the isolated vertex where there are any, a repeated source"""
    out = [hub] + extra + random_sources(ptr, max(count - len(extra) - 2, 0), seed=seed)
    out.append(out[-1])
    return out[:count]


def descriptor(**args):
    d = g.Descriptor()
    assert d.loadArgs(struconly=1, opreuse=1, **args) == 0
    return d


def batch(srcs, cap=None, **args):
    if cap is not None:
        args["max_niter"] = cap
    d = descriptor(**args)
    vs = [g.Vector(n) for _ in srcs]
    for rep in range(2):                                            # twice on the same buffers: what the first leaves, the second finds
        info, res = g.bfs_batch(vs, A, srcs, d)
        assert info == 0, info
        for v, s_ in zip(vs, srcs):
            w = want(s_)
            assert np.array_equal(v.extractTuples()[1], w if cap is None else np.where(w <= cap, w, 0)), (args, rep, s_)
        if cap is None or cap > max(int(want(s_).max()) for s_ in srcs):
            assert res["reached"] == sum(int(np.count_nonzero(want(s_))) for s_ in srcs), (args, rep)
            assert res["edges_traversed"] == sum(int(deg[want(s_) != 0].sum()) for s_ in srcs), (args, rep)
    return res


def routed(srcs):
    d = descriptor(mxvmode=0)
    vs = [g.Vector(n) for _ in srcs]
    for rep in range(2):
        c0 = g.bfs_sweep_counts()
        tickets = []
        for v, s_ in zip(vs, srcs):
            info, t = g.bfs_enqueue(v, A, s_, d)
            assert info == 0 and t != 0, info
            tickets.append(t)
        res = []
        for t in tickets:
            info, r = g.bfs_wait(t)
            assert info == 0, info
            res.append(r)
        c1 = g.bfs_sweep_counts()
        # (the queue launches what has gathered at 48: 64 queued are a sweep of 48 and one of 16)
        assert (c1["sweeps"] - c0["sweeps"], c1["traversals"] - c0["traversals"]) == ((len(srcs) + 47) // 48, len(srcs)), (c0, c1)
        for v, r, s_ in zip(vs, res, srcs):
            assert np.array_equal(v.extractTuples()[1], want(s_)), ("routed", rep, s_)
            vb = g.Vector(n)
            info, rb = g.bfs(vb, A, s_, d, fused=True)
            assert info == 0
            assert all(r[k] == rb[k] for k in KEYS), (s_, {k: (r[k], rb[k]) for k in KEYS})


before = g.bfs_batch_set_tail(-1)
try:
    for limit in LIMITS:
        g.bfs_batch_set_tail(limit)
        if mode == "sizes":                                         # push-pull, every k, both entrances
            for k in KS:
                batch(sources(k), mxvmode=0)
            kstar = g.bfs_set_sweep_from(2)
            for k in KS[1:]:
                routed(sources(k, seed=5))
            g.bfs_set_sweep_from(kstar)
        elif mode == "rules":
            srcs = sources(20)
            batch(srcs, mxvmode=2)                                  # pull-only: every level a host level, the sweep ends on one
            batch(srcs, mxvmode=1)                                  # push-only: nothing is launched ahead
            # no source ever passes the switch point: pulled by the budget alone at the widest level, all pushed on the
            # next -- a host level whose words the pull kernel zeroes
            batch(srcs, mxvmode=0, switchpoint=0.9)
            batch(sources(64), mxvmode=0, switchpoint=0.9)
            os.environ["GRB_SPARSE_MATRIX_FORMAT"] = "1"            # no CSC side: every source pushed, nothing ahead
            A_csr, A = A, g.Matrix(n, n)
            assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
            del os.environ["GRB_SPARSE_MATRIX_FORMAT"]
            batch(srcs, mxvmode=0)
            A = A_csr
        elif mode == "caps":                                        # max_niter = 1 .. levels + 1
            srcs = sources(20)
            depth = max(int(want(s_).max()) for s_ in srcs)
            for cap in range(1, depth + 2):
                batch(srcs, cap=cap, mxvmode=0)
                if graph != "path":
                    batch(srcs, cap=cap, mxvmode=2)
        elif mode == "paths":
            # GRB_BATCH_TRACE is on: the library logs every level to stderr; a marker in front of each sweep lets the
            # parent check that the path a case is meant to take was taken
            def marked(tag, srcs, **args):
                print("@@ %s limit=%d" % (tag, limit), file=sys.stderr, flush=True)
                batch(srcs, **args)
            if graph == "path":
                marked("zeroing", sources(20), mxvmode=0, switchpoint=0.9)
            elif graph == "grid":
                marked("launches", sources(2), mxvmode=0)
            else:
                marked("bigrows", sources(20), mxvmode=0)
finally:
    g.bfs_batch_set_tail(before)
print("OK")
'''


def run_child(graph, mode, ahead, trace=False):
    env = dict(os.environ)
    env.pop("GRB_BATCH_AHEAD", None)
    env.pop("GRB_BATCH_TRACE", None)
    if not ahead:
        env["GRB_BATCH_AHEAD"] = "0"
    if trace:
        env["GRB_BATCH_TRACE"] = "1"
    out = subprocess.run([sys.executable, "-c", CHILD, graph, mode], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2500:]
    return out.stderr


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["hub", "hubsplit", "grid", "path"])
def test_every_k_through_both_entrances(graph, ahead):
    """k = 1, 2, 20, 33, 64 (the hub, a repeated source, an isolated one, the component of three) through grb_bfs_batch and,
    from k = 2, as a routed sweep (64 queued: one of 48 and one of 16); each twice on the same buffers; light-level limit 0 and 64 (on the grid: far more than
    four light-level launches in one sweep)."""
    run_child(graph, "sizes", ahead)


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["hub", "hubsplit", "grid"])
def test_rules(graph, ahead):
    """pull-only, push-only, a switch point nobody passes (a pulled level, then an all-pushed host level), a matrix without
    its CSC side."""
    run_child(graph, "rules", ahead)


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["hub", "grid", "path"])
def test_iteration_caps(graph, ahead):
    """max_niter = 1 .. levels + 1: the cap falls on every level once, ahead launches included."""
    run_child(graph, "caps", ahead)


def traced_sweeps(graph, ahead):
    """{(tag, limit): [the trace lines of each sweep]} of the child's "paths" mode"""
    sweeps, cur = {}, None
    for line in run_child(graph, "paths", ahead, trace=True).splitlines():
        if line.startswith("@@ "):
            _, tag, lim = line.split()
            cur = sweeps.setdefault((tag, int(lim.split("=")[1])), [])
        elif cur is not None and line.startswith("batch level") and "owner-computes" not in line:
            if re.match(r"batch levels? 1[ .:]", line):             # a sweep's first level, alone or as the first of a launch
                cur.append([])
            cur[-1].append(line)
    return sweeps


HOST_LEVEL = re.compile(r"batch level (\d+): pull (\d+) sources, push (\d+) .*big in-rows open (\(not counted\) )?(\d+), "
                        r"big out-rows found (-?\d+), next level (pulled ahead|host|light|none)")


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_a_pulled_level_is_followed_by_an_all_pushed_host_level(ahead):
    """The path, light-level launch off, a switch point nobody passes: twenty sources are over the budget together, so the
    heaviest are pulled, until enough of them have run out -- then a host level pushes every live source, into words that
    (launched ahead) the pull kernel has zeroed."""
    for sweep in traced_sweeps("path", ahead)[("zeroing", 0)]:
        levels = [HOST_LEVEL.match(x) for x in sweep]
        levels = [(int(m.group(2)), int(m.group(3)), m.group(7)) for m in levels if m]
        follows = [i for i in range(1, len(levels)) if levels[i - 1][0] > 0 and levels[i][0] == 0 and levels[i][1] > 0]
        assert follows, levels
        if ahead:
            assert all(levels[i - 1][2] == "pulled ahead" for i in follows), levels


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_more_than_four_light_level_launches_in_one_sweep(ahead):
    """Two sources on the grid with limit 64: the frontier's out-edges cross the limit again and again, five launches at
    the least -- the fifth clears its state block itself."""
    for sweep in traced_sweeps("grid", ahead)[("launches", 64)]:
        assert sum("one launch (light levels)" in x for x in sweep) > 4, sweep


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_big_row_counts_stop_the_helper_kernels_only_when_they_may(ahead):
    """Light-level launch off.  hub: every source reaches the 8192-entry row in its first level, so the first apply kernel
    counts 0 open big in-rows, and the hub among the discoveries is a big out-row found.  hubsplit: the source in the
    component of three never reaches it -- every count stays above 0 and the slice kernels stay."""
    for graph in ("hub", "hubsplit"):
        for sweep in traced_sweeps(graph, ahead)[("bigrows", 0)]:
            levels = [HOST_LEVEL.match(x) for x in sweep]
            counted = [int(m.group(5)) for m in levels if m and not m.group(4)]
            found = [int(m.group(6)) for m in levels if m]
            assert counted and max(found) > 0, sweep
            assert (min(counted) == 0) if graph == "hub" else (min(counted) > 0), (graph, counted)
