"""GPU suite (-m gpu): the bit-parallel sweep's first level as a plain launch (bfs_batch.hip: batch_first_level_kernel).
When the rule pushes every source at level 1 the seeds get their labels from the seed kernel, the level's words go to
the first kept slot, a wave takes a 256-edge piece of a source's row, and the level after it is decided on the device; a
light-level launch that follows starts at level 2 from the kept words.  Any source pulled at level 1: the path with seed
words, as before.

Everything is compared exactly: labels against the oracle and the blocking traversal, the totals of grb_bfs_batch against
the blocking traversals' (sums; levels: the longest), the routed sweep's result blocks against them one by one.  Every
sweep runs twice on the same buffers, the second time with the sources in another order (what the first leaves -- the
clean-array bookkeeping -- the second finds); light-level limit 0 and the default; each case in a fresh child process,
with GRB_BATCH_AHEAD 1 and 0.

Graphs (n is no multiple of 64):
  pieces  4999 vertices: a hub adjacent to all but an isolated one (4997 edges: 20 pieces), stars of out-degree 1, 255,
          256, 257 and 1025 (a piece's boundaries, from both sides), a stored self-loop, 40 K random edges among the rest
          (so that the sources' rows stay under the push budget)
  path    301 vertices in a row and an isolated one (a source alone is under the switch point only from n > 100, and
          twenty sources' level-2 frontiers -- at most 80 out-edges -- stay under the push budget of 0.15 * 600 entries, so
          that the device decides "light" for level 2)
  grid    the thinned 48 x 48 grid of test_gpu_batch_ahead.py and an isolated vertex
  star    a hub and 4098 leaves: the hub's row alone is over the push budget, so level 1 pulls it"""
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
from graphblast_amd.graphgen import grid_edges
from oracle import simple_reference as sr

graph, mode = sys.argv[1], sys.argv[2]
KEYS = ("levels", "reached", "edges_traversed")
HUB, C1, C255, C256, C257, C1025, LOOP = 5, 0, 1, 2, 3, 4, 6


def csr(n, s, d):
    """symmetrised, duplicates merged, a self-loop stored once"""
    s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
    key = np.unique(np.concatenate([s * n + d, d * n + s]))
    ptr = np.zeros(n + 1, dtype=np.int32)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    return ptr, (key % n).astype(np.int32)


def make(name):
    if name == "pieces":
        n = 4999
        s, d = [], []
        s += [HUB] * (n - 2)
        d += [v for v in range(n - 1) if v != HUB]                  # vertex n - 1 stays isolated
        leaf = 7
        for c, deg in ((C255, 255), (C256, 256), (C257, 257), (C1025, 1025)):
            s += [c] * (deg - 1)                                    # the hub is a neighbour already
            d += list(range(leaf, leaf + deg - 1))
            leaf += deg - 1
        s.append(LOOP); d.append(LOOP)
        rng = np.random.default_rng(7)
        s += list(rng.integers(leaf, n - 1, 40000)); d += list(rng.integers(leaf, n - 1, 40000))
        ptr, ind = csr(n, s, d)
        deg = np.diff(ptr)
        assert [int(deg[v]) for v in (n - 1, C1, C255, C256, C257, C1025, HUB)] == [0, 1, 255, 256, 257, 1025, n - 2], deg[:8]
        assert LOOP in ind[ptr[LOOP]:ptr[LOOP + 1]]
        special = [HUB, C1025, C257, C256, C255, C1, n - 1, LOOP, C256, C256]   # hub and C1025 adjacent; C256 three times
    elif name == "path":
        n = 302
        ptr, ind = csr(n, np.arange(300), np.arange(1, 301))
        special = [0, 100, n - 1, 100, 300, 57]
    elif name == "grid":
        s, d, n = grid_edges(48, keep=0.6, seed=3)
        n += 1
        ptr, ind = csr(n, s, d)
        top = int(np.argmax(np.diff(ptr)))
        special = [top, int(ind[ptr[top]]), n - 1, top]             # a vertex of the largest degree, a neighbour of it
    else:
        n = 4099
        ptr, ind = csr(n, np.zeros(n - 1, dtype=np.int64), np.arange(1, n))
        special = [0, 17, 17, 4000]
    assert n % 64 != 0
    return n, ptr, ind, special


n, ptr, ind, special = make(graph)
deg = np.diff(ptr)
A = g.Matrix(n, n)
assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
oracle, blocking = {}, {}


def descriptor(**args):
    d = g.Descriptor()
    assert d.loadArgs(struconly=1, opreuse=1, **args) == 0
    return d


def want(s_):
    if s_ not in oracle:
        oracle[s_] = sr.bfs(ptr, ind, s_)[0]
        vb = g.Vector(n)
        info, rb = g.bfs(vb, A, s_, descriptor(mxvmode=0), fused=True)
        assert info == 0
        assert np.array_equal(vb.extractTuples()[1], oracle[s_]), ("blocking", s_)
        blocking[s_] = rb
    return oracle[s_]


def sources(k):
    rest = [int(x) for x in np.random.default_rng(11).permutation(n) if deg[x] > 0]
    return (special + rest)[:k]


def batch(srcs, cap=None, tag=None, **args):
    if cap is not None:
        args["max_niter"] = cap
    d = descriptor(**args)
    vs = [g.Vector(n) for _ in srcs]
    for rep in range(2):
        order = srcs if rep == 0 else srcs[::-1]
        if tag:
            print("@@ %s" % tag, file=sys.stderr, flush=True)
        info, res = g.bfs_batch(vs, A, order, d)
        assert info == 0, info
        for v, s_ in zip(vs, order):
            w = want(s_)
            assert np.array_equal(v.extractTuples()[1], w if cap is None else np.where(w <= cap, w, 0)), (args, rep, s_)
        if cap is None:
            assert res["reached"] == sum(blocking[s_]["reached"] for s_ in order), (args, rep)
            assert res["edges_traversed"] == sum(blocking[s_]["edges_traversed"] for s_ in order), (args, rep)
            assert res["levels"] == max(blocking[s_]["levels"] for s_ in order), (args, rep)
            assert res["reached"] == sum(int(np.count_nonzero(want(s_))) for s_ in order), (args, rep)


def routed(srcs):
    d = descriptor(mxvmode=0)
    vs = [g.Vector(n) for _ in srcs]
    for rep in range(2):
        order = srcs if rep == 0 else srcs[::-1]
        c0 = g.bfs_sweep_counts()
        tickets = []
        for v, s_ in zip(vs, order):
            info, t = g.bfs_enqueue(v, A, s_, d)
            assert info == 0 and t != 0, info
            tickets.append(t)
        res = []
        for t in tickets:
            info, r = g.bfs_wait(t)
            assert info == 0, info
            res.append(r)
        c1 = g.bfs_sweep_counts()
        assert (c1["sweeps"] - c0["sweeps"], c1["traversals"] - c0["traversals"]) == ((len(srcs) + 47) // 48, len(srcs)), (c0, c1)
        for v, r, s_ in zip(vs, res, order):
            assert np.array_equal(v.extractTuples()[1], want(s_)), ("routed", rep, s_)
            assert all(r[k] == blocking[s_][k] for k in KEYS), (s_, {k: (r[k], blocking[s_][k]) for k in KEYS})


default = g.bfs_batch_set_tail(-1)
assert default > 0
try:
    for limit in (0, default):
        g.bfs_batch_set_tail(limit)
        if mode == "sizes":
            for k in (1, 2, 31, 32, 33, 64):
                batch(sources(k), mxvmode=0)
            for s_ in dict.fromkeys(special):                       # one at a time
                batch([s_], mxvmode=0)
            kstar = g.bfs_set_sweep_from(2)
            for k in (2, 31, 32, 33, 64):
                routed(sources(k))
            g.bfs_set_sweep_from(kstar)
        elif mode == "rules":
            srcs = sources(20)
            batch(srcs, mxvmode=2)                                  # pull-only
            batch(srcs, mxvmode=0, switchpoint=0.0)                 # every source past the switch point at once
            batch(srcs, mxvmode=1)                                  # push-only
            os.environ["GRB_SPARSE_MATRIX_FORMAT"] = "1"            # no CSC side
            A_csr, A = A, g.Matrix(n, n)
            assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
            del os.environ["GRB_SPARSE_MATRIX_FORMAT"]
            batch(srcs, mxvmode=0)
            A = A_csr
        elif mode == "caps":
            for cap in (1, 2, 3):
                batch(sources(20), cap=cap, mxvmode=0)
                batch(sources(1), cap=cap, mxvmode=0)
        elif mode == "labels_ahead" and limit == default:
            # the label pass enqueued behind a light-level launch: the launch ends the sweep (the pass runs), hands a level
            # back to the host (limit 64: it must leave at once, again and again), ends on the cap (the pass runs, the
            # cap's unlabel pass follows)
            batch(sources(2), tag="ends", mxvmode=0)
            batch(sources(20), tag="ends", mxvmode=0)
            g.bfs_batch_set_tail(64)
            batch(sources(2), tag="handsback", mxvmode=0)
            batch(sources(20), tag="limit64", mxvmode=0)
            g.bfs_batch_set_tail(default)
            for cap in (4, 9):
                batch(sources(2), cap=cap, tag="capped", mxvmode=0)
        elif mode == "trace":
            batch(sources(2), tag="k2 limit=%d" % limit, mxvmode=0)
            batch(sources(20), tag="k20 limit=%d" % limit, mxvmode=0)
            batch(sources(20), tag="pullonly limit=%d" % limit, mxvmode=2)
            batch(sources(20), tag="switch0 limit=%d" % limit, mxvmode=0, switchpoint=0.0)
finally:
    g.bfs_batch_set_tail(default)
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


AHEAD = pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])


@AHEAD
@pytest.mark.parametrize("graph", ["pieces", "path", "grid"])
def test_source_sets_through_both_entrances(graph, ahead):
    """k = 1, 2, 31, 32, 33, 64 through grb_bfs_batch, every special source alone, and from k = 2 as a routed sweep: rows of
    0, 1, 255, 256, 257, 1025 and 4997 edges, a vertex named twice and three times, adjacent sources, an isolated one, a
    stored self-loop."""
    run_child(graph, "sizes", ahead)


@AHEAD
@pytest.mark.parametrize("graph", ["pieces", "star"])
def test_rules(graph, ahead):
    """pull-only and a switch point of 0 (level 1 pulls: seed words), push-only and a matrix without its CSC side (level 1
    is the plain launch, nothing is launched ahead); on the star the hub's row is over the budget."""
    run_child(graph, "rules", ahead)


@AHEAD
@pytest.mark.parametrize("graph", ["pieces", "path"])
def test_iteration_caps(graph, ahead):
    """max_niter = 1, 2, 3: what level 1 discovers under cap 1 is never assigned, the sources always are."""
    run_child(graph, "caps", ahead)


HOST_LEVEL = re.compile(r"batch level (\d+): pull (\d+) sources, push (\d+) .*big in-rows open (\(not counted\) )?(\d+), "
                        r"big out-rows found (-?\d+), next level (pulled ahead|host|light|none)")


def traced_sweeps(graph, ahead, mode="trace"):
    """{tag: [the trace lines of each sweep]}"""
    sweeps, cur = {}, None
    for line in run_child(graph, mode, ahead, trace=True).splitlines():
        if line.startswith("@@ "):
            cur = sweeps.setdefault(line[3:], [])
            cur.append([])
        elif cur is not None and line.startswith("batch level") and "owner-computes" not in line:
            cur[-1].append(line)
    return sweeps


@AHEAD
@pytest.mark.parametrize("graph", ["pieces", "path", "grid"])
def test_level_one_is_a_host_level_and_the_launch_starts_at_two(graph, ahead):
    """Every source pushed at level 1: the sweep's first line is the host-level line of the plain launch, at limit 0 and at
    the default, and no light-level launch starts at level 1.  At the default limit the levels after it run in light-level
    launches, from the kept words.  On the pieces graph the hub is among level 1's discoveries: a big out-row found."""
    sweeps = traced_sweeps(graph, ahead)
    default = [t for t in sweeps if t.startswith("k2 limit=") and t != "k2 limit=0"][0].split("=")[1]
    for k in (2, 20):
        for limit in ("0", default):
            runs = sweeps["k%d limit=%s" % (k, limit)]
            assert len(runs) == 2
            for sweep in runs:
                assert sweep and sweep[0].startswith("batch level 1: pull 0 sources, push %d " % k), sweep[:2]
                assert not any(x.startswith("batch levels 1") for x in sweep), sweep
                m = HOST_LEVEL.match(sweep[0])
                assert m, sweep[0]
                if graph == "pieces" and k == 20:
                    assert int(m.group(6)) > 0, sweep[0]
                if graph != "pieces" and limit != "0":
                    assert any(x.startswith("batch levels 2..") for x in sweep), sweep
    for tag in ("pullonly", "switch0"):
        for sweep in sweeps["%s limit=0" % tag]:
            m = HOST_LEVEL.match(sweep[0])
            assert m and int(m.group(1)) == 1 and int(m.group(2)) == 20 and int(m.group(3)) == 0, sweep[0]


@AHEAD
def test_sources_over_the_budget_take_the_path_with_seed_words(ahead):
    """The star: the hub's 4098 out-edges are over the budget at level 1, so the hub is pulled (qmask != 0) and level 1
    runs through the general kernels."""
    sweeps = traced_sweeps("star", ahead)
    for tag, runs in sweeps.items():
        if not tag.startswith("k"):
            continue
        for sweep in runs:
            m = HOST_LEVEL.match(sweep[0])
            assert m and int(m.group(1)) == 1 and int(m.group(2)) > 0, sweep[0]


@AHEAD
@pytest.mark.parametrize("graph", ["grid", "path"])
def test_label_pass_behind_a_light_level_launch(graph, ahead):
    """Three kinds of sweep, labels against the oracle with the pass enqueued ahead and with GRB_BATCH_AHEAD=0: the last
    light-level launch ends the sweep (status 0), a launch hands a level back to the host (status 2, limit 64 on the grid;
    the path never crosses 64 out-edges with two sources), the cap falls inside a launch (status 1)."""
    sweeps = traced_sweeps(graph, ahead, mode="labels_ahead")
    status = lambda sweep: [int(re.search(r"status (\d)", x).group(1)) for x in sweep if "one launch (light levels)" in x]
    for sweep in sweeps["ends"]:
        assert status(sweep)[-1:] == [0], sweep
    if graph == "grid":
        assert all(2 in status(sweep) for sweep in sweeps["handsback"]), sweeps["handsback"]
    for sweep in sweeps["capped"]:
        assert status(sweep)[-1:] == [1], sweep
