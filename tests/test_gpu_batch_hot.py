"""GPU suite (-m gpu): the sweep's hot block (bfs_batch.hip: make_hot, batch_hot_copy).  The vertices of largest out-degree
get a second place for their frontier word behind the n words of every level-word array, and the pull kernels gather
through copies of the CSC indices and of the hint that name hub j as n + j.  Nothing but placement may change: depth
vectors, result blocks and the GRB_BATCH_TRACE level lines (masks, pairs, edges, U) are what they are with
GRB_BATCH_HOT=0.  The switches are read once per process, so every setting is a fresh child with its own time limit.

Every child checks the depth vectors of every source against the oracle's BFS and the exported query (H, t, the hub list)
against numpy.  Small graphs never leave the light-level launch at its default limit, where nothing is pulled: the cases
set the limit to 0 (every level through the host loop) unless they say otherwise.

Graphs.  sym12 / dir12: RMAT-12, edge factor 16, seed 1, symmetrised / as generated (CSC != CSR: the hubs are taken by
out-degree, the gathers go through in-lists); sym13 / dir13: RMAT-13, seed 3.  hub: sym13 plus a vertex adjacent to all
others (an 8192-entry in-row: the slice kernel's gathers).  twin12: sym12 plus a copy of its maximum-degree vertex, so
the two largest out-degrees tie.  ring: a cycle of 4096, all degrees equal (H = 0).
Sources: the maximum-degree vertex (a hub that is itself a source), an isolated vertex, a random one twice, random ones."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import hashlib, json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import graphblast_amd as g
from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
from oracle import simple_reference as sr

graph, mode = sys.argv[1], sys.argv[2]
KEYS = ("levels", "reached", "edges_traversed")


def csr_of(name):
    if name == "ring":
        n = 4096
        s = np.arange(n, dtype=np.int64)
        d = (s + 1) % n
        sym = True
    else:
        scale, seed = (13, 3) if name in ("sym13", "dir13", "hub") else (12, 1)
        s, d, n = rmat_edges(scale, 16, seed=seed)
        s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
        sym = not name.startswith("dir")
        if name == "hub":                                           # vertex n, adjacent to every other
            s = np.concatenate([s, np.full(n, n, dtype=np.int64)])
            d = np.concatenate([d, np.arange(n, dtype=np.int64)])
            n += 1
        if name == "twin12":                                        # vertex n: the maximum-degree vertex's neighbours, not the vertex itself
            p0, i0 = [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=True)["csr"]]
            top = int(np.argmax(np.diff(p0)))
            nb = i0[p0[top]:p0[top + 1]].astype(np.int64)
            assert top not in nb
            s = np.concatenate([s, np.full(nb.size, n, dtype=np.int64)])
            d = np.concatenate([d, nb])
            n += 1
    return [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=sym)["csr"]]


def make(name):
    ptr, ind = csr_of(name)
    A = g.Matrix(ptr.size - 1, ptr.size - 1)
    assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
    return dict(name=name, ptr=ptr, ind=ind, n=ptr.size - 1, deg=np.diff(ptr), A=A, oracle={})


def want(G, s_):
    if s_ not in G["oracle"]:
        G["oracle"][s_] = sr.bfs(G["ptr"], G["ind"], s_)[0]
    return G["oracle"][s_]


def sources(G, count):
    deg = G["deg"]
    if G["name"] == "ring":
        return [int(x) for x in np.arange(count) * 61 % G["n"]]
    rnd = random_sources(G["ptr"], 64, seed=11)
    indeg = np.bincount(G["ind"], minlength=G["n"])
    iso = [int(x) for x in np.nonzero((deg == 0) & (indeg == 0))[0][:1]]   # (hub has none)
    out = [int(np.argmax(deg))] + iso + [rnd[0], rnd[0]] + rnd[1:]
    return out[:count]


def leaves(G):
    return [int(x) for x in np.nonzero(G["deg"] == 1)[0][:2]]


def rule(deg, cap):
    """t = the smallest threshold with at most cap vertices of out-degree >= t; the hubs, ascending"""
    t = 0 if cap >= deg.size else int(np.sort(deg)[::-1][cap]) + 1
    return t, np.nonzero(deg >= t)[0]


def query(G):
    q = g.bfs_batch_hot(G["A"])
    off = os.environ.get("GRB_BATCH_HOT") == "0"
    if off:
        assert q["H"] == 0 and q["cap"] == 0, q
    else:
        t, hubs = rule(G["deg"], q["cap"])
        assert q["cap"] == int(os.environ.get("GRB_BATCH_HOT_MAX", q["cap"])), q
        assert (q["H"], q["t"]) == (hubs.size, t) and np.array_equal(q["hubs"], hubs), (q["H"], q["t"], hubs.size, t)
    ds = np.sort(G["deg"])[::-1]
    print("QUERY " + json.dumps({"graph": G["name"], "H": q["H"], "t": q["t"], "cap": q["cap"], "n": G["n"],
                                 "top": [int(x) for x in ds[:8]], "hub_source": bool(q["H"]) and int(np.argmax(G["deg"])) in q["hubs"]}), flush=True)
    return q


def digest(vs):
    h = hashlib.sha1()
    for v in vs:
        h.update(np.ascontiguousarray(v.extractTuples()[1]).tobytes())
    return h.hexdigest()


def descriptor(**args):
    d = g.Descriptor()
    assert d.loadArgs(struconly=1, opreuse=1, **args) == 0
    return d


def batch(G, tag, srcs, **args):
    print("@@ %s" % tag, file=sys.stderr, flush=True)
    n, deg = G["n"], G["deg"]
    vs = [g.Vector(n) for _ in srcs]
    info, res = g.bfs_batch(vs, G["A"], srcs, descriptor(**args))
    assert info == 0, info
    for v, s_ in zip(vs, srcs):
        assert np.array_equal(v.extractTuples()[1], want(G, s_)), (tag, s_)
    assert res["reached"] == sum(int(np.count_nonzero(want(G, s_))) for s_ in srcs), tag
    assert res["edges_traversed"] == sum(int(deg[want(G, s_) != 0].sum()) for s_ in srcs), tag
    print("RESULT " + json.dumps({"tag": tag, "res": [[int(res[k]) for k in KEYS]], "labels": digest(vs)}), flush=True)


def routed(G, tag, srcs, **args):
    print("@@ %s" % tag, file=sys.stderr, flush=True)
    n, deg = G["n"], G["deg"]
    d = descriptor(mxvmode=0, **args)
    vs = [g.Vector(n) for _ in srcs]
    kstar = g.bfs_set_sweep_from(2)
    try:
        c0 = g.bfs_sweep_counts()
        tickets = []
        for v, s_ in zip(vs, srcs):
            info, t = g.bfs_enqueue(v, G["A"], s_, d)
            assert info == 0 and t != 0, info
            tickets.append(t)
        res = []
        for t in tickets:
            info, r = g.bfs_wait(t)
            assert info == 0, info
            res.append(r)
        c1 = g.bfs_sweep_counts()
        assert (c1["sweeps"] - c0["sweeps"], c1["traversals"] - c0["traversals"]) == ((len(srcs) + 47) // 48, len(srcs)), (c0, c1)
    finally:
        g.bfs_set_sweep_from(kstar)
    for v, r, s_ in zip(vs, res, srcs):
        w = want(G, s_)
        assert np.array_equal(v.extractTuples()[1], w), (tag, s_)
        assert r["reached"] == int(np.count_nonzero(w)) and r["edges_traversed"] == int(deg[w != 0].sum()), (tag, s_, r)
    print("RESULT " + json.dumps({"tag": tag, "res": [[int(r[k]) for k in KEYS] for r in res], "labels": digest(vs)}), flush=True)


before = g.bfs_batch_set_tail(-1)
try:
    if mode == "two":
        # one process, two matrices on the queue's shared buffers and on the scratch slots: the ring (H = 0) first, then the
        # other, alternately -- the stride of the word arrays changes from sweep to sweep, n does not
        R, G = make("ring"), make(graph)
        assert R["n"] == G["n"]
        for rnd in range(2):
            for X in (R, G):
                g.bfs_batch_set_tail(before if X is R else 0)       # (the ring's 2048 levels: in its one light-level launch)
                routed(X, "%s routed %d" % (X["name"], rnd), sources(X, 20))
                batch(X, "%s batch %d" % (X["name"], rnd), sources(X, 20), mxvmode=0)
                if rnd == 0:
                    query(X)
    else:
        G = make(graph)
        query(G)
        g.bfs_batch_set_tail(0)
        if mode == "sizes":                                         # k = 2, 20, 33, 64, both entrances; then the light-level launch at its default
            for k in (2, 20, 33, 64):
                batch(G, "batch k=%d" % k, sources(G, k), mxvmode=0)
                routed(G, "routed k=%d" % k, sources(G, k))
            g.bfs_batch_set_tail(before)
            batch(G, "tail batch k=20", sources(G, 20), mxvmode=0)
            routed(G, "tail routed k=20", sources(G, 20))
        elif mode == "caps":
            batch(G, "batch k=2", sources(G, 2), mxvmode=0)
            batch(G, "batch k=20", sources(G, 20), mxvmode=0)
            routed(G, "routed k=20", sources(G, 20))
            batch(G, "pullonly k=20", sources(G, 20), mxvmode=2)
        elif mode == "pullonly":                                    # level 1 pulls from the seeds' words; hub: the 8192-entry in-row is open at level 1
            for k in (2, 20, 64):
                batch(G, "pullonly k=%d" % k, sources(G, k), mxvmode=2)
            batch(G, "batch k=20", sources(G, 20), mxvmode=0)
            routed(G, "routed k=20", sources(G, 20))
        elif mode == "handback":                                    # two leaves: light levels until the frontiers' out-edges pass 2048
            g.bfs_batch_set_tail(2048)
            batch(G, "batch leaves", leaves(G), mxvmode=0)
            routed(G, "routed leaves", leaves(G))
finally:
    g.bfs_batch_set_tail(before)
print("OK")
'''

ONE_LAUNCH = re.compile(r"batch levels (\d+)\.\.(\d+): one launch \(light levels\), status (\d+)")
LEVEL = re.compile(r"batch level (\d+): pull (\d+) sources, push (\d+) ")
OWN_COPY = re.compile(r"sweep hot block: level (\d+) pulls behind a copy launch of its own")


class Run:
    """one child: {tag: result block}, {tag: its trace lines}, the queries"""

    def __init__(self, graph, mode, ahead=True, hot=True, cap=None):
        env = dict(os.environ)
        for name in ("GRB_BATCH_AHEAD", "GRB_BATCH_HOT", "GRB_BATCH_HOT_MAX", "GRB_BATCH_FINISH", "GRB_BATCH_FINISH_LIMIT", "GRB_BATCH_BUDGET"):
            env.pop(name, None)
        env["GRB_BATCH_TRACE"] = "1"
        if not ahead:
            env["GRB_BATCH_AHEAD"] = "0"
        if not hot:
            env["GRB_BATCH_HOT"] = "0"
        if cap is not None:
            env["GRB_BATCH_HOT_MAX"] = str(cap)
        out = subprocess.run([sys.executable, "-c", CHILD, graph, mode], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2500:]
        self.results, self.queries = {}, {}
        for line in out.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                self.results[r["tag"]] = r
            elif line.startswith("QUERY "):
                q = json.loads(line[6:])
                self.queries[q["graph"]] = q
        self.lines, cur = {}, None
        for line in out.stderr.splitlines():
            if line.startswith("@@ "):
                cur = self.lines.setdefault(line[3:], [])
            elif cur is not None and (line.startswith("batch ") or line.startswith("sweep hot block: level")):
                cur.append(line)

    def levels(self, tag):
        """the level lines without their times"""
        return [re.sub(r"\d+\.\d+ us", "us", x) for x in self.lines[tag] if x.startswith("batch ")]

    def pulled(self, tag):
        return [int(m.group(1)) for m in map(LEVEL.match, self.lines[tag]) if m and int(m.group(2)) > 0]


def same(on, off):
    """result blocks, depth vectors and level lines: what they are without the hot block"""
    assert set(on.results) == set(off.results) and on.results
    for tag, r in on.results.items():
        assert r["res"] == off.results[tag]["res"] and r["labels"] == off.results[tag]["labels"], tag
        assert on.levels(tag) == off.levels(tag) and on.levels(tag), tag


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["sym12", "dir12", "sym13", "dir13"])
def test_nothing_but_placement_changes(graph, ahead):
    """k = 2, 20, 33, 64 through grb_bfs_batch and as a routed sweep: oracle labels in both children, equal result blocks,
    equal level lines.  A cap of 256: some of a row's entries are renamed, most vertices are not hot (the default cap is
    above these graphs' vertex counts and makes every vertex hot: test_caps).  The hub source, the isolated and the repeated
    one are among the sources."""
    on, off = Run(graph, "sizes", ahead, cap=256), Run(graph, "sizes", ahead, hot=False)
    same(on, off)
    q = on.queries[graph]
    assert 128 < q["H"] <= 256 and q["hub_source"] and off.queries[graph]["H"] == 0
    for tag in ("batch k=2", "routed k=20", "batch k=33", "routed k=64"):
        assert on.pulled(tag), (tag, on.lines[tag])                 # the renamed arrays were gathered through


@pytest.mark.parametrize("graph,cap", [("sym12", 1), ("dir12", 1), ("sym12", 64), ("dir13", 64), ("sym12", 1 << 20), ("dir12", 4096)])
def test_caps(graph, cap):
    """one hot word, 64, every vertex: the query equals numpy (asserted in the child), the sweeps equal the ones without"""
    on, off = Run(graph, "caps", cap=cap), Run(graph, "caps", hot=False)
    same(on, off)
    q = on.queries[graph]
    assert q["cap"] == cap
    if cap == 1:
        assert (q["H"], q["t"]) == (1, q["top"][1] + 1) and q["top"][0] > q["top"][1]
    elif cap == 64:
        assert 32 < q["H"] <= 64
    else:
        assert (q["H"], q["t"]) == (q["n"], 0)


def test_a_cap_on_a_tie():
    """Ties at the threshold stay out together.  sym12, cap 6: the sixth and seventh largest out-degrees are equal, so five
    hubs.  twin12, cap 1: the two largest are equal, so none -- H = 0, and the k = 2 sweep is the one without a hot block."""
    on = Run("sym12", "caps", cap=6)
    q = on.queries["sym12"]
    assert q["top"][5] == q["top"][6] and q["top"][4] > q["top"][5]
    assert (q["H"], q["t"]) == (5, q["top"][5] + 1)
    on, off = Run("twin12", "caps", cap=1), Run("twin12", "caps", hot=False)
    q = on.queries["twin12"]
    assert q["top"][0] == q["top"][1]                               # the tie
    assert (q["H"], q["t"], q["cap"]) == (0, q["top"][0] + 1, 1)
    same(on, off)
    assert on.pulled("batch k=2")


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["sym12", "dir12", "hub"])
def test_level_one_pulls_behind_its_own_copy(graph, ahead):
    """A pull-only rule: level 1 pulls from the seeds' words, which no totals launch has copied -- the copy is a launch of
    its own, and the hub source's seed bit is read through the tail.  hub: at level 1 the 8192-entry in-row is open for
    every source but its neighbours, and the slice kernel gathers through the renamed ids.  A cap of 64: some of a row's
    entries are hubs, most are not."""
    on, off = Run(graph, "pullonly", ahead, cap=64), Run(graph, "pullonly", ahead, hot=False)
    same(on, off)
    assert on.queries[graph]["H"] > 0 and on.queries[graph]["hub_source"]
    for tag in ("pullonly k=2", "pullonly k=20", "pullonly k=64"):
        assert on.pulled(tag)[0] == 1, on.lines[tag]
        own = [int(m.group(1)) for m in map(OWN_COPY.match, on.lines[tag]) if m]
        assert own == [1], (tag, on.lines[tag])                     # every later level's tail is the totals launch's
    assert not any(OWN_COPY.match(x) for tag in off.lines for x in off.lines[tag])


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["sym12", "dir12"])
def test_a_level_handed_back_pulls_behind_its_own_copy(graph, ahead):
    """Two leaves, 2048 out-edges to a light-level launch: the launch hands a level back (status 2) and the host level that
    follows pulls from the array the launch wrote -- behind a copy launch of its own.  The route is read off the trace."""
    on, off = Run(graph, "handback", ahead, cap=64), Run(graph, "handback", ahead, hot=False)
    same(on, off)
    for tag in ("batch leaves", "routed leaves"):
        lines = on.lines[tag]
        handed = [(i, int(m.group(2))) for i, m in enumerate(map(ONE_LAUNCH.match, lines)) if m and int(m.group(3)) == 2]
        assert handed, lines
        i, last = handed[0]
        after = lines[i + 1:]
        own = [int(m.group(1)) for m in map(OWN_COPY.match, after) if m]
        nxt = [m for m in map(LEVEL.match, after) if m][0]
        assert int(nxt.group(1)) == last + 1 and int(nxt.group(2)) > 0 and own and own[0] == last + 1, lines


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_two_matrices_in_one_process(ahead):
    """ring (all degrees equal: H = 0 under a cap of 64) and sym12 (H > 0), both of 4096 vertices, swept alternately in one process, the ring
    first: the word arrays' stride changes from sweep to sweep on the same buffers, and what is known all-zero under one
    stride is not under the other."""
    on, off = Run("sym12", "two", ahead, cap=64), Run("sym12", "two", ahead, hot=False)
    same(on, off)
    assert on.queries["ring"]["H"] == 0 and on.queries["ring"]["t"] == 3 and on.queries["sym12"]["H"] > 0
    assert len(on.results) == 8
