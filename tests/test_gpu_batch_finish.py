"""GPU suite (-m gpu): the sweep's finishing rule (bfs_batch.hip, batch_decide.hpp: batch_decide_finish) and the counter
it reads.  U = the in-edges of the rows a level's pull leaves open; after a level that pulled every live source it is
complete, and when it is at most finish_limit * nvals the next level pulls the sources the per-source rule would push:
no push stage.  GRB_BATCH_FINISH=0 switches the rule off, GRB_BATCH_FINISH_LIMIT sets the limit; both are read once, so
every run is a fresh child process with its own time limit, each once more with GRB_BATCH_AHEAD=0.

Every child checks the depth vectors of every source against the oracle and prints each sweep's result blocks; a case
runs with the rule on and off and the blocks must be equal.  Both entrances: grb_bfs_batch and the queue's routed sweep
-- except the iteration caps and the pull-only sweeps, which run through grb_bfs_batch alone: the queue routes only
uncapped push-pull traversals to the sweep (bfs_persist.hip), so there is no routed form of them.
Small graphs never leave the light-level launch at its default limit, so the cases that read level lines set the limit
to 0 (every level through the host loop).

Graphs.  W: RMAT-12, edge factor 16, seed 1, symmetrised; the sources are the neighbour of the first degree-1 vertex, that
vertex (its traversal is the neighbour's, one level late), the maximum-degree vertex and random ones -- chosen with
tools/batch_rule_model.py: level 4 pulls every live source and leaves U = 5 .. 53 of 96 444 entries, at level 5 the
per-source rule pulls some and pushes the rest, at k = 2, 20, 33 and 64.  hub / hubsplit: RMAT-13 plus a vertex adjacent
to all others (an 8192-entry in-row: the slice and apply kernels; in hubsplit a source in a component of three never
reaches it, so it stays open and the apply kernel counts it while that source lives).  twin: two copies of W joined by
a path of six vertices.  grid: a thinned 48 x 48 grid."""
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import graphblast_amd as g
from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges, random_sources
from oracle import simple_reference as sr

graph, mode = sys.argv[1], sys.argv[2]
KEYS = ("levels", "reached", "edges_traversed")


def rmat(scale, seed):
    s, d, n = rmat_edges(scale, 16, seed=seed)
    return np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64), n


def csr_of(name):
    extra = []
    if name == "grid":
        s, d, n = grid_edges(48, keep=0.6, seed=3)
        s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
    elif name == "W":
        s, d, n = rmat(12, 1)
    elif name == "twin":                                            # copy 1, copy 2, a path of six between their vertices 0
        s, d, n1 = rmat(12, 1)
        path = np.arange(2 * n1, 2 * n1 + 6, dtype=np.int64)
        s = np.concatenate([s, s + n1, [0], path[:-1], [path[-1]]])
        d = np.concatenate([d, d + n1, [path[0]], path[1:], [n1]])
        n = 2 * n1 + 6
    else:
        s, d, n = rmat(13, 3)
        s = np.concatenate([s, np.full(n, n, dtype=np.int64)])      # vertex n, adjacent to every other
        d = np.concatenate([d, np.arange(n, dtype=np.int64)])
        n += 1
        if name == "hubsplit":                                      # a component of three, apart from everything
            s = np.concatenate([s, [n, n + 1]])
            d = np.concatenate([d, [n + 1, n + 2]])
            extra = [n + 1]
            n += 3
    ptr, ind = [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=True)["csr"]]
    return ptr, ind, extra


ptr, ind, extra = csr_of(graph)
n = ptr.size - 1
deg = np.diff(ptr)
A = g.Matrix(n, n)
assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
oracle = {}


def want(s_):
    if s_ not in oracle:
        oracle[s_] = sr.bfs(ptr, ind, s_)[0]
    return oracle[s_]


def sources(count):
    if graph in ("W", "twin"):
        n1 = n if graph == "W" else (n - 6) // 2
        d1 = deg[:n1] if graph == "W" else np.diff(ptr[:n1 + 1])
        leaf = int(np.nonzero(deg[:n1] == 1)[0][0])                 # (in twin, vertex 0 of copy 1 has one more edge; it is no leaf either way)
        first = [int(ind[ptr[leaf]]), leaf, int(np.argmax(d1))]
        rest = [x for x in random_sources(ptr[:n1 + 1], 61, seed=5)]
        out = first + rest
    elif graph == "grid":
        out = random_sources(ptr, 64, seed=11)
    else:
        out = [int(np.argmax(deg))] + extra + random_sources(ptr, 64, seed=11)
    assert graph != "twin" or max(out[:count]) < (n - 6) // 2
    return out[:count]


def want_u(srcs):
    """per level L: [sources live in it, U if the level pulls them all]: the in-degrees of the rows (in-degree > 0) that
    some live source has not reached after the level (depth label L + 1 or less)"""
    D = np.stack([want(s_) for s_ in srcs])
    out = {}
    for L in range(1, int(D.max()) + 1):
        live = np.nonzero((D == L).any(axis=1))[0]
        if live.size == 0:
            break
        open_rows = ((D[live] == 0) | (D[live] > L + 1)).any(axis=0) & (deg > 0)
        out[L] = [int(live.size), int(deg[open_rows].sum())]
    return out


def descriptor(**args):
    d = g.Descriptor()
    assert d.loadArgs(struconly=1, opreuse=1, **args) == 0
    return d


def batch(tag, srcs, cap=None, **args):
    print("@@ %s" % tag, file=sys.stderr, flush=True)
    if cap is not None:
        args["max_niter"] = cap
    d = descriptor(**args)
    vs = [g.Vector(n) for _ in srcs]
    info, res = g.bfs_batch(vs, A, srcs, d)
    assert info == 0, info
    for v, s_ in zip(vs, srcs):
        w = want(s_)
        assert np.array_equal(v.extractTuples()[1], w if cap is None else np.where(w <= cap, w, 0)), (tag, s_)
    if cap is None:
        assert res["reached"] == sum(int(np.count_nonzero(want(s_))) for s_ in srcs), tag
        assert res["edges_traversed"] == sum(int(deg[want(s_) != 0].sum()) for s_ in srcs), tag
    print("RESULT " + json.dumps({"tag": tag, "res": [[int(res[k]) for k in KEYS]], "sources": [int(x) for x in srcs], "nvals": int(ind.size), "want_u": want_u(srcs) if cap is None else {}}), flush=True)


def routed(tag, srcs, **args):
    print("@@ %s" % tag, file=sys.stderr, flush=True)
    d = descriptor(mxvmode=0, **args)
    vs = [g.Vector(n) for _ in srcs]
    kstar = g.bfs_set_sweep_from(2)
    try:
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
        assert (c1["sweeps"] - c0["sweeps"], c1["traversals"] - c0["traversals"]) == ((len(srcs) + 47) // 48, len(srcs)), (c0, c1)
    finally:
        g.bfs_set_sweep_from(kstar)
    for v, r, s_ in zip(vs, res, srcs):
        w = want(s_)
        assert np.array_equal(v.extractTuples()[1], w), (tag, s_)
        assert r["reached"] == int(np.count_nonzero(w)) and r["edges_traversed"] == int(deg[w != 0].sum()), (tag, s_, r)
    print("RESULT " + json.dumps({"tag": tag, "res": [[int(r[k]) for k in KEYS] for r in res], "nvals": int(ind.size),
                                  "want_u": want_u(srcs) if len(srcs) <= 48 else {}}), flush=True)


before = g.bfs_batch_set_tail(-1)
try:
    if mode == "sizes":                                             # every level through the host loop; k = 2, 20, 33, 64, both entrances
        g.bfs_batch_set_tail(0)
        for k in (2, 20, 33, 64):
            batch("batch k=%d" % k, sources(k), mxvmode=0)
            routed("routed k=%d" % k, sources(k))
        g.bfs_batch_set_tail(before)                                # ... and with the light-level launch at its default
        for k in (20, 64):
            batch("tail batch k=%d" % k, sources(k), mxvmode=0)
            routed("tail routed k=%d" % k, sources(k))
    elif mode == "counter":                                         # U on every level that pulls everybody: push-pull and pull-only
        g.bfs_batch_set_tail(0)
        for k in (2, 20, 64):
            batch("batch k=%d" % k, sources(k), mxvmode=0)
            batch("pullonly k=%d" % k, sources(k), mxvmode=2)
        routed("routed k=20", sources(20))
    elif mode == "grid":                                            # a switch point nobody passes, two sources: far under the budget
        for limit in (0, 64):
            g.bfs_batch_set_tail(limit)
            batch("batch limit=%d" % limit, sources(2), mxvmode=0, switchpoint=0.9)
        g.bfs_batch_set_tail(0)
        routed("routed", sources(2), switchpoint=0.9)
    elif mode == "caps":                                            # max_niter = 1 .. levels + 1
        g.bfs_batch_set_tail(0)
        srcs = sources(20)
        depth = max(int(want(s_).max()) for s_ in srcs)
        for cap in range(1, depth + 2):
            batch("cap=%d" % cap, srcs, cap=cap, mxvmode=0)
    elif mode == "edge":
        # twin has twice W's vertices: half the switch point keeps it at W's 41 vertices, so the first copy is flooded level
        # by level as W is -- level 4 pulls all twenty, level 5 pulls eleven and pushes nine
        sw = dict(switchpoint=0.005) if graph == "twin" else {}
        g.bfs_batch_set_tail(0)
        batch("batch k=20", sources(20), mxvmode=0, **sw)
        routed("routed k=20", sources(20), **sw)
finally:
    g.bfs_batch_set_tail(before)
print("OK")
'''

LEVEL = re.compile(r"batch level (\d+): pull (\d+) sources, push (\d+) \((\d+) edges, (claims|direct)\).* us, U (\d+)( \(not complete\))?$")
PUSH_STAGE = re.compile(r"batch push stage of level (\d+): batch_push_kernel")


class Run:
    """one child: {tag: result block}, {tag: [sweep, ...]}, a sweep = ([(level, pull, push, edges, U, complete)], {levels with a push stage}, its raw lines)"""

    def __init__(self, graph, mode, ahead, finish=True, limit=None):
        env = dict(os.environ)
        for name in ("GRB_BATCH_AHEAD", "GRB_BATCH_FINISH", "GRB_BATCH_FINISH_LIMIT", "GRB_BATCH_BUDGET"):
            env.pop(name, None)
        env["GRB_BATCH_TRACE"] = "1"
        if not ahead:
            env["GRB_BATCH_AHEAD"] = "0"
        if not finish:
            env["GRB_BATCH_FINISH"] = "0"
        if limit is not None:
            env["GRB_BATCH_FINISH_LIMIT"] = repr(limit)
        out = subprocess.run([sys.executable, "-c", CHILD, graph, mode], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2500:]
        self.results = {}
        for line in out.stdout.splitlines():
            if line.startswith("RESULT "):
                r = json.loads(line[7:])
                self.results[r["tag"]] = r
        self.sweeps, cur = {}, None
        for line in out.stderr.splitlines():
            if line.startswith("@@ "):
                cur = self.sweeps.setdefault(line[3:], [])
            elif cur is not None and line.startswith("batch "):
                if re.match(r"batch levels? 1[ .:]", line):
                    cur.append(([], set(), []))
                if not cur:
                    continue
                cur[-1][2].append(line)
                m = LEVEL.match(line)
                if m:
                    cur[-1][0].append((int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(6)), m.group(7) is None))
                    # U is complete exactly when the level pulled every live source
                    assert (m.group(7) is None) == (int(m.group(3)) == 0 and int(m.group(2)) > 0), line
                m = PUSH_STAGE.match(line)
                if m:
                    cur[-1][1].add(int(m.group(1)))


def same_results(on, off):
    assert set(on.results) == set(off.results) and on.results
    for tag, r in on.results.items():
        assert r["res"] == off.results[tag]["res"], (tag, r["res"], off.results[tag]["res"])


def mixed_after_all_pulled(levels):
    """the levels with pull > 0 and push > 0 whose level before pulled every live source"""
    return [levels[i][0] for i in range(1, len(levels)) if levels[i - 1][1] > 0 and levels[i - 1][2] == 0 and levels[i - 1][0] + 1 == levels[i][0]
            and levels[i][1] > 0 and levels[i][2] > 0]


def check_u(run):
    """every level that pulled all live sources: the sources pulled and U against numpy on the oracle's depths"""
    checked = 0
    for tag, sweeps in run.sweeps.items():
        want = run.results[tag]["want_u"]
        if not want:
            continue
        for levels, _, _ in sweeps:
            for lv, pull, push, _, u, complete in levels:
                if complete:
                    assert [pull, u] == want[str(lv)], (tag, lv, pull, u, want[str(lv)])
                    checked += 1
    return checked


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_the_rule_fires(ahead):
    """W, k = 2, 20, 33, 64, both entrances.  Rule off: some level after an all-pulled level pulls and pushes.  Rule on: that
    level pushes nothing and logs no push stage; depths, levels, reached and edges are what they were."""
    on, off = Run("W", "sizes", ahead), Run("W", "sizes", ahead, finish=False)
    same_results(on, off)
    for tag, sweeps_off in off.sweeps.items():
        sweeps_on = on.sweeps[tag]
        assert len(sweeps_on) == len(sweeps_off) == (2 if tag.endswith("routed k=64") else 1), tag
        fired = []                                                  # per sweep
        for (lv_off, st_off, _), (lv_on, st_on, raw_on) in zip(sweeps_off, sweeps_on):
            fired.append(0)
            for L in mixed_after_all_pulled(lv_off):
                assert L in st_off, (tag, L)
                at = [x for x in lv_on if x[0] == L]
                assert at and at[0][2] == 0 and at[0][1] > 0 and L not in st_on, (tag, L, raw_on)
                # ... and it pulled what the per-source rule would have pulled and pushed together
                assert at[0][1] == [x for x in lv_off if x[0] == L][0][1] + [x for x in lv_off if x[0] == L][0][2], (tag, L)
                fired[-1] += 1
            assert not mixed_after_all_pulled(lv_on), (tag, raw_on)   # U is far under the limit on this graph
        # 64 queued are a sweep of 48 and one of 16: the first, with the leaf and its neighbour among its sources, must fire
        assert fired[0] >= 1, (tag, sweeps_off)
    assert check_u(on) > 0 and check_u(off) > 0


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
@pytest.mark.parametrize("graph", ["W", "hub", "hubsplit"])
def test_u_is_exact(graph, ahead):
    """Every level that pulled all live sources, push-pull and pull-only: U on the trace line is the sum, over the vertices
    some source of the level had not reached after it, of their in-degrees.  hubsplit: the 8192-entry row stays open while
    the source that cannot reach it lives, counted by the apply kernel.  hub: the row gets every bit in the first levels,
    and the later levels run without the slice kernels (in_done); for U that path is vacuous -- in_done means no big row
    can be open, so the big rows the pull kernel then takes itself add 0 by construction -- and hub only shows that U
    stays right across the switch."""
    on, off = Run(graph, "counter", ahead), Run(graph, "counter", ahead, finish=False)
    same_results(on, off)
    assert check_u(on) >= 6 and check_u(off) >= 6
    if graph == "hubsplit":                                         # the row that never closes, while the source that cannot reach it lives
        levels = on.sweeps["pullonly k=2"][0][0]
        assert levels[0][5] and levels[0][4] >= 8192, levels


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_a_large_u_keeps_the_pushed_sources(ahead):
    """twin, every source in the first copy: when they have flooded it, every live source is pulled and the second copy's
    rows are all open -- half the matrix.  The level after keeps its pushed sources."""
    on, off = Run("twin", "edge", ahead), Run("twin", "edge", ahead, finish=False)
    same_results(on, off)
    for tag, sweeps_off in off.sweeps.items():
        (lv_off, _, _), (lv_on, st_on, raw_on) = sweeps_off[0], on.sweeps[tag][0]
        nvals = on.results[tag]["nvals"]
        held = 0
        for L in mixed_after_all_pulled(lv_off):
            u = [x for x in lv_on if x[0] == L - 1][0][4]
            if u > 0.01 * nvals:
                assert u >= 0.4 * nvals, (tag, L, u)
                at = [x for x in lv_on if x[0] == L][0]
                assert at[2] > 0 and at[1:4] == [x for x in lv_off if x[0] == L][0][1:4] and L in st_on, (tag, L, raw_on)
                held += 1
        assert held >= 1, (tag, lv_off)
    assert check_u(on) > 0


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_nobody_pulled_nothing_changes(ahead):
    """grid, a switch point nobody passes: every level is light or all-pushed, with the rule on as with it off -- the trace
    lines of both runs are identical apart from the times."""
    on, off = Run("grid", "grid", ahead), Run("grid", "grid", ahead, finish=False)
    same_results(on, off)

    def untimed(run):
        return {tag: [[re.sub(r"\d+\.\d+ us", "us", x) for x in raw] for _, _, raw in sweeps]
                for tag, sweeps in run.sweeps.items()}
    assert untimed(on) == untimed(off)
    for tag, sweeps in on.sweeps.items():
        assert sweeps and all(pull == 0 for levels, _, _ in sweeps for _, pull, _, _, _, _ in levels), tag
        assert any(levels or raw for levels, _, raw in sweeps)


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_iteration_caps(ahead):
    """W, k = 20, max_niter = 1 .. levels + 1: the cap falls on every level once, the level the rule changed among them."""
    on, off = Run("W", "caps", ahead), Run("W", "caps", ahead, finish=False)
    same_results(on, off)
    changed = [tag for tag, sweeps in off.sweeps.items() if mixed_after_all_pulled(sweeps[0][0])]
    assert len(changed) >= 2, list(off.sweeps)                      # the cap on the changed level, and past it
    for tag in changed:
        assert not mixed_after_all_pulled(on.sweeps[tag][0][0]), tag


@pytest.mark.parametrize("ahead", [True, False], ids=["ahead", "wait_first"])
def test_the_limits_edge(ahead):
    """U after the all-pulled level from a first run; with the limit at exactly U / nvals the rule fires, one entry lower it
    does not."""
    first = Run("W", "edge", ahead)
    tag = "batch k=20"
    nvals = first.results[tag]["nvals"]
    levels = first.sweeps[tag][0][0]
    off = Run("W", "edge", ahead, finish=False)
    L = mixed_after_all_pulled(off.sweeps[tag][0][0])[0]
    assert [x for x in levels if x[0] == L][0][2] == 0              # at the default limit it fires
    u = [x for x in levels if x[0] == L - 1][0][4]
    assert 1 <= u <= 0.01 * nvals

    def limit_for(entries):
        """the double x with entries <= x * nvals < entries + 1, as the library multiplies it out"""
        import math
        x = entries / nvals
        while x * float(nvals) < float(entries):
            x = math.nextafter(x, math.inf)
        assert float(entries) <= x * float(nvals) < float(entries + 1)
        return x
    at = Run("W", "edge", ahead, limit=limit_for(u))
    below = Run("W", "edge", ahead, limit=limit_for(u - 1))
    same_results(at, off)
    same_results(below, off)
    for t in ("batch k=20", "routed k=20"):
        a = [x for x in at.sweeps[t][0][0] if x[0] == L][0]
        b = [x for x in below.sweeps[t][0][0] if x[0] == L][0]
        assert a[2] == 0 and L not in at.sweeps[t][0][1], (t, a)
        assert b[2] > 0 and L in below.sweeps[t][0][1], (t, b)


def test_the_model_tool_agrees_with_the_trace():
    """tools/batch_rule_model.py on W with the child's twenty sources, every level through the host loop: the same sources
    pulled and pushed and the same U on every level, complete or not, as the library's trace lines."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, ROOT)
    from batch_rule_model import run_model
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    on = Run("W", "edge", True)
    s, d, n = rmat_edges(12, 16, seed=1)
    csr = finalize_edges(np.asarray(s), np.asarray(d), n, symmetrize=True)["csr"]
    line = re.compile(r"level (\d+): pull (\d+) sources, push (\d+) \((\d+) edges\).* U (\d+)( \(not complete\))?$")
    for finish, run in ((0.01, on), (-1.0, Run("W", "edge", True, finish=False))):
        model = [line.match(x) for x in run_model(csr, csr, run.results["batch k=20"]["sources"], finish_limit=finish, tail_edges=0)]
        model = [(int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)), int(m.group(5)), m.group(6) is None) for m in model if m]
        assert model and model == run.sweeps["batch k=20"][0][0], (finish, model, run.sweeps["batch k=20"][0][0])
