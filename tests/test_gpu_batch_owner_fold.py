"""GPU suite (-m gpu): the owner-computes push of heavy levels (bfs_batch.hip) on a graph that runs BOTH
instances of the owner kernel, the narrow and the wide one, over the row-major offsets table.  (The hub graphs of the other
test files cut into narrow ranges only, so the instance that dominates at bench size had no small-shape coverage.)  Every
case runs in a fresh child process under GRB_BATCH_TRACE, whose `owner-computes push` lines say how many narrow and wide
ranges were launched; the parent asserts that such a level ran in every sweep.  Labels against the oracle and the blocking
call, totals against the blocking call, everything equal between GRB_BATCH_OWNER=1 / 0 and GRB_BATCH_AHEAD=1 / 0.

(The name: the file was written for a variant in which the owners also committed the level at their write-back; that variant
measured slower and was not kept, docs/experiments.md R11 -- the graphs and cases are what the owner kernels lacked.)

Graphs (the light-level launch is switched off, grb_bfs_batch_set_tail(0): on graphs this small it would take every level):
  W       RMAT-13 (ef 16, seed 3, symmetrised) on vertices 0 .. 8191, 24 576 tail vertices of which every 8th is adjacent to
          one hub vertex, which is also adjacent to the whole core; n = 32 769.  The ranges of the core are narrow, those of
          the tail wide (the cut rule is restated below and both kinds asserted), and the hub's row reaches both.  A source
          in the tail has the hub alone in its second frontier (11 264 out-edges, pushed), two of them make the level heavy.
  Wpath   W plus a path of 20 vertices hung on a core vertex that has the hub as its only other neighbour: two traversals from
          the far end reach the hub together and push its row at level 22, past the stored level words, so the commit pass behind the owners
          labels directly (k = 2 and 24 only: one such traversal alone pushes too little for a heavy level).
  hub15   RMAT-15 plus a vertex adjacent to all others (tests/test_gpu_bfs_sweep_route.py): narrow ranges only."""
import functools
import json
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import json, os, sys, zlib
import numpy as np
sys.path.insert(0, os.getcwd())
import graphblast_amd as g
from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
from oracle import simple_reference as sr

graph, mode = sys.argv[1], sys.argv[2]
KEYS = ("levels", "reached", "edges_traversed")
CORE, TAIL, PATH = 8192, 24576, 20
OWN_ROWS, OWN_SMALL_ROWS, BIG_OUT = 8192, 2048, 512      # kOwnRows, kOwnSmallRows, kBatchBigPush


def csr_of(name):
    if name == "hub15":
        s, d, n = rmat_edges(15, 16, seed=3)
        s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
        s = np.concatenate([s, np.full(n, n, dtype=np.int64)])      # vertex n, adjacent to every other
        d = np.concatenate([d, np.arange(n, dtype=np.int64)])
        n += 1
    else:
        s, d, n = rmat_edges(13, 16, seed=3)
        assert n == CORE
        s, d = np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)
        hub = CORE + TAIL
        to = np.concatenate([np.arange(CORE, dtype=np.int64), np.arange(CORE, hub, 8, dtype=np.int64)])
        s = np.concatenate([s, np.full(to.size, hub, dtype=np.int64)])
        d = np.concatenate([d, to])
        n = hub + 1
        if name == "Wpath":                                         # n .. n + 19, the first of them adjacent to a core vertex
            anchor = int(np.setdiff1d(np.arange(CORE), np.concatenate([s[:-to.size], d[:-to.size]]))[0])   # (one the hub alone reaches)
            s = np.concatenate([s, [anchor], np.arange(n, n + PATH - 1, dtype=np.int64)])
            d = np.concatenate([d, [n], np.arange(n + 1, n + PATH, dtype=np.int64)])
            n += PATH
    return [np.asarray(x) for x in finalize_edges(s, d, n, symmetrize=True)["csr"]]


def ranges(ptr):
    """the owner ranges as make_slices cuts them: equal in-degree mass (a 768th of the entries), at most OWN_ROWS rows"""
    n = ptr.size - 1
    p = ptr.astype(np.int64)
    target = max(1, int(p[n]) // (3 * 256))
    bounds = [0]
    while bounds[-1] < n:
        s0 = bounds[-1]
        e = min(n, s0 + OWN_ROWS)
        e2 = s0 + int(np.searchsorted(p[s0 + 1:e + 1], min(int(p[s0]) + target, 0x7fffffff), side="right"))
        bounds.append(min(e, max(e2, s0 + 1)))
    width = np.diff(np.array(bounds))
    return int((width <= OWN_SMALL_ROWS).sum()), int((width > OWN_SMALL_ROWS).sum())


ptr, ind = csr_of(graph)
n = ptr.size - 1
deg = np.diff(ptr).astype(np.int64)
hub = int(np.argmax(deg))
assert n % 64 != 0 and n >= 2 * OWN_ROWS
narrow, wide = ranges(ptr)
if graph == "hub15":
    assert narrow > 0 and wide == 0, (narrow, wide)
else:
    assert hub == CORE + TAIL and deg[hub] == CORE + TAIL // 8
    assert narrow > 0 and wide > 0 and int((deg >= BIG_OUT).sum()) > 1, (narrow, wide)
print("RANGES %d %d" % (narrow, wide))
A = g.Matrix(n, n)
assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
desc = g.Descriptor()
assert desc.loadArgs(mxvmode=0, struconly=1, opreuse=1) == 0
oracle, blocking = {}, {}


def want(s_):
    if s_ not in oracle:
        oracle[s_] = sr.bfs(ptr, ind, s_)[0]
    return oracle[s_]


def blocking_call(s_):
    if s_ not in blocking:
        vb = g.Vector(n)
        info, res = g.bfs(vb, A, s_, desc, fused=True)
        assert info == 0, info
        blocking[s_] = (vb.extractTuples()[1], res)
    return blocking[s_]


def sources(count):
    """One source whose second frontier is heavy by itself, then what makes it heavy however many are pulled: sources next
    to the hub alone (their second frontier is the hub's row: the lightest of all, pushed last of all to be pulled).  Then
    the hub, an isolated vertex, random ones, and a repeated source at the end."""
    if graph == "hub15":
        out = [int(np.nonzero((deg > 1) & (deg < 64))[0][0]), hub]
        lonely = np.nonzero(deg == 0)[0]
        out += [int(lonely[0])] if lonely.size else []
    else:
        rows = np.repeat(np.arange(n), deg)
        second = np.bincount(rows, weights=deg[ind], minlength=n)           # the out-edges of a source's second frontier
        budget = 0.15 * ind.size
        alone = np.nonzero((np.arange(n) < CORE) & (deg > 0) & (deg <= 0.01 * n) & (second > n / 2)
                           & (second + deg[hub] <= budget))[0]       # (pushed together with one tail source)
        tail_a, tail_b, isolated = CORE, CORE + 8, CORE + 1
        assert deg[tail_a] == 1 and deg[tail_b] == 1 and deg[isolated] == 0 and 2 * deg[hub] > n / 2 and 2 * deg[hub] <= budget
        if graph == "Wpath":
            out = [n - 1, n - 1, tail_a, tail_b, hub, isolated]     # the path's far end twice: heavy at level 22
        else:
            assert alone.size > 0
            out = [int(alone[0]), tail_a, tail_b, hub, isolated]
    out += random_sources(ptr, max(count - len(out) - 1, 0), seed=11)
    out.append(out[-1])
    return out[:count]


def digest(tag, vs, res):
    crc = 0
    for v in vs:
        crc = zlib.crc32(np.ascontiguousarray(v.extractTuples()[1]).tobytes(), crc)
    print("RESULT " + json.dumps({"tag": tag, "labels": crc, "res": res}), flush=True)


def batch(srcs):
    vs = [g.Vector(n) for _ in srcs]
    for rep in range(2):                                            # twice on the same buffers
        print("@@ batch%d rep%d" % (len(srcs), rep), file=sys.stderr, flush=True)
        info, res = g.bfs_batch(vs, A, srcs, desc)
        assert info == 0, info
        for v, s_ in zip(vs, srcs):
            got = v.extractTuples()[1]
            assert np.array_equal(got, want(s_)), ("labels differ from the oracle", len(srcs), rep, s_)
            assert np.array_equal(got, blocking_call(s_)[0]), ("labels differ from the blocking call", len(srcs), rep, s_)
        assert res["reached"] == sum(blocking_call(s_)[1]["reached"] for s_ in srcs), (len(srcs), rep, res)
        assert res["edges_traversed"] == sum(blocking_call(s_)[1]["edges_traversed"] for s_ in srcs), (len(srcs), rep, res)
    digest("batch%d" % len(srcs), vs, [res[k] for k in KEYS])


def queued(srcs):
    """under the default width rule: a gathered group of k* or more is one sweep (48 fill a group)"""
    vs = [g.Vector(n) for _ in srcs]
    for rep in range(2):                                            # two sweeps back to back: the second finds what the first left
        print("@@ queue%d rep%d" % (len(srcs), rep), file=sys.stderr, flush=True)
        c0 = g.bfs_sweep_counts()
        tickets = []
        for v, s_ in zip(vs, srcs):
            info, t = g.bfs_enqueue(v, A, s_, desc)
            assert info == 0 and t != 0, info
            tickets.append(t)
        res = []
        for t in tickets:
            info, r = g.bfs_wait(t)
            assert info == 0, info
            res.append(r)
        c1 = g.bfs_sweep_counts()
        assert (c1["sweeps"] - c0["sweeps"], c1["traversals"] - c0["traversals"]) == (1, len(srcs)), (c0, c1)
        for v, r, s_ in zip(vs, res, srcs):
            got = v.extractTuples()[1]
            lb, rb = blocking_call(s_)
            assert np.array_equal(got, want(s_)), ("labels differ from the oracle", len(srcs), rep, s_)
            assert np.array_equal(got, lb), ("labels differ from the blocking call", len(srcs), rep, s_)
            assert all(r[k] == rb[k] for k in KEYS), (s_, {k: (r[k], rb[k]) for k in KEYS})
    digest("queue%d" % len(srcs), vs, [[r[k] for k in KEYS] for r in res])


before = g.bfs_batch_set_tail(0)
try:
    if mode == "batch":
        for k in ((2, 24) if graph == "Wpath" else (1, 2, 24, 33, 64)):
            batch(sources(k))
    else:
        assert g.bfs_set_coschedule(-1) == 1 and 2 <= g.bfs_set_sweep_from(-1) <= 24
        for k in ((24,) if graph == "Wpath" else (24, 48)):
            queued(sources(k))
finally:
    g.bfs_batch_set_tail(before)
print("OK")
'''

VARIANTS = {"default": {}, "owner_off": {"GRB_BATCH_OWNER": "0"}, "wait_first": {"GRB_BATCH_AHEAD": "0"}}
OWNER_LINE = re.compile(r"batch level (\d+): owner-computes push, (\d+) of (\d+) big rows in the frontier, (\d+) ranges "
                        r"\((\d+) narrow, (\d+) wide\)$")


@functools.lru_cache(maxsize=None)
def child(graph, mode, variant):
    """-> (the RESULT records by tag, {sweep marker: [its owner-computes lines]}, (narrow, wide) as the child cut them)"""
    env = dict(os.environ)
    for name in ("GRB_BATCH_OWNER", "GRB_BATCH_AHEAD", "GRB_BATCH_BIG_OUT", "GRB_BATCH_BUDGET", "GRB_BATCH_TAIL", "GRB_BATCH_TAIL_EDGES"):
        env.pop(name, None)
    env.update(VARIANTS[variant])
    env["GRB_BATCH_TRACE"] = "1"
    out = subprocess.run([sys.executable, "-c", CHILD, graph, mode], capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout[-1000:] + out.stderr[-2500:]
    results, cut = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            rec = json.loads(line[7:])
            results[rec["tag"]] = rec
        elif line.startswith("RANGES "):
            cut = tuple(int(x) for x in line.split()[1:])
    sweeps, cur = {}, None
    for line in out.stderr.splitlines():
        if line.startswith("@@ "):
            cur = sweeps.setdefault(line[3:], [])
        elif cur is not None and "owner-computes" in line:
            cur.append(line)
    return results, sweeps, cut


def owner_levels_ran(graph, mode, variant):
    """every sweep of the child ran an owner-computes level, over the narrow and wide ranges the matrix has"""
    results, sweeps, cut = child(graph, mode, variant)
    assert results and sweeps
    for marker, lines in sweeps.items():
        hits = [OWNER_LINE.match(x) for x in lines]
        assert hits and all(hits), (marker, lines)
        for m in hits:
            assert (int(m.group(5)), int(m.group(6))) == cut and int(m.group(4)) == sum(cut), (marker, m.group(0), cut)
            assert int(m.group(2)) >= 1, (marker, m.group(0))
            assert (int(m.group(6)) > 0) == (graph != "hub15") and int(m.group(5)) > 0, (marker, m.group(0))
        if graph == "Wpath":
            assert max(int(m.group(1)) for m in hits) > 17, (marker, lines)      # past the stored level words


@pytest.mark.parametrize("variant", ["default", "wait_first"])
@pytest.mark.parametrize("graph", ["W", "hub15"])
def test_batch_of_every_size_runs_both_owner_instances(graph, variant):
    """grb_bfs_batch with k = 1, 2, 24, 33, 64 (a source heavy by itself, two next to the hub, the hub, an isolated vertex,
    a repeated source), twice each; W runs narrow and wide ranges, hub15 narrow ones alone."""
    owner_levels_ran(graph, "batch", variant)


@pytest.mark.parametrize("variant", ["default", "wait_first"])
@pytest.mark.parametrize("graph", ["W", "hub15"])
def test_queued_groups_under_the_default_width_rule(graph, variant):
    """24 and 48 traversals queued, each group one sweep, twice back to back on the sweep's own buffers: the second finds the
    counters and the big-row list's length as the first left them."""
    owner_levels_ran(graph, "queue", variant)


@pytest.mark.parametrize("mode", ["batch", "queue"])
def test_owner_levels_past_the_stored_level_words(mode):
    """Wpath: the heavy level is level 22 -- its discoveries are labelled directly."""
    owner_levels_ran("Wpath", mode, "default")


@pytest.mark.parametrize("mode", ["batch", "queue"])
@pytest.mark.parametrize("graph", ["W", "Wpath", "hub15"])
def test_results_do_not_depend_on_the_route(graph, mode):
    """GRB_BATCH_OWNER=0 (the slice kernels; its trace has no owner-computes line) and GRB_BATCH_AHEAD=0
    give the labels and result blocks of the default."""
    base = child(graph, mode, "default")[0]
    off, off_sweeps, _ = child(graph, mode, "owner_off")
    assert off_sweeps and not any(off_sweeps.values()), off_sweeps
    assert off == base
    assert child(graph, mode, "wait_first")[0] == base
