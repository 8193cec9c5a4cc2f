"""GPU suite (-m gpu): the sweep's heavy push levels without the `seen` copy, the list pass and the lone narrow owner launch
(bfs_batch.hip).  On a heavy level the pull pass stashes the pushed sources' old seen-bits in the level's own
words and the commit pass takes them back; batch_push_kernel lists the big frontier rows it skips; few narrow ranges run in
the wide owner instance's launch (GRB_BATCH_OWNER_MERGE=0: always two launches).  Every case runs in a fresh child process
under GRB_BATCH_TRACE with its own time limit; the parent asserts from the trace that every sweep reached an owner-computes
level with at least one big row listed (a case cannot pass by never reaching the path), how many owner launches it took, and
which kinds of heavy level ran.  Labels against the oracle and the blocking call, totals against the blocking call, label
CRCs and result blocks equal across every switch setting of a case.

Graphs (restated from tests/test_gpu_batch_owner_fold.py, not imported; the light-level launch is off unless a case says so):
  W       RMAT-13 core (ef 16, seed 3, symmetrised), 24 576 tail vertices of which every 8th is adjacent to one hub, which is
          also adjacent to the whole core; n = 32 769.  747 narrow ranges and 10 wide ones: more narrow ranges than any CDNA
          part has CUs, so the rule keeps the two launches.
  Wpath   W plus a path of 20 vertices hung on a core vertex whose only other neighbour is the hub: two traversals from the far
          end push the hub's row at level 22, past the stored level words (the commit labels directly).
  hub15   RMAT-15 plus a vertex adjacent to all others: narrow ranges only, one launch either way.
  Dfew    directed: 16 hubs, 16 384 tail vertices that all point at every hub (the hubs hold nearly all in-degree mass: one
          single-row range each), the hubs point at each other, at every 32nd tail vertex and at every 128th of 16 385 "desert"
          vertices; n = 32 785.  Fewer than 64 narrow ranges and several wide ones: the rule merges.  Two tail sources push
          the 16 hub rows together at level 2 (heavy, nothing pulled); a fourth tail source is over the budget and is pulled."""
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

graph, mode, ks, tail = sys.argv[1], sys.argv[2], [int(x) for x in sys.argv[3].split(",")], sys.argv[4]
KEYS = ("levels", "reached", "edges_traversed")
CORE, TAIL, PATH = 8192, 24576, 20
HUBS, DTAIL, DESERT = 16, 16384, 16385
OWN_ROWS, OWN_SMALL_ROWS = 8192, 2048                    # kOwnRows, kOwnSmallRows
BIG_OUT = max(64, int(os.environ.get("GRB_BATCH_BIG_OUT", "512")))   # kBatchBigPush


def csr_of(name):
    if name == "Dfew":
        hubs = np.arange(HUBS, dtype=np.int64)
        tails = np.arange(HUBS, HUBS + DTAIL, dtype=np.int64)
        desert = np.arange(HUBS + DTAIL, HUBS + DTAIL + DESERT, dtype=np.int64)
        to = np.concatenate([hubs, tails[::32], desert[::128]])
        s = np.concatenate([np.repeat(tails, HUBS), np.repeat(hubs, to.size)])
        d = np.concatenate([np.tile(hubs, DTAIL), np.tile(to, HUBS)])
        keep = s != d
        return [np.asarray(x) for x in finalize_edges(s[keep], d[keep], HUBS + DTAIL + DESERT, symmetrize=False)["csr"]]
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


def ranges(in_ptr):
    """the owner ranges as make_slices cuts them: equal in-degree mass (a 768th of the entries), at most OWN_ROWS rows"""
    n = in_ptr.size - 1
    p = in_ptr.astype(np.int64)
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
in_ptr = np.concatenate([[0], np.cumsum(np.bincount(ind, minlength=n))])
narrow, wide = ranges(in_ptr)
if graph == "hub15":
    assert narrow > 0 and wide == 0, (narrow, wide)
elif graph == "Dfew":
    assert 0 < narrow < 64 and wide > 1 and int((deg >= 512).sum()) == HUBS, (narrow, wide)
else:
    assert hub == CORE + TAIL and deg[hub] == CORE + TAIL // 8
    assert narrow > 304 and wide > 0 and int((deg >= BIG_OUT).sum()) > 1, (narrow, wide)
print("RANGES %d %d" % (narrow, wide))
print("BIGROWS %d" % int((deg >= BIG_OUT).sum()))
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
    """First what makes a level heavy with nothing pulled (k = 2), then the hub, a vertex without out-edges, random ones (with
    them some source is pulled at the heavy level), and a repeated source at the end."""
    if graph == "hub15":
        out = [int(np.nonzero((deg > 1) & (deg < 64))[0][0]), hub]
        lonely = np.nonzero(deg == 0)[0]
        out += [int(lonely[0])] if lonely.size else []
    elif graph == "Dfew":
        budget = 0.15 * ind.size
        hubs_out = int(deg[:HUBS].sum())
        assert 2 * hubs_out > n / 2 and 3 * hubs_out <= budget < 4 * hubs_out
        out = [HUBS + 1, HUBS + 2, 0, n - 2, HUBS + 3, HUBS + 5]    # tail, tail, a hub, a desert vertex, two more tail vertices
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
    for rep in range(2):                                            # two sweeps back to back on the same buffers
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
    for rep in range(2):
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


if graph in ("W", "Dfew"):
    # k = 2: both sources are pushed at level 2, the heavy one; its list is the big rows among their neighbours
    s0, s1 = sources(2)
    front = np.union1d(ind[ptr[s0]:ptr[s0 + 1]], ind[ptr[s1]:ptr[s1 + 1]])
    print("LISTED2 %d" % int((deg[np.setdiff1d(front, [s0, s1])] >= BIG_OUT).sum()))
before = g.bfs_batch_set_tail(-1)
if tail == "off":
    g.bfs_batch_set_tail(0)
else:
    assert 0 < before < 11264                                       # the hub's row alone is over the light-level limit
try:
    if mode == "queue":
        assert g.bfs_set_coschedule(-1) == 1 and 2 <= g.bfs_set_sweep_from(-1) <= 24
    for k in ks:
        (batch if mode == "batch" else queued)(sources(k))
finally:
    g.bfs_batch_set_tail(before)
print("OK")
'''

VARIANTS = {
    "default": {},
    "merge_off": {"GRB_BATCH_OWNER_MERGE": "0"},
    "wait_first": {"GRB_BATCH_AHEAD": "0"},
    "owner_off": {"GRB_BATCH_OWNER": "0"},
    "big_out_64": {"GRB_BATCH_BIG_OUT": "64"},
    "big_out_64_merge_off": {"GRB_BATCH_BIG_OUT": "64", "GRB_BATCH_OWNER_MERGE": "0"},
    "tail_on": {"GRB_BATCH_TAIL_EDGES": "2000"},
    "tail_on_wait_first": {"GRB_BATCH_TAIL_EDGES": "2000", "GRB_BATCH_AHEAD": "0"},
}
SWITCHES = ("GRB_BATCH_OWNER", "GRB_BATCH_OWNER_MERGE", "GRB_BATCH_AHEAD", "GRB_BATCH_BIG_OUT", "GRB_BATCH_BIG_IN", "GRB_BATCH_BUDGET",
            "GRB_BATCH_TAIL", "GRB_BATCH_TAIL_EDGES")
OWNER_LINE = re.compile(r"batch level (\d+): owner-computes push, (\d+) of (\d+) big rows in the frontier, (\d+) ranges "
                        r"\((\d+) narrow, (\d+) wide\)$")
LAUNCH_LINE = re.compile(r"batch level (\d+): range owners in (\d+) launch(?:es)?$")
LEVEL_LINE = re.compile(r"batch level (\d+): pull (\d+) sources, push (\d+) \((\d+) edges, (claims|direct)\)")
LIGHT_LINE = re.compile(r"batch levels (\d+)\.\.(\d+): one launch \(light levels\), status (\d+)")
FACTS = {}                                  # what a child says about its graph: (graph, mode, variant, name) -> number
KS = {"W": "2,24,33,64", "Wpath": "2,24", "hub15": "2,24", "Dfew": "2,24,64"}


@functools.lru_cache(maxsize=None)
def child(graph, mode, variant):
    """-> (the RESULT records by tag, {sweep marker: its trace lines}, (narrow, wide) as the child cut them)"""
    env = dict(os.environ)
    for name in SWITCHES:
        env.pop(name, None)
    env.update(VARIANTS[variant])
    env["GRB_BATCH_TRACE"] = "1"
    ks = KS[graph] if mode == "batch" else "24,48" if graph in ("W", "Dfew") else "24"
    out = subprocess.run([sys.executable, "-c", CHILD, graph, mode, ks, "on" if variant.startswith("tail_on") else "off"],
                         capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout[-1000:] + out.stderr[-2500:]
    results, cut = {}, None
    for line in out.stdout.splitlines():
        if line.startswith("RESULT "):
            rec = json.loads(line[7:])
            results[rec["tag"]] = rec
        elif line.startswith("RANGES "):
            cut = tuple(int(x) for x in line.split()[1:])
        elif line.startswith("BIGROWS ") or line.startswith("LISTED2 "):
            FACTS[(graph, mode, variant, line.split()[0])] = int(line.split()[1])
    sweeps, cur = {}, None
    for line in out.stderr.splitlines():
        if line.startswith("@@ "):
            cur = sweeps.setdefault(line[3:], [])
        elif cur is not None and line.startswith("batch level"):
            cur.append(line)
    assert results and sweeps and cut
    return results, sweeps, cut


def heavy_levels(lines):
    """[(level, sources pulled)] of a sweep's claims-only levels"""
    hits = [LEVEL_LINE.match(x) for x in lines]
    return [(int(m.group(1)), int(m.group(2))) for m in hits if m and m.group(5) == "claims"]


def owner_levels_ran(graph, mode, variant):
    """Every sweep ran an owner-computes level with big rows listed, over the ranges the matrix has, and its owners were
    launched as the rule says: once when the narrow ranges are fewer than the CUs (Dfew: fewer than 64) and the switch allows
    it, or when the matrix has one kind of range only; else twice.  -> the RESULT records"""
    results, sweeps, cut = child(graph, mode, variant)
    narrow, wide = cut
    merged = "merge_off" not in variant and 0 < narrow < 64 and wide > 0
    launches = 1 if merged or narrow == 0 or wide == 0 else 2
    for marker, lines in sweeps.items():
        owner = [x for x in lines if "owner-computes" in x]
        hits = [OWNER_LINE.match(x) for x in owner]
        assert hits and all(hits), (marker, lines)
        for m in hits:
            assert (int(m.group(5)), int(m.group(6))) == cut and int(m.group(4)) == sum(cut), (marker, m.group(0), cut)
            assert 1 <= int(m.group(2)) <= int(m.group(3)), (marker, m.group(0))      # at least one big row listed
        how = [LAUNCH_LINE.match(x) for x in lines if "range owners" in x]
        assert len(how) == len(hits) and all(how), (marker, lines)
        assert all(int(m.group(2)) == launches for m in how), (marker, launches, lines)
        assert sorted(int(m.group(1)) for m in how) == sorted(int(m.group(1)) for m in hits)
        claims = {lv for lv, _ in heavy_levels(lines)}
        assert all(int(m.group(1)) in claims for m in hits), (marker, lines)        # an owner level is a claims-only level
        assert all(int(m.group(3)) == FACTS[(graph, mode, variant, "BIGROWS")] for m in hits), (marker, lines)
        if marker.startswith("batch2 ") and (graph, mode, variant, "LISTED2") in FACTS:
            # the list batch_push_kernel wrote is exactly the big rows of the two sources' neighbourhoods
            assert [(int(m.group(1)), int(m.group(2))) for m in hits] == [(2, FACTS[(graph, mode, variant, "LISTED2")])], (marker, lines)
    return results


@pytest.mark.parametrize("graph", ["W", "hub15", "Dfew"])
def test_owner_merge_unset_against_off(graph):
    """(a) W keeps two launches either way (747 narrow ranges), hub15 has the narrow instance alone either way, Dfew runs
    its narrow ranges in the wide instance's launch unless the switch forbids it.  The same labels and result blocks."""
    assert owner_levels_ran(graph, "batch", "default") == owner_levels_ran(graph, "batch", "merge_off")


@pytest.mark.parametrize("variant", ["big_out_64", "big_out_64_merge_off"])
def test_list_append_with_many_big_rows(variant):
    """(b) GRB_BATCH_BIG_OUT=64 on W: 904 rows of 64 entries or more instead of 24, the last chunk of batch_push_kernel partly
    out of range (n = 32 769).  The heavy levels of W push the neighbourhoods of single sources, so their lists stay short
    (eleven rows at k = 2, asserted exactly by owner_levels_ran); the case of many rows in ONE wave is Dfew's, whose 16 hubs
    are vertices 0 .. 15 and all in the level-2 frontier: one ballot, sixteen offsets, asserted there as 16 of 16."""
    base = owner_levels_ran("W", "batch", "default")
    got = owner_levels_ran("W", "batch", variant)
    assert FACTS[("W", "batch", variant, "BIGROWS")] > 640 and FACTS[("W", "batch", variant, "LISTED2")] > FACTS[("W", "batch", "default", "LISTED2")]
    owner_levels_ran("Dfew", "batch", "default")
    assert FACTS[("Dfew", "batch", "default", "LISTED2")] == 16
    assert got == base


@pytest.mark.parametrize("variant", ["default", "wait_first"])
@pytest.mark.parametrize("graph", ["W", "Wpath", "Dfew"])
def test_heavy_levels_with_and_without_pulled_sources(graph, variant):
    """(c) k = 2, 24, 33, 64 (Wpath: 2 and 24; Dfew: 2, 24 and 64), launched ahead and not: a heavy level with nothing pulled
    (the pull kernel's zeroing loop stashes) and one with sources pulled in the same level (the chunk stores stash; 33 and
    64 put stashed bits into the upper half of the word).  Two sweeps back to back each."""
    results, sweeps, _ = child(graph, "batch", variant)
    owner_levels_ran(graph, "batch", variant)
    heavy = [h for lines in sweeps.values() for h in heavy_levels(lines)]
    assert any(q == 0 for _, q in heavy) and any(q > 0 for _, q in heavy), heavy
    if graph == "Wpath":
        assert max(lv for lv, _ in heavy) > 17, heavy                 # past the stored level words
    assert results == child(graph, "batch", "default")[0]


@pytest.mark.parametrize("variant", ["tail_on", "tail_on_wait_first"])
def test_host_decided_heavy_level_after_a_hand_back(variant):
    """(d) Wpath with the light-level launch on and a limit of 2000 out-edges: the path's levels run inside it, it hands back
    when the hub's row arrives, and the heavy level that follows is decided by the host with nothing pulled -- the pull
    kernel in place of the fill."""
    results = owner_levels_ran("Wpath", "batch", variant)
    found = 0
    for lines in child("Wpath", "batch", variant)[1].values():
        summary = [x for x in lines if LIGHT_LINE.match(x) or LEVEL_LINE.match(x)]
        for prev, cur in zip(summary, summary[1:]):
            a, b = LIGHT_LINE.match(prev), LEVEL_LINE.match(cur)
            if a and b and a.group(3) == "2" and int(a.group(2)) > int(a.group(1)) and b.group(5) == "claims" and int(b.group(2)) == 0:
                found += 1
    assert found >= 2, found                                          # both sweeps of a size
    assert results == child("Wpath", "batch", "default")[0]


@pytest.mark.parametrize("graph", ["W", "Dfew"])
def test_claims_through_the_slice_kernel(graph):
    """(e) GRB_BATCH_OWNER=0: the heavy levels claim through batch_push_slices_kernel, with the stash and no list."""
    results, sweeps, _ = child(graph, "batch", "owner_off")
    for marker, lines in sweeps.items():
        assert not any("owner-computes" in x or "range owners" in x for x in lines), (marker, lines)
        assert heavy_levels(lines), (marker, lines)
    assert results == child(graph, "batch", "default")[0]


@pytest.mark.parametrize("graph", ["W", "Dfew"])
def test_queued_groups(graph):
    """(f) 24 and 48 traversals enqueued, each group one sweep on the sweep's own buffers, twice back to back."""
    base = owner_levels_ran(graph, "queue", "default")
    assert owner_levels_ran(graph, "queue", "merge_off") == base
