"""GPU suite (-m gpu): queued traversals share launches by default (grb_bfs_fused_enqueue with no
grb_bfs_set_coschedule call).  Other test files fix the width with grb_bfs_set_coschedule and leave it set, and nothing
restores the default, so the checks under the default run in a fresh child process each; labels are compared with the
oracle and with the blocking call, result blocks with the blocking call."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r'''
import os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import graphblast_amd as g
from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
from oracle import simple_reference as sr

mode = sys.argv[1]
assert g.bfs_set_coschedule(-1) == 1                    # (what a query answers while the library picks the width)
s, d, n = rmat_edges(15, 16, seed=3)
gr = finalize_edges(s, d, n, symmetrize=True)
ptr, ind = gr["csr"]
A = g.Matrix(n, n)
assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
desc = g.Descriptor()
assert desc.loadArgs(mxvmode=0, struconly=1, opreuse=1, edgeswitch=0.05) == 0
KEYS = ("levels", "reached", "edges_traversed")
blocking = {}


def blocking_call(src):
    if src not in blocking:
        vb = g.Vector(n)
        info, res = g.bfs(vb, A, src, desc, fused=True)
        assert info == 0, info
        blocking[src] = (vb.extractTuples()[1], res)
    return blocking[src]


def queue(vecs, srcs):
    tickets = []
    for v, s_ in zip(vecs, srcs):
        info, t = g.bfs_enqueue(v, A, s_, desc)
        assert info == 0 and t != 0, info
        tickets.append(t)
    out = []
    for t in tickets:
        info, res = g.bfs_wait(t)
        assert info == 0, info
        out.append(res)
    return out


if mode == "twenty":
    srcs = [int(np.argmax(np.diff(ptr)))] + random_sources(ptr, 19, seed=11)
    vs = [g.Vector(n) for _ in srcs]
    g.bfs_coschedule_profile(True)
    res = queue(vs, srcs)
    prof = g.bfs_coschedule_profile(False)
    assert (prof["launches"], prof["traversals"]) == (1, 20), prof
    for v, r, s_ in zip(vs, res, srcs):
        want = sr.bfs(ptr, ind, s_)[0]
        assert np.array_equal(v.extractTuples()[1], want), s_
        assert r["reached"] == int(np.count_nonzero(want)), s_
        assert all(r[k] == blocking_call(s_)[1][k] for k in KEYS), s_
elif mode == "same_vector":
    s0, s1, s2, s3 = random_sources(ptr, 4, seed=5)
    v, w = g.Vector(n), g.Vector(n)
    res = queue([v, v, w, v], [s0, s1, s2, s3])
    assert np.array_equal(v.extractTuples()[1], blocking_call(s3)[0])
    assert np.array_equal(w.extractTuples()[1], blocking_call(s2)[0])
    for r, s_ in zip(res, (s0, s1, s2, s3)):
        assert all(r[k] == blocking_call(s_)[1][k] for k in KEYS), s_
elif mode == "counts":
    srcs_all = random_sources(ptr, 49, seed=7)
    for count in (1, 2, 12, 13, 48, 49):
        srcs = srcs_all[:count]
        vs = [g.Vector(n) for _ in srcs]
        g.bfs_coschedule_profile(True)
        res = queue(vs, srcs)
        prof = g.bfs_coschedule_profile(False)
        # a lone traversal goes to the one-traversal kernel; 48 fill a launch, the 49th goes alone
        assert (prof["launches"], prof["traversals"]) == ((0, 0) if count == 1 else (1, min(count, 48))), (count, prof)
        for v, r, s_ in zip(vs, res, srcs):
            assert np.array_equal(v.extractTuples()[1], blocking_call(s_)[0]), (count, s_)
            assert all(r[k] == blocking_call(s_)[1][k] for k in KEYS), (count, s_)
print("OK")
'''


def run_child(mode):
    out = subprocess.run([sys.executable, "-c", CHILD, mode], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0 and "OK" in out.stdout, out.stdout[-1000:] + out.stderr[-2500:]
    assert "not published" not in out.stderr and "host-driven" not in out.stderr, out.stderr[-1500:]


def test_twenty_queued_traversals_share_one_launch_by_default():
    """20 traversals queued with no setting made: one launch carries all 20, labels equal the oracle's, result blocks
    the blocking call's."""
    run_child("twenty")


def test_a_vector_queued_into_twice_holds_the_last_traversal():
    """v <- s0, v <- s1, w <- s2, v <- s3 under the default: the traversals of one launch run concurrently, so a second
    one into the same vector starts the next launch; v ends as the blocking call from s3 leaves it, w as the one from s2,
    and every result block is the blocking call's for its source."""
    run_child("same_vector")


def test_counts_around_the_launch_boundaries():
    """1, 2, 12, 13, 48 and 49 traversals queued under the default: one launch per 48 gathered (a lone one takes the
    one-traversal kernel), and labels and result blocks equal the blocking call's."""
    run_child("counts")


def test_coschedule_one_gives_one_launch_per_traversal():
    """grb_bfs_set_coschedule(1): no launch of several traversals, the same results; the previous setting is restored."""
    import graphblast_amd as g
    from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
    s, d, n = rmat_edges(14, 16, seed=4)
    ptr, ind = finalize_edges(s, d, n, symmetrize=True)["csr"]
    A = g.Matrix(n, n)
    assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
    desc = g.Descriptor()
    assert desc.loadArgs(mxvmode=0, struconly=1, opreuse=1) == 0
    srcs = random_sources(ptr, 13, seed=2)
    before = g.bfs_set_coschedule(1)
    try:
        vs = [g.Vector(n) for _ in srcs]
        g.bfs_coschedule_profile(True)
        tickets = [g.bfs_enqueue(v, A, s_, desc) for v, s_ in zip(vs, srcs)]
        assert all(i == 0 for i, _ in tickets)
        res = [g.bfs_wait(t) for _, t in tickets]
        prof = g.bfs_coschedule_profile(False)
        assert all(i == 0 for i, _ in res)
        assert (prof["launches"], prof["traversals"]) == (0, 0), prof
        for v, (_, r), s_ in zip(vs, res, srcs):
            vb = g.Vector(n)
            info, rb = g.bfs(vb, A, s_, desc, fused=True)
            assert info == 0
            assert np.array_equal(v.extractTuples()[1], vb.extractTuples()[1]), s_
            assert all(r[k] == rb[k] for k in ("levels", "reached", "edges_traversed")), s_
    finally:
        g.bfs_set_coschedule(before)
