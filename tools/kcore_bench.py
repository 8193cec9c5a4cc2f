"""The k-core decomposition (csrc/kcore.hip: grb_coreness) beside the loop over the library's public operations that was the
only way to it before:

  graphs     RMAT-16 and RMAT-20 (edge factor 16, seed 1, symmetrised), graphgen.grid_edges(1000) (the thinned 1000 x 1000
             grid), a path of 1 M vertices; rmatN and pathN take any size
  coreness   api.coreness: ms per call (warm, the median of --reps), kmax, levels, the device's passes (rounds), launches
  loop       the synchronous peel op by op, in f32: the degrees by a row reduce; per round the frontier by a vector select
             (degree + 1 <= k + 1), its size read by the host, the removed neighbours of every vertex by mxv with the sparse
             frontier (values -1), the new degrees by eWiseAdd, the core numbers and the "gone" mark by two masked
             assigns; when a level is over the next one by a Minimum reduce.  One timed run; when that took under
             --rerun-under seconds, the median of --loop-reps more
  ratio      loop / coreness.  The two must give the same core numbers: asserted.

Every figure is timed with HIP events on the library's stream (grb_timer_start / grb_timer_stop around the call).

  python tools/kcore_bench.py [--only rmat16,rmat20,grid,path1000000] [--reps 5] [--loop-reps 2] [--rerun-under 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, I = np.float32, np.int32
GONE = 1e30


def graph(name):
    """-> n, CSR pointers and indices of the symmetrised graph"""
    from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges
    if name.startswith("rmat"):
        s, d, n = rmat_edges(int(name[4:]), 16, seed=1)
    elif name.startswith("path"):
        n = int(name[4:] or 1000000)
        s = np.arange(n - 1, dtype=np.int64)
        d = s + 1
    else:
        s, d, n = grid_edges(1000)
    gr = finalize_edges(np.asarray(s), np.asarray(d), n, symmetrize=True)
    ptr, ind = (np.asarray(x).astype(I) for x in gr["csr"])
    return n, ptr, ind


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def timed(g, call, reps):
    call()                                                # warm
    runs = [timed_once(g, call) for _ in range(reps)]
    return float(np.median([r[0] for r in runs])), runs[-1][1]


def peel_loop(g, A, n, desc):
    """the synchronous peel over the public operations; -> (core as an f32 vector, rounds)"""
    deg, d1, d2, core, front, gone, cnt = (g.Vector(n, F) for _ in range(7))
    assert g.reduce(None, "Plus", A, desc, w=deg) == 0    # A holds ones: the degrees
    if deg.nvals() != n:                                  # (rows without entries)
        assert deg.sparse2dense(0.0, desc) == 0
    assert g.eWiseAdd(d1, None, None, "PlusMultiplies", deg, 1.0, desc) == 0   # degree + 1: a mask must not meet a zero
    assert core.fill(0.0) == 0
    removed, rounds, k = 0, 0, 0
    while removed < n:
        assert g.select(front, None, None, "valuele", d1, float(k + 1), desc) == 0
        nf = front.nvals()                                # the host's read of the round
        if nf == 0:
            info, low = g.reduce(None, "Minimum", d1, desc)
            assert info == 0 and low < GONE, (info, low)
            k = int(low) - 1                              # the next level there is
            continue
        assert g.apply(gone, None, None, "bind_second", front, desc, binop="second", scalar=-1.0) == 0
        assert g.mxv(cnt, None, None, "PlusMultiplies", A, gone, desc) == 0    # minus the neighbours that went
        assert g.eWiseAdd(d2, None, None, "PlusMultiplies", d1, cnt, desc) == 0
        d1, d2 = d2, d1
        assert g.assign(core, gone, None, float(k), None, n, desc) == 0
        assert g.assign(d1, gone, None, GONE, None, n, desc) == 0
        removed += nf
        rounds += 1
    return core, rounds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,grid,path1000000")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-reps", type=int, default=2)
    ap.add_argument("--rerun-under", type=float, default=5.0)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("kcore_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    for name in a.only.split(","):
        n, ptr, ind = graph(name)
        A = g.Matrix(n, n, F)
        assert A.build_csr(ptr, ind, np.ones(ind.size, F)) == 0
        v = g.Vector(n, I)
        ms, (info, res) = timed(g, lambda: g.coreness(v, A, None), a.reps)
        assert info == 0, info
        want = v.extractTuples()[1]
        row = dict(graph=name, n=n, nnz=int(ind.size), coreness_ms=ms, loop_ms=res["loop_ms"], kmax=res["kmax"], levels=res["levels"],
                   rounds=res["rounds"], launches=res["launches"])
        print(json.dumps(row), flush=True)                # (the loop may take long: the device's figures first)
        lms, (core, rounds) = timed_once(g, lambda: peel_loop(g, A, n, desc))
        warm = 0
        if lms < 1e3 * a.rerun_under and a.loop_reps > 0:
            runs = [timed_once(g, lambda: peel_loop(g, A, n, desc)) for _ in range(a.loop_reps)]
            lms, (core, rounds) = float(np.median([r[0] for r in runs])), runs[-1][1]
            warm = 1
        got = core.extractTuples()[1]
        assert np.array_equal(got.astype(np.int64), want.astype(np.int64)), (name, np.flatnonzero(got != want)[:10])
        row.update(op_by_op_ms=lms, op_by_op_rounds=rounds, op_by_op_warm=warm, op_by_op_over_coreness=lms / ms)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
