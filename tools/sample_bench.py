"""Random walks and neighbour sampling (csrc/sample.hip: grb_random_walk, grb_sample_neighbors) on the bench shapes:

  inputs     rmat16, rmat20 (edge factor 16, seed 1, symmetrised) and grid (1000 x 1000), i32 values: symmetric weights
             1 .. 64.  rmatN and gridN take any size
  walks      every vertex a walker (a NULL list) at length 8 and 80, uniform and weighted: ms per call by the library's timer
             around the call (the median of --reps after a warm one), the record's loop_ms, and steps per second.  Beside it,
             for scale only, one grb_bfs_batch of 64 sources on the same matrix
  sampling   1 024, 65 536 and n seeds (drawn with replacement; n: every row in order) at fanout 5, 10 and 25: ms per call,
             and grb_matrix_extract of the same rows beside it -- the natural yardstick: sampling writes fewer bytes and reads
             no values it drops.  The ratio is reported, not asserted
Every call's output is checked to be the same bits as the warm call's.

  python tools/sample_bench.py [--only rmat16,rmat20,grid] [--reps 5] [--no-walks] [--no-sample]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I = np.int32


def graph(name):
    """-> n, ptr, ind, val (i32, symmetric weights 1 .. 64)"""
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    if name.startswith("grid"):
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        d = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    else:
        s, d, n = rmat_edges(int(name[4:]), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    ptr, ind = finalize_edges(s, d, n, symmetrize=True, want_csc=False)["csr"]
    ptr, ind = np.asarray(ptr, I), np.asarray(ind, I)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    lo, hi = np.minimum(rows, ind), np.maximum(rows, ind)
    val = (1 + ((lo * 2654435761 + hi * 40503) >> 7) % 64).astype(I)              # the same both ways
    return n, ptr, ind, val


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def median_of(g, call, reps):
    timed_once(g, call)                                    # warm
    runs = [timed_once(g, call) for _ in range(max(1, reps))]
    return float(np.median([r[0] for r in runs])), runs[-1][1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,grid")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-walks", action="store_true")
    ap.add_argument("--no-sample", action="store_true")
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("sample_bench needs the GPU: " + g.device_info())
    for name in a.only.split(","):
        n, ptr, ind, val = graph(name)
        A = g.Matrix(n, n, I)
        assert A.build_csr(ptr, ind, val) == 0
        base = dict(graph=name, n=n, nnz=int(ind.size))
        if not a.no_walks:
            for length in (8, 80):
                for mode, tag in ((g.GRB_WALK_UNIFORM, "uniform"), (g.GRB_WALK_WEIGHTED, "weighted")):
                    walks = g.Vector(n * (length + 1), I)

                    def call():
                        info, res = g.random_walk(walks, A, None, length, mode, 1, None)
                        assert info == 0, info
                        return res

                    timed_once(g, call)
                    first = walks.extractTuples()[1].tobytes()
                    ms, res = median_of(g, call, a.reps)
                    assert walks.extractTuples()[1].tobytes() == first, (name, length, tag)       # the same bits every call
                    print(json.dumps(dict(base, op="walk", mode=tag, length=length, ms=ms, loop_ms=res["loop_ms"], steps=res["steps"],
                                          dead_ends=res["dead_ends"], steps_per_s=res["steps"] / (ms * 1e-3))), flush=True)
                    del walks
            # for scale only: one batched BFS of 64 sources
            src = np.argsort(-np.diff(ptr), kind="stable")[:64].astype(I)
            vs = [g.Vector(n) for _ in src]
            desc = g.Descriptor()
            assert desc.loadArgs(mxvmode=0, struconly=1, opreuse=1) == 0
            ms, res = median_of(g, lambda: g.bfs_batch(vs, A, src, desc), a.reps)
            assert res[0] == 0
            print(json.dumps(dict(base, op="bfs_batch", sources=64, ms=ms, levels=res[1]["levels"])), flush=True)
            del vs
        if not a.no_sample:
            rng = np.random.default_rng(1)
            for ns in (1024, 65536, n):
                seeds = np.arange(n, dtype=I) if ns == n else rng.integers(0, n, ns).astype(I)
                X = g.Matrix(ns, n, I)
                ems, info = median_of(g, lambda: g.extract(X, None, None, A, seeds, None, None), a.reps)
                assert info == 0, info
                xn = X.nvals()
                del X
                for fanout in (5, 10, 25):
                    Cm = g.Matrix(ns, n, I)

                    def call():
                        info, res = g.sample_neighbors(Cm, A, seeds, fanout, 1, None)
                        assert info == 0, info
                        return res

                    timed_once(g, call)
                    first = [x.tobytes() for x in Cm.host_csr()]
                    ms, res = median_of(g, call, a.reps)
                    assert [x.tobytes() for x in Cm.host_csr()] == first, (name, ns, fanout)
                    print(json.dumps(dict(base, op="sample", seeds=ns, fanout=fanout, ms=ms, loop_ms=res["loop_ms"], entries=res["entries"],
                                          full_rows=res["full_rows"], extract_ms=ems, extract_entries=xn, sample_over_extract=ms / ems)),
                          flush=True)
                    del Cm
    return 0


if __name__ == "__main__":
    sys.exit(main())
