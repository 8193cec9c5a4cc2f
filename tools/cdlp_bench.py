"""Community detection by label propagation (csrc/cdlp.hip: grb_cdlp) with and without the skipping of vertices none of
whose neighbours changed:

  graphs     RMAT-16 and RMAT-20 (edge factor 16, seed 1, symmetrised), RMAT-16 as drawn (directed = 1: rows and columns), a
             1000 x 1000 grid
  cdlp       api.cdlp from L(v) = v with at most --max-iter iterations: ms per call, iterations, ms per iteration, evaluated
             (the (vertex, iteration) pairs whose mode was computed), communities
  skip off   the same after api.cdlp_set_skip(0): every vertex with neighbours, every iteration; the labels must be the same
  floor      what one fully evaluated iteration cannot beat: list entries x 8 bytes (4 of index, 4 of gathered label) at
             8 TB/s; list entries = nnz, rows and columns together in the directed case

Each figure is the median of --reps calls after one warm call, timed with HIP events on the library's stream
(grb_timer_start / grb_timer_stop around the call).

  python tools/cdlp_bench.py [--only rmat16,rmat20,rmat16d,grid] [--reps 5] [--max-iter 10]
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


def graph(name):
    """-> n, CSR pointers and indices, directed"""
    from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges
    directed = name.endswith("d") and name.startswith("rmat")
    if name.startswith("rmat"):
        s, d, n = rmat_edges(int(name[4:].rstrip("d")), 16, seed=1)
    else:
        s, d, n = grid_edges(1000, keep=1.0)
    gr = finalize_edges(np.asarray(s), np.asarray(d), n, symmetrize=not directed)
    ptr, ind = (np.asarray(x).astype(I) for x in gr["csr"])
    return n, ptr, ind, directed


def timed(g, call, reps):
    lib = g._lib.load()
    out = call()                                          # warm
    ms = []
    for _ in range(reps):
        t = ctypes.c_float(0)
        assert lib.grb_timer_start() == 0
        out = call()
        assert lib.grb_timer_stop(ctypes.byref(t)) == 0
        ms.append(t.value)
    return float(np.median(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,rmat16d,grid")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-iter", type=int, default=10)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("cdlp_bench needs the GPU: " + g.device_info())
    good = True
    for name in a.only.split(","):
        n, ptr, ind, directed = graph(name)
        A = g.Matrix(n, n, F)
        assert A.build_csr(ptr, ind, np.ones(ind.size, F)) == 0
        entries = int(ind.size) * (2 if directed else 1)
        floor_ms = entries * 8 / 8e12 * 1e3
        v = g.Vector(n, I)
        labels = {}
        was = g.cdlp_set_skip(1)
        try:
            for skip in (1, 0):
                g.cdlp_set_skip(skip)
                ms, (info, res) = timed(g, lambda: g.cdlp(v, A, None, None, directed, a.max_iter), a.reps)
                assert info == 0, info
                labels[skip] = v.extractTuples()[1].copy()
                print(json.dumps(dict(graph=name, n=n, nnz=int(ind.size), directed=int(directed), skip=skip, ms=ms,
                                      loop_ms=res["loop_ms"], iterations=res["iterations"], ms_per_iteration=ms / res["iterations"],
                                      changed=res["changed"], evaluated=res["evaluated"], communities=res["communities"],
                                      floor_ms_per_full_iteration=floor_ms)), flush=True)
        finally:
            g.cdlp_set_skip(was)
        same = bool(np.array_equal(labels[0], labels[1]))
        good = good and same
        print(json.dumps(dict(graph=name, same_labels_with_and_without_skip=same)), flush=True)
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
