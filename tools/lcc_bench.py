"""The local clustering coefficient (csrc/lcc.hip: grb_lcc) beside the composition that was the only way to it before, and
beside the triangle count:

  graphs       RMAT-16 and RMAT-20 (edge factor 16, seed 1, symmetrised), RMAT-16 as drawn (directed = 1: rows and columns), a
               1000 x 1000 grid
  lcc          api.lcc: ms per call, the list entries of the working graph (2 edges), triangles, loop_ms
  composed     the symmetric graphs only: ktruss(k = 2) for the per-edge supports, reduce_matrix_rows under Plus for num,
               the degrees as the row sums of the ones, then d - 1, d (d - 1) and the quotient as vector operations, in f32
               (so its values agree with lcc's only to f32 rounding of the sums; the largest difference is printed)
  tc           grb_tc's warm count on the lower triangle (the orientation is prepared by the warm call and kept)
  ratios       composed / lcc and lcc / tc

Each figure is the median of --reps calls after one warm call, timed with HIP events on the library's stream
(grb_timer_start / grb_timer_stop around the call).

  python tools/lcc_bench.py [--only rmat16,rmat20,rmat16d,grid] [--reps 5]
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


def composed(g, A, n, desc):
    """lcc through ktruss(k = 2) and a row reduction; -> the f32 vector"""
    T = g.Matrix(n, n, F)
    info, _ = g.ktruss(T, A, 2, desc)
    assert info == 0, info
    num, d, dm1, q, out = (g.Vector(n, F) for _ in range(5))
    assert g.reduce(None, "Plus", T, desc, w=num) == 0
    assert g.reduce(None, "Plus", A, desc, w=d) == 0      # A holds ones: the degrees
    assert g.apply(dm1, None, None, "bind_second", d, desc, binop="minus", scalar=1.0) == 0
    assert g.eWiseMult(q, None, None, "PlusMultiplies", d, dm1, desc) == 0
    assert g.eWiseMult(out, None, None, "PlusDivides", num, q, desc) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,rmat16d,grid")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("lcc_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    for name in a.only.split(","):
        n, ptr, ind, directed = graph(name)
        A = g.Matrix(n, n, F)                             # (finalize_edges drops the loops: tc takes none)
        assert A.build_csr(ptr, ind, np.ones(ind.size, F)) == 0
        v = g.Vector(n, F)
        ms, (info, res) = timed(g, lambda: g.lcc(v, A, None, directed), a.reps)
        assert info == 0, info
        row = dict(graph=name, n=n, nnz=int(ind.size), directed=int(directed), lcc_ms=ms, loop_ms=res["loop_ms"],
                   list_entries=2 * res["edges"], triangles=res["triangles"], closed=res["closed"], wedges=res["wedges"],
                   max_degree=res["max_degree"])
        if not directed:
            cms, out = timed(g, lambda: composed(g, A, n, desc), a.reps)
            got, want = out.extractTuples()[1], v.extractTuples()[1]
            some = np.diff(ptr) >= 2
            row.update(composed_ms=cms, composed_over_lcc=cms / ms,
                       composed_max_diff=float(np.abs(got[some] - want[some]).max()) if some.any() else 0.0)
            Ai, L, B = g.Matrix(n, n, I), g.Matrix(n, n, I), g.Matrix(n, n, I)   # (i32: an f32 count above 2^24 is rounded)
            assert Ai.build_csr(ptr, ind, np.ones(ind.size, I)) == 0
            assert g.tril(L, Ai, desc) == 0
            tms, (info, ntris, _) = timed(g, lambda: g.tc(L, B, desc), a.reps)
            assert info == 0 and ntris == res["triangles"], (info, ntris, res["triangles"])
            row.update(tc_ms=tms, lcc_over_tc=ms / tms)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
