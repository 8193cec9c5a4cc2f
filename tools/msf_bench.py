"""The minimum spanning forest (csrc/msf.hip: grb_msf) on the bench shapes, with the host's scipy and the library's own
grb_cc and grb_scc on the same matrix beside it (the cost of the components alone):

  graphs     rmat16, rmat20 (edge factor 16, seed 1, symmetrised), each with random i32 weights in 1 .. 64 ("i") and with
             random f32 weights in (0, 1] ("f"); grid (a 1000 x 1000 grid) and path (1 M vertices), both with i32 weights
             in 1 .. 64.  rmatN, gridN and pathN take any size
  msf        api.msf with comp: ms per call (the median of --reps after a warm one), the device's rounds and passes, the
             forest's edges and weight.  Every call must give the same weight bits and the same C: asserted
  scipy      scipy.sparse.csgraph.minimum_spanning_tree on the host, one wall-clock run, as context.  Its total weight is
             asserted equal: exactly for i32 weights, within forest_edges x 2^-53 x sum |w| for f32 (its forest is the same
             one, its order of summation is not)
  cc, scc    api.cc (FastSV) and api.scc on the same matrix (for the f32 shapes an i32 matrix of ones with the same structure:
             cc takes no other): ms per call, the median of --reps; comp is asserted to be scc's vector

The device's figures are timed with HIP events on the library's stream (grb_timer_start / grb_timer_stop around the call).

  python tools/msf_bench.py [--only rmat16i,rmat16f,rmat20i,rmat20f,grid,path] [--reps 5]
"""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, I = np.float32, np.int32


def graph(name):
    """-> n, the upper triangle as a scipy CSR with the weights (each undirected edge once), the element type"""
    import scipy.sparse as sp
    from graphblast_amd.graphgen import rmat_edges
    rng = np.random.default_rng(7)
    dt = I
    if name.startswith("rmat"):
        dt = F if name.endswith("f") else I
        s, d, n = rmat_edges(int(name[4:].rstrip("if")), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    elif name.startswith("path"):
        n = int(name[4:] or 1000000)
        s = np.arange(n - 1, dtype=np.int64)
        d = s + 1
    else:
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        d = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    keep = s != d
    lo, hi = np.minimum(s, d)[keep], np.maximum(s, d)[keep]
    key = np.unique(lo * n + hi)
    lo, hi = key // n, key % n
    if dt is F:
        w = (1.0 - rng.random(lo.size)).astype(F)          # (0, 1]
        w[w == 0] = F(1)
    else:
        w = rng.integers(1, 65, lo.size).astype(I)
    return n, sp.csr_matrix((w, (lo, hi)), shape=(n, n)), dt


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16i,rmat16f,rmat20i,rmat20f,grid,path")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from scipy.sparse.csgraph import minimum_spanning_tree
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("msf_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    assert desc.loadArgs() == 0
    for name in a.only.split(","):
        n, U, dt = graph(name)
        S = (U + U.T).tocsr()
        S.sort_indices()
        A = g.Matrix(n, n, dt)
        assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), S.data.astype(dt)) == 0
        Cm, comp = g.Matrix(n, n, dt), g.Vector(n, I)

        def call():
            info, res = g.msf(Cm, comp, A, None)
            assert info == 0, info
            return res

        _, first = timed_once(g, call)                    # warm
        first_c = [x.tobytes() for x in Cm.host_csr()]
        runs = [timed_once(g, call) for _ in range(max(1, a.reps))]
        assert all(np.float64(r[1]["weight"]).tobytes() == np.float64(first["weight"]).tobytes() for r in runs), name
        assert [x.tobytes() for x in Cm.host_csr()] == first_c, name
        ms, res = float(np.median([r[0] for r in runs])), runs[-1][1]
        row = dict(graph=name, n=n, nnz=int(S.nnz), msf_ms=ms, loop_ms=res["loop_ms"], rounds=res["rounds"], passes=res["passes"],
                   forest_edges=res["forest_edges"], weight=res["weight"], components=res["components"], isolated=res["isolated"],
                   launches=res["launches"], us_per_pass=1e3 * res["loop_ms"] / max(1, res["passes"]))
        print(json.dumps(row), flush=True)                # (the host may take long: the device's figures first)
        labels = comp.extractTuples()[1]
        B = A                                             # cc takes an i32 matrix: the same structure, ones
        if dt is F:
            B = g.Matrix(n, n, I)
            assert B.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, I)) == 0
        for what, fn in (("cc", lambda v: g.cc(v, B, 0, desc)), ("scc", lambda v: g.scc(v, B, None))):
            v = g.Vector(n, I)

            def other():
                assert fn(v)[0] == 0
            timed_once(g, other)                          # warm
            row[what + "_ms"] = float(np.median([timed_once(g, other)[0] for _ in range(max(1, a.reps))]))
            if what == "scc":
                assert np.array_equal(v.extractTuples()[1], labels), name
        t0 = time.perf_counter()
        T = minimum_spanning_tree(U)
        row["scipy_ms"] = 1e3 * (time.perf_counter() - t0)
        assert T.nnz == res["forest_edges"], (name, T.nnz, res["forest_edges"])
        if dt is I:
            assert int(T.data.astype(np.int64).sum()) == int(res["weight"]), name
        else:
            want = math.fsum(T.data.astype(np.float64).tolist())
            assert abs(want - res["weight"]) <= T.nnz * 2.0 ** -53 * want, (name, want, res["weight"])
        row.update(scipy_over_msf=row["scipy_ms"] / ms, msf_over_cc=ms / row["cc_ms"], msf_over_scc=ms / row["scc_ms"])
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
