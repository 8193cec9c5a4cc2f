"""The strongly connected components (csrc/scc.hip: grb_scc) on the bench shapes, with the host's scipy and, where the
structure is symmetric, the library's own grb_cc beside it:

  graphs     rmat16, rmat20 (edge factor 16, seed 1, directed as drawn); rmat16s, rmat20s (the same symmetrised); grid (a
             1000 x 1000 grid, every edge one way by a coin, seed 3); cycle (one directed cycle of 1 M vertices).  rmatN,
             rmatNs, gridN and cycleN take any size
  scc        api.scc: ms per call (one timed call after a warm one; when that took under --rerun-under seconds, the median
             of --reps more), the device's passes, colouring rounds and trimmed vertices, components, the largest one.
             The labels of every call must be the same bytes: asserted
  scipy      scipy.sparse.csgraph.connected_components(connection="strong") on the host, one wall-clock run, as context:
             it gives the same partition (asserted) and is no competitor for the device
  cc         on the symmetrised shapes api.cc (FastSV: hooking and shortcutting), the comparator for the same partition
             (asserted): ms per call, the median of --reps

The device's figures are timed with HIP events on the library's stream (grb_timer_start / grb_timer_stop around the call).

  python tools/scc_bench.py [--only rmat16,rmat20,rmat16s,rmat20s,grid,cycle] [--reps 5] [--rerun-under 2]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F, I = np.float32, np.int32


def graph(name):
    """-> n, the pattern as a scipy CSR (duplicates merged, no diagonal, columns ascending), symmetric or not"""
    import scipy.sparse as sp
    from graphblast_amd.graphgen import rmat_edges
    sym = False
    if name.startswith("rmat"):
        sym = name.endswith("s")
        s, d, n = rmat_edges(int(name[4:].rstrip("s")), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    elif name.startswith("cycle"):
        n = int(name[5:] or 1000000)
        s = np.arange(n, dtype=np.int64)
        d = (s + 1) % n
    else:
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
        flip = np.random.default_rng(3).random(a.size) < 0.5
        s, d = np.where(flip, b, a), np.where(flip, a, b)
    keep = s != d
    s, d = s[keep], d[keep]
    if sym:
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
    S = sp.csr_matrix((np.ones(s.size, np.int8), (s, d)), shape=(n, n))
    S.data[:] = 1
    S.sort_indices()
    return n, S, sym


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def same_partition(a, b):
    _, ia = np.unique(a, return_inverse=True)
    _, ib = np.unique(b, return_inverse=True)
    pairs = np.unique(ia.astype(np.int64) * (int(ib.max()) + 1) + ib).size
    return pairs == ia.max() + 1 == ib.max() + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,rmat16s,rmat20s,grid,cycle")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rerun-under", type=float, default=2.0)
    a = ap.parse_args()
    from scipy.sparse.csgraph import connected_components
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("scc_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    assert desc.loadArgs() == 0
    for name in a.only.split(","):
        n, S, sym = graph(name)
        A = g.Matrix(n, n, I)
        assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, I)) == 0
        v = g.Vector(n, I)

        def call():
            info, res = g.scc(v, A, None)
            assert info == 0, info
            return res, v.extractTuples()[1].tobytes()

        _, (_, first) = timed_once(g, call)               # warm
        ms, (res, labels) = timed_once(g, call)
        assert labels == first, name
        warm = 1
        if ms < 1e3 * a.rerun_under and a.reps > 0:
            runs = [timed_once(g, call) for _ in range(a.reps)]
            assert all(r[1][1] == first for r in runs), name
            ms, res = float(np.median([r[0] for r in runs])), runs[-1][1][0]
            warm = a.reps
        row = dict(graph=name, n=n, nnz=int(S.nnz), scc_ms=ms, loop_ms=res["loop_ms"], runs=warm, passes=res["passes"], rounds=res["rounds"],
                   trimmed=res["trimmed"], components=res["components"], largest=res["largest"], trivial=res["trivial"],
                   launches=res["launches"], us_per_pass=1e3 * res["loop_ms"] / max(1, res["passes"]))
        print(json.dumps(row), flush=True)                # (the host may take long: the device's figures first)
        got = np.frombuffer(labels, I)
        t0 = time.perf_counter()
        k, lab = connected_components(S, directed=True, connection="strong")
        sms = 1e3 * (time.perf_counter() - t0)
        assert k == res["components"] and same_partition(lab, got), name
        low = np.full(k, n, np.int64)
        np.minimum.at(low, lab, np.arange(n))
        assert np.array_equal(low[lab], got), name        # ... and labelled by the smallest member
        row.update(scipy_ms=sms, scipy_over_scc=sms / ms)
        if sym:
            w = g.Vector(n, I)

            def cc_call():
                info, cres = g.cc(w, A, 0, desc)
                assert info == 0, info
                return cres

            timed_once(g, cc_call)                        # warm
            cms = float(np.median([timed_once(g, cc_call)[0] for _ in range(max(1, a.reps))]))
            assert same_partition(w.extractTuples()[1], got), name
            row.update(cc_ms=cms, scc_over_cc=ms / cms)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
