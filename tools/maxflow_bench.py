"""Maximum flow (csrc/maxflow.hip: grb_maxflow) on the bench shapes, with scipy.sparse.csgraph.maximum_flow on the host beside
it:

  networks   rmat16, rmat20 (edge factor 16, seed 1, as drawn: directed) with random i32 capacities in 1 .. 64; rmat16s (the
             same structure symmetrised, an independent capacity per direction); grid (a 1000 x 1000 grid, every edge in both
             directions, capacities in 1 .. 64, corner to corner); bip (a random bipartite graph, 100 000 + 100 000 vertices
             of degree 8, unit capacities through a super source and a super sink: the maximum bipartite matching).  rmatN,
             rmatNs, gridN and bipN take any size
  terminals  rmat: the vertex of largest out-degree and a vertex at the largest BFS depth from it; grid and bip as said
  maxflow    api.maxflow with F and side, and with side alone: ms per call (the median of --reps after a warm one), the
             device's rounds, passes and global relabelings, the value and the cut.  Every call must give the same record,
             the same side and the same F: asserted
  host       scipy's maximum_flow on the same network, one wall-clock run; its flow_value is asserted equal to the device's.
             Skipped above --host-arcs arcs

The device's figures are timed with HIP events on the library's stream (grb_timer_start / grb_timer_stop around the call).

  python tools/maxflow_bench.py [--only rmat16,rmat20,rmat16s,grid,bip] [--reps 5] [--host-arcs 40000000]
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

I = np.int32
CAPACITY, UNIT = 0, 1
EXACT = ("value", "arcs", "flow_arcs", "sink_side", "cut_arcs", "cut_capacity", "launches")


def network(name):
    """-> n, i, j, c (every arc once, i != j, sorted by (i, j)), source, sink, the mode"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import breadth_first_order
    from graphblast_amd.graphgen import rmat_edges
    rng = np.random.default_rng(9)
    mode = CAPACITY
    if name.startswith("rmat"):
        sym = name.endswith("s")
        s, d, n = rmat_edges(int(name[4:].rstrip("s")), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
        if sym:
            s, d = np.concatenate([s, d]), np.concatenate([d, s])
        key = np.unique(s[s != d] * n + d[s != d])
        i, j = key // n, key % n
        c = rng.integers(1, 65, i.size).astype(I)
        source = int(np.argmax(np.bincount(i, minlength=n)))
        S = sp.csr_matrix((np.ones(i.size, np.int8), (i, j)), shape=(n, n))
        order, pred = breadth_first_order(S, source, directed=True, return_predecessors=True)
        sink = int(order[-1])                              # (BFS order: the last vertex is at the largest depth)
    elif name.startswith("grid"):
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        a = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        b = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
        key = np.sort(np.concatenate([a * n + b, b * n + a]))
        i, j = key // n, key % n
        c = rng.integers(1, 65, i.size).astype(I)
        source, sink = 0, n - 1
    else:
        k = int(name[3:] or 100000)
        n = 2 * k + 2
        left = np.repeat(np.arange(k, dtype=np.int64), 8)
        right = k + rng.integers(0, k, left.size)
        source, sink = 2 * k, 2 * k + 1
        a = np.concatenate([np.full(k, source, np.int64), left, k + np.arange(k, dtype=np.int64)])
        b = np.concatenate([np.arange(k, dtype=np.int64), right, np.full(k, sink, np.int64)])
        key = np.unique(a * n + b)
        i, j = key // n, key % n
        c = np.ones(i.size, I)
        mode = UNIT
    assert source != sink
    return n, i, j, c, source, sink, mode


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,rmat16s,grid,bip")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-arcs", type=int, default=40000000)
    a = ap.parse_args()
    import scipy.sparse as sp
    from scipy.sparse.csgraph import maximum_flow
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("maxflow_bench needs the GPU: " + g.device_info())
    for name in a.only.split(","):
        n, i, j, c, source, sink, mode = network(name)
        S = sp.csr_matrix((c, (i, j)), shape=(n, n))
        S.sort_indices()
        A = g.Matrix(n, n, I)
        assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), S.data.astype(I)) == 0
        row = dict(network=name, n=n, arcs=int(i.size), source=source, sink=sink, mode=mode)
        first = None
        for what in ("flow", "cut"):
            Fm = g.Matrix(n, n, I) if what == "flow" else None
            side = g.Vector(n, I)

            def call():
                info, res = g.maxflow(Fm, side, A, source, sink, mode, None)
                assert info == 0, info
                return res

            _, warm = timed_once(g, call)
            state = [side.extractTuples()[1].tobytes()] + ([x.tobytes() for x in Fm.host_csr()] if Fm is not None else [])
            runs = [timed_once(g, call) for _ in range(max(1, a.reps))]
            assert all(r[1][x] == warm[x] for r in runs for x in EXACT), name
            assert state == [side.extractTuples()[1].tobytes()] + ([x.tobytes() for x in Fm.host_csr()] if Fm is not None else []), name
            ms, res = float(np.median([r[0] for r in runs])), runs[-1][1]
            assert res["cut_capacity"] == res["value"] and res["launches"] == 1 and res["arcs"] == i.size, (name, res)
            if first is None:
                first = res
            assert all(res[x] == first[x] for x in EXACT if x != "flow_arcs"), (name, res, first)
            row.update({what + "_ms": ms, what + "_loop_ms": res["loop_ms"], what + "_rounds": res["rounds"], what + "_passes": res["passes"],
                        what + "_global_relabels": res["global_relabels"], what + "_us_per_pass": 1e3 * res["loop_ms"] / max(1, res["passes"])})
        row.update(value=first["value"], flow_arcs=first["flow_arcs"], sink_side=first["sink_side"], cut_arcs=first["cut_arcs"])
        print(json.dumps(row), flush=True)                # (the host may take long: the device's figures first)
        if i.size <= a.host_arcs:
            t0 = time.perf_counter()
            want = int(maximum_flow(S.astype(I), source, sink).flow_value)
            row["host_ms"] = 1e3 * (time.perf_counter() - t0)
            assert want == first["value"], (name, want, first["value"])
            row.update(host_over_flow=row["host_ms"] / row["flow_ms"], host_over_cut=row["host_ms"] / row["cut_ms"], equal_to_host=True)
            print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
