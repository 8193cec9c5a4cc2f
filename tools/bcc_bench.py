"""Biconnected components (csrc/bcc.hip: grb_bcc) on the bench shapes, with the library's own grb_cc and grb_msf on the same
matrix beside it (the cost of the components and of a spanning forest alone) and networkx on the host where it finishes:

  graphs     rmat16, rmat20 (edge factor 16, seed 1, symmetrised); grid (a 1000 x 1000 grid: one block, 1 999 levels); tree
             (a random tree of 1 M vertices: every edge a bridge); path (1 M vertices: the worst case, a level a vertex).
             rmatN, gridN, treeN and pathN take any size
  bcc        api.bcc in both modes with C and art, and with neither ("record"): ms per call (the median of --reps after a
             warm one), the device's levels, rounds and passes, the launches of the loop.  Every call must give the same
             exact fields, the same C and the same art: asserted
  cc, msf    api.cc (FastSV) and api.msf on the same structure with i32 ones: ms per call, the median of --reps
  networkx   nx.biconnected_component_edges / articulation_points on the host, one wall-clock run, for the graphs named in
             --nx (default rmat16,grid): blocks, bridges and articulation asserted equal.  "not measured" elsewhere

The device's figures are timed with HIP events on the library's stream (grb_timer_start / grb_timer_stop around the call).

  python tools/bcc_bench.py [--only rmat16,rmat20,grid,tree,path] [--nx rmat16,grid] [--reps 5]
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
EXACT = ("edges", "largest", "blocks", "bridges", "articulation", "components", "isolated", "levels", "launches")


def graph(name):
    """-> n, the edges (lo, hi), each undirected edge once"""
    from graphblast_amd.graphgen import rmat_edges
    rng = np.random.default_rng(7)
    if name.startswith("rmat"):
        s, d, n = rmat_edges(int(name[4:]), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    elif name.startswith("path"):
        n = int(name[4:] or 1000000)
        s = np.arange(n - 1, dtype=np.int64)
        d = s + 1
    elif name.startswith("tree"):
        n = int(name[4:] or 1000000)
        d = np.arange(1, n, dtype=np.int64)
        s = (rng.random(n - 1) * d).astype(np.int64)        # vertex k hangs on a random earlier one
        perm = rng.permutation(n)
        s, d = perm[s], perm[d]
    else:
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        d = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    keep = s != d
    lo, hi = np.minimum(s, d)[keep], np.maximum(s, d)[keep]
    key = np.unique(lo * n + hi)
    return n, key // n, key % n


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,grid,tree,path")
    ap.add_argument("--nx", default="rmat16,grid")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import scipy.sparse as sp
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("bcc_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    assert desc.loadArgs() == 0
    reps = max(1, a.reps)
    for name in a.only.split(","):
        n, lo, hi = graph(name)
        S = sp.csr_matrix((np.ones(2 * lo.size, I), (np.concatenate([lo, hi]), np.concatenate([hi, lo]))), shape=(n, n))
        S.sort_indices()
        A = g.Matrix(n, n, I)
        assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), S.data) == 0
        row = dict(graph=name, n=n, nnz=int(S.nnz))
        exact = None
        for what, mode, out in (("blocks", 0, True), ("bridges", 1, True), ("record", 0, False)):
            Cm, art = (g.Matrix(n, n, I), g.Vector(n, I)) if out else (None, None)

            def call():
                info, res = g.bcc(Cm, art, A, mode, None)
                assert info == 0, info
                return res

            _, first = timed_once(g, call)                # warm
            if exact is None:
                exact = [first[x] for x in EXACT]
            first_out = [x.tobytes() for x in Cm.host_csr()] + [art.extractTuples()[1].tobytes()] if out else None
            runs = [timed_once(g, call) for _ in range(reps)]
            assert all([r[1][x] for x in EXACT] == exact for r in runs), name
            if out:
                assert [x.tobytes() for x in Cm.host_csr()] + [art.extractTuples()[1].tobytes()] == first_out, name
            res = runs[-1][1]
            row[what + "_ms"] = float(np.median([r[0] for r in runs]))
            if what == "blocks":
                row.update({x: res[x] for x in EXACT})
                row.update(loop_ms=res["loop_ms"], rounds=res["rounds"], passes=res["passes"],
                           us_per_pass=1e3 * res["loop_ms"] / max(1, res["passes"]))
        print(json.dumps(row), flush=True)                # (the host may take long: the device's figures first)
        Cf = g.Matrix(n, n, I)
        for what, fn in (("cc", lambda v: g.cc(v, A, 0, desc)), ("msf", lambda v: g.msf(Cf, v, A, None))):
            v = g.Vector(n, I)

            def other():
                assert fn(v)[0] == 0
            timed_once(g, other)                          # warm
            row[what + "_ms"] = float(np.median([timed_once(g, other)[0] for _ in range(reps)]))
        row.update(bcc_over_cc=row["blocks_ms"] / row["cc_ms"], bcc_over_msf=row["blocks_ms"] / row["msf_ms"])
        if name in a.nx.split(","):
            import networkx as nx
            G = nx.Graph()
            G.add_nodes_from(range(n))
            G.add_edges_from(zip(lo.tolist(), hi.tolist()))
            t0 = time.perf_counter()
            sizes = [len(es) for es in nx.biconnected_component_edges(G)]
            cut = sum(1 for _ in nx.articulation_points(G))
            row["networkx_ms"] = 1e3 * (time.perf_counter() - t0)
            assert (len(sizes), sum(1 for x in sizes if x == 1), cut, max(sizes)) == \
                (row["blocks"], row["bridges"], row["articulation"], row["largest"]), (name, len(sizes), cut)
            row["networkx_over_bcc"] = row["networkx_ms"] / row["blocks_ms"]
        else:
            row["networkx_ms"] = "not measured"
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
