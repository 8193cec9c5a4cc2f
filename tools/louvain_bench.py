"""Louvain community detection (csrc/louvain.hip: grb_louvain) on the bench shapes, with label propagation plus contraction
on the same library and networkx's Louvain on the host beside it:

  inputs     rmat16, rmat20 (edge factor 16, seed 1, symmetrised), unweighted and with symmetric i32 weights 1 .. 64
             (rmat16w, rmat20w); grid (1000 x 1000); path (1 M vertices: the expected worst case, chains of equal gains
             serialise on the smallest-v tie); stars (256 hubs of 4096 leaves each, the hubs on a ring).  rmatN, rmatNw,
             gridN, pathN take any size
  louvain    api.louvain: ms per call by the library's timer around the call (the median of --reps after a warm one), and
             levels, rounds, passes, Q and communities from the record.  The labels of every call are the same bits
  cdlp       grb_cdlp (ten iterations), grb_relabel and grb_contract (PLUS, loops kept) on the same matrix: ms for the three
             together, the communities, and Q of cdlp's labels by the same formula (computed on the host)
  networkx   louvain_communities(seed=1) on the host where it finishes in reasonable time (up to --nx-max entries, rmat16 at
             most by default), wall clock, with its Q by the same formula; skipped when networkx is missing

  python tools/louvain_bench.py [--only rmat16,rmat16w,rmat20,rmat20w,grid,path,stars] [--reps 3] [--no-nx] [--nx-only]
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
BIG = 1 << 30


def graph(name):
    """-> n, ptr, ind, val (i32, symmetric), weighted"""
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    weighted = 0
    if name.startswith("grid"):
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        d = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
    elif name.startswith("path"):
        n = int(name[4:] or 1 << 20)
        s = np.arange(n - 1, dtype=np.int64)
        d = s + 1
    elif name.startswith("stars"):
        hubs, leaves = 256, 4096
        n = hubs * (leaves + 1)
        h = np.arange(hubs, dtype=np.int64) * (leaves + 1)
        s = np.concatenate([np.repeat(h, leaves), h])
        d = np.concatenate([(h[:, None] + 1 + np.arange(leaves)[None, :]).ravel(), np.roll(h, -1)])
    else:
        weighted = 1 if name.endswith("w") else 0
        s, d, n = rmat_edges(int(name[4:].rstrip("w")), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    ptr, ind = finalize_edges(s, d, n, symmetrize=True, want_csc=False)["csr"]
    ptr, ind = np.asarray(ptr, I), np.asarray(ind, I)
    val = np.ones(ind.size, I)
    if weighted:
        rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
        lo, hi = np.minimum(rows, ind), np.maximum(rows, ind)
        val = (1 + ((lo * 2654435761 + hi * 40503) >> 7) % 64).astype(I)          # the same both ways
    return n, ptr, ind, val, weighted


def modularity(n, ptr, ind, val, labels):
    """Q = (W sum in(x) - sum tot(x)^2) / W^2 of any labelling, in exact integers"""
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(ptr))
    w = val.astype(np.int64)
    W = int(w.sum())
    if W == 0:
        return 0.0
    _, c = np.unique(labels, return_inverse=True)
    inner = int(w[c[rows] == c[ind]].sum())
    k = np.bincount(rows, weights=w, minlength=n)           # (f64 sums of integers below 2^31: exact)
    tot = np.bincount(c, weights=k).astype(np.int64)
    return (W * inner - sum(int(t) * int(t) for t in tot.tolist())) / (W * W)


def networkx_row(row, n, ptr, ind, val):
    """louvain_communities(seed=1) on the host, wall clock, and its Q by the same formula; nothing when networkx is missing"""
    try:
        import networkx as nx
    except ImportError:
        return
    rows = np.repeat(np.arange(n), np.diff(ptr))
    up = rows <= ind
    G = nx.Graph()
    G.add_nodes_from(range(n))
    G.add_weighted_edges_from(zip(rows[up].tolist(), ind[up].tolist(), val[up].tolist()))
    t0 = time.perf_counter()
    parts = nx.community.louvain_communities(G, weight="weight", seed=1)
    nx_ms = 1e3 * (time.perf_counter() - t0)
    nl = np.zeros(n, np.int64)
    for k, p in enumerate(parts):
        nl[list(p)] = k
    row.update(nx_ms=nx_ms, nx_communities=len(parts), nx_Q=modularity(n, ptr, ind, val, nl))


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat16w,rmat20,rmat20w,grid,path,stars")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-nx", action="store_true")
    ap.add_argument("--nx-max", type=int, default=2_000_000)
    ap.add_argument("--nx-only", action="store_true", help="only the networkx rows: needs no GPU")
    a = ap.parse_args()
    import graphblast_amd as g
    if not a.nx_only and not g.device_info().startswith("gfx"):
        raise SystemExit("louvain_bench needs the GPU: " + g.device_info())
    for name in a.only.split(","):
        n, ptr, ind, val, weighted = graph(name)
        if a.nx_only:
            row = dict(graph=name, n=n, nnz=int(ind.size), weighted=weighted)
            if ind.size <= a.nx_max:
                networkx_row(row, n, ptr, ind, val)
            print(json.dumps(row), flush=True)
            continue
        A = g.Matrix(n, n, I)
        assert A.build_csr(ptr, ind, val) == 0
        lab = g.Vector(n, I)

        def call():
            info, res = g.louvain(lab, A, weighted, BIG, BIG, None)
            assert info == 0, info
            return res

        timed_once(g, call)                                # warm
        first = lab.extractTuples()[1].tobytes()
        runs = [timed_once(g, call) for _ in range(max(1, a.reps))]
        labels = lab.extractTuples()[1]
        assert labels.tobytes() == first, name             # the same bits every call
        ms, res = float(np.median([r[0] for r in runs])), runs[-1][1]
        q_host = modularity(n, ptr, ind, val, labels)
        assert abs(q_host - res["modularity"]) < 1e-12, (name, q_host, res["modularity"])
        row = dict(graph=name, n=n, nnz=int(ind.size), weighted=weighted, louvain_ms=ms, loop_ms=res["loop_ms"], levels=res["levels"],
                   rounds=res["rounds"], passes=res["passes"], launches=res["launches"], moves=res["moves"], proposals=res["proposals"],
                   Q=res["modularity"], communities=res["communities"])
        print(json.dumps(row), flush=True)
        # ---- label propagation, then the community graph
        cl, mp = g.Vector(n, I), g.Vector(n, I)

        def route():
            assert g.cdlp(cl, A, None, max_iter=10)[0] == 0
            info, nc = g.relabel(mp, cl, g.GRB_RELABEL_LABELS)
            assert info == 0
            Cm = g.Matrix(nc, nc, I)
            assert g.contract(Cm, None, A, mp, "plus", 1, None)[0] == 0
            return nc

        timed_once(g, route)
        rr = [timed_once(g, route) for _ in range(max(1, a.reps))]
        row.update(cdlp_contract_ms=float(np.median([r[0] for r in rr])), cdlp_communities=int(rr[-1][1]),
                   cdlp_Q=modularity(n, ptr, ind, val, cl.extractTuples()[1]))
        # ---- networkx on the host
        if not a.no_nx and ind.size <= a.nx_max:
            networkx_row(row, n, ptr, ind, val)
        print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
