"""Betweenness centrality (csrc/bc.hip: grb_bc, batched Brandes) against the traversal it follows and against the loop a
caller writes with the library's operations:

  graphs     RMAT-14 and RMAT-16 (edge factor 16, seed 1, symmetrised) with 64 sources, a 1000 x 1000 grid with 8 sources
             (sources of nonzero out-degree, graphgen.random_sources)
  bc         api.bc on all the sources: ms per call = per batch (at most 64 sources: one batch), ms per source
  bfs_batch  api.bfs_batch alone on the same sources: the depths bc starts from, as bits; bc / bfs_batch says how far the
             two passes over 8-byte path counts are from the traversal they follow
  op-by-op   single-source Brandes over vxm / mxv / eWiseAdd / eWiseMult / reduce in f32, one source after the other (the
             only way to centrality before grb_bc): per level forwards a masked vxm, a reduce and an eWiseAdd, per level
             backwards two element-wise calls, an mxv and two more, one of them under the level's mask; timed on the
             first --loop-sources sources (the grid: 1), ms per source, and compared with api.bc on those sources

Each figure is the median of --reps calls after one warm call, timed with HIP events on the library's stream
(grb_timer_start / grb_timer_stop around the call).

  python tools/bc_bench.py [--only rmat14,rmat16,grid] [--reps 5] [--loop-sources 8]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F = np.float32


def graph(name):
    from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges, random_sources
    if name.startswith("rmat"):
        s, d, n = rmat_edges(int(name[4:]), 16, seed=1)
        ns = 64
    else:
        s, d, n = grid_edges(1000, keep=1.0)
        ns = 8
    gr = finalize_edges(np.asarray(s), np.asarray(d), n, symmetrize=True)
    ptr, ind = (np.asarray(x).astype(np.int32) for x in gr["csr"])
    return n, ptr, ind, np.asarray(random_sources(ptr, ns, seed=0)).astype(np.int32)


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


def ok(info):
    if info != 0:
        raise SystemExit("a library call of the op-by-op loop returned %d" % info)


def op_by_op(g, A, n, sources, d, d_scmp):
    """-> the centrality of `sources` as a dense f32 vector's values: Brandes, one source after the other"""
    bc = g.Vector(n, F)
    ok(bc.fill(0.0))
    for s in sources:
        sigma = g.Vector(n, F)
        ok(sigma.fill(0.0))
        ok(sigma.setElement(1.0, int(s)))
        q = g.Vector(n, F)
        ok(q.build(np.array([s], np.int32), np.array([1.0], F), 1, None))
        fronts = []
        while True:                                       # forwards: fronts[k] = the path counts of the vertices at depth k
            keep = g.Vector(n, F)
            ok(keep.dup(q))
            fronts.append(keep)
            nq = g.Vector(n, F)
            ok(g.vxm(nq, sigma, None, "PlusMultiplies", q, A, d_scmp))     # where sigma is still 0
            q = nq
            info, succ = g.reduce(None, "Plus", q, d)
            ok(info)
            if succ == 0:
                break
            ok(g.eWiseAdd(sigma, None, None, "PlusMultiplies", sigma, q, d))
        delta = g.Vector(n, F)
        ok(delta.fill(0.0))
        for k in range(len(fronts) - 1, 1, -1):           # backwards: the dependencies of depth k - 1 from depth k
            t1, t2, w, w2 = (g.Vector(n, F) for _ in range(4))
            ok(g.eWiseAdd(t1, None, None, "PlusMultiplies", delta, 1.0, d))             # 1 + delta
            ok(g.eWiseMult(t2, None, None, "PlusDivides", t1, fronts[k], d))            # ... / sigma, at depth k only
            ok(g.mxv(w, None, None, "PlusMultiplies", A, t2, d))                        # summed over the children
            ok(g.eWiseMult(w2, fronts[k - 1], None, "PlusMultiplies", w, sigma, d))     # ... times sigma, at depth k - 1 only
            ok(g.eWiseAdd(delta, None, None, "PlusMultiplies", delta, w2, d))
        ok(g.eWiseAdd(bc, None, None, "PlusMultiplies", bc, delta, d))
    info, vals = bc.extractTuples()
    ok(info)
    return vals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat14,rmat16,grid")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--loop-sources", type=int, default=8)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("bc_bench needs the GPU: " + g.device_info())
    d, d_scmp = g.Descriptor(), g.Descriptor()
    assert d.loadArgs() == 0 and d_scmp.loadArgs() == 0 and d_scmp.toggle(g.GrB_MASK) == 0
    good = True
    for name in a.only.split(","):
        n, ptr, ind, src = graph(name)
        A = g.Matrix(n, n, F)
        assert A.build_csr(ptr, ind, np.ones(ind.size, F)) == 0
        ns = int(src.size)
        v = g.Vector(n, F)
        ms, (info, res) = timed(g, lambda: g.bc(v, A, src, None), a.reps)
        assert info == 0
        vs = [g.Vector(n, F) for _ in range(ns)]
        ms_bfs, (info, rec) = timed(g, lambda: g.bfs_batch(vs, A, src, d), a.reps)
        assert info == 0 and rec["reached"] == res["reached"], (rec, res)
        base = {"graph": name, "n": n, "edges": int(ind.size) // 2}
        print(json.dumps(dict(base, sources=ns, batches=res["batches"], levels=res["levels"], reached=res["reached"], bc_ms=ms,
                              bc_loop_ms=res["loop_ms"], bc_ms_per_batch=ms / res["batches"], bc_ms_per_source=ms / ns,
                              bfs_batch_ms=ms_bfs, bc_over_bfs_batch=ms / ms_bfs)), flush=True)
        nl = 1 if name == "grid" else min(a.loop_sources, ns)
        ms_part, _ = timed(g, lambda: g.bc(v, A, src[:nl], None), a.reps)
        part = v.extractTuples()[1].astype(np.float64)
        ms_loop, vals = timed(g, lambda: op_by_op(g, A, n, src[:nl], d, d_scmp), 1 if name == "grid" else a.reps)
        # the loop works in f32 all the way: compared loosely, as a check that it computes the same thing -- where both are
        # finite: on the grid the path counts pass f32's range (the loop's) and, from most sources, f64's (bc's: undefined
        # by its contract), and only the times mean anything
        finite = bool(np.all(np.isfinite(vals)) and np.all(np.isfinite(part)))
        err = float(np.abs(vals - part).max() / max(part.max(), 1.0)) if finite else None
        same = bool(err < 1e-3) if finite else None
        good = good and same is not False
        print(json.dumps(dict(base, loop_sources=nl, op_by_op_ms_per_source=ms_loop / nl, bc_ms_on_loop_sources=ms_part,
                              op_by_op_per_source_over_bc_per_source=(ms_loop / nl) / (ms / ns), finite=finite,
                              op_by_op_max_difference=err, same=same)), flush=True)
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
