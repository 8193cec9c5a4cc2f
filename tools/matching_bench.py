"""Greedy matching (csrc/matching.hip: grb_matching) on the bench shapes, with the library's own grb_msf and grb_mis on the
same matrix and the host's greedy scan beside it:

  graphs     rmat16, rmat20 (edge factor 16, seed 1, symmetrised), each with random i32 weights in 1 .. 64 ("i") and with
             random f32 weights in (0, 1] ("f"), in each of the three modes; grid (a 1000 x 1000 grid, i32 weights in 1 .. 64,
             heaviest first); pathh (a path of 1 M vertices, hashed keys) and pathe (the same path with equal weights,
             heaviest first: the worst case, n / 2 rounds).  rmatN, gridN and pathhN / patheN take any size
  matching   api.matching with C: ms per call (the median of --reps after a warm one; pathe: one call), the device's rounds,
             passes and evaluations, the matching's edges and weight.  Every call must give the same mate, the same C and
             the same weight bits: asserted
  msf, mis   api.msf and api.mis on the same matrix (mis takes an i32 matrix: for the f32 shapes one of ones with the same
             structure): ms per call, the median of --reps
  host       the greedy scan on the host (np.lexsort((max, min, p)) and one loop), one wall-clock run, for scale only; its
             mate is asserted equal to the device's.  Skipped above --host-edges edges (the loop is Python)

The device's figures are timed with HIP events on the library's stream (grb_timer_start / grb_timer_stop around the call).

  python tools/matching_bench.py [--only rmat16i,rmat16f,rmat20i,rmat20f,grid,pathh,pathe] [--reps 5] [--host-edges 3000000]
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
HEAVIEST, LIGHTEST, HASHED = 0, 1, 2
SEED = 1


def graph(name):
    """-> n, lo, hi, w (each undirected edge once, lo < hi), the element type, the modes to run, whether one call is enough"""
    from graphblast_amd.graphgen import rmat_edges
    rng = np.random.default_rng(7)
    dt, modes, once, equal = I, (HEAVIEST,), False, False
    if name.startswith("rmat"):
        dt = F if name.endswith("f") else I
        modes = (HEAVIEST, LIGHTEST, HASHED)
        s, d, n = rmat_edges(int(name[4:].rstrip("if")), 16, seed=1)
        s, d = np.asarray(s, np.int64), np.asarray(d, np.int64)
    elif name.startswith("path"):
        n = int(name[5:] or 1000000)
        s = np.arange(n - 1, dtype=np.int64)
        d = s + 1
        equal = name[4] == "e"
        modes = (HEAVIEST,) if equal else (HASHED,)
        once = equal
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
    if equal:
        w = np.full(lo.size, 7, I)
    elif dt is F:
        w = (1.0 - rng.random(lo.size)).astype(F)          # (0, 1]
        w[w == 0] = F(1)
    else:
        w = rng.integers(1, 65, lo.size).astype(I)
    return n, lo, hi, w, dt, modes, once


def mix(x):
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = (x.astype(np.uint64) * np.uint64(0x85ebca6b)).astype(np.uint32)
    x = x ^ (x >> np.uint32(13))
    x = (x.astype(np.uint64) * np.uint64(0xc2b2ae35)).astype(np.uint32)
    return x ^ (x >> np.uint32(16))


def host_greedy(n, lo, hi, w, mode, seed):
    """the definition: the edges in the order of (p, min, max), an edge kept when both ends are free"""
    if mode == HASHED:
        p = mix(mix(((lo + seed) & 0xffffffff).astype(np.uint32)) ^ hi.astype(np.uint32))
    else:
        p = w.astype(np.float64) if w.dtype == F else w.astype(np.int64)
        p = -p if mode == HEAVIEST else p
    order = np.lexsort((hi, lo, p))
    mate = [-1] * n
    for a, b in zip(lo[order].tolist(), hi[order].tolist()):
        if mate[a] < 0 and mate[b] < 0:
            mate[a], mate[b] = b, a
    return np.asarray(mate, I)


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16i,rmat16f,rmat20i,rmat20f,grid,pathh,pathe")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-edges", type=int, default=3000000)
    a = ap.parse_args()
    import scipy.sparse as sp
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("matching_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    assert desc.loadArgs() == 0
    for name in a.only.split(","):
        n, lo, hi, w, dt, modes, once = graph(name)
        U = sp.csr_matrix((w, (lo, hi)), shape=(n, n))
        S = (U + U.T).tocsr()
        S.sort_indices()
        A = g.Matrix(n, n, dt)
        assert A.build_csr(S.indptr.astype(I), S.indices.astype(I), S.data.astype(dt)) == 0
        others = {}
        for mode in modes:
            Cm, mate = g.Matrix(n, n, dt), g.Vector(n, I)

            def call():
                info, res = g.matching(mate, Cm, A, mode, SEED, None)
                assert info == 0, info
                return res

            if once:
                runs = [timed_once(g, call)]
            else:
                _, first = timed_once(g, call)            # warm
                first_c = [x.tobytes() for x in Cm.host_csr()]
                first_m = mate.extractTuples()[1].tobytes()
                runs = [timed_once(g, call) for _ in range(max(1, a.reps))]
                assert all(np.float64(r[1]["weight"]).tobytes() == np.float64(first["weight"]).tobytes() for r in runs), name
                assert [x.tobytes() for x in Cm.host_csr()] == first_c and mate.extractTuples()[1].tobytes() == first_m, name
            ms, res = float(np.median([r[0] for r in runs])), runs[-1][1]
            row = dict(graph=name, mode=mode, n=n, nnz=int(S.nnz), matching_ms=ms, loop_ms=res["loop_ms"], rounds=res["rounds"],
                       passes=res["passes"], evaluations=res["evaluations"], evaluations_per_vertex=res["evaluations"] / max(1, n),
                       matched=res["matched"], weight=res["weight"], exposed=res["exposed"], isolated=res["isolated"],
                       launches=res["launches"], us_per_pass=1e3 * res["loop_ms"] / max(1, res["passes"]))
            print(json.dumps(row), flush=True)            # (the host may take long: the device's figures first)
            if not others:
                B = A                                     # mis takes an i32 matrix: the same structure, ones
                if dt is F:
                    B = g.Matrix(n, n, I)
                    assert B.build_csr(S.indptr.astype(I), S.indices.astype(I), np.ones(S.nnz, I)) == 0
                Fm, comp = g.Matrix(n, n, dt), g.Vector(n, I)
                for what, fn in (("msf", lambda: g.msf(Fm, comp, A, None)), ("mis", lambda: g.mis(g.Vector(n, I), B, SEED, desc))):
                    def other():
                        assert fn()[0] == 0
                    timed_once(g, other)                  # warm
                    others[what + "_ms"] = float(np.median([timed_once(g, other)[0] for _ in range(max(1, a.reps))]))
            row.update(others)
            row.update(matching_over_msf=ms / others["msf_ms"], matching_over_mis=ms / others["mis_ms"])
            if lo.size <= a.host_edges:
                t0 = time.perf_counter()
                want = host_greedy(n, lo, hi, w, mode, SEED)
                row["host_ms"] = 1e3 * (time.perf_counter() - t0)
                assert np.array_equal(want, mate.extractTuples()[1]), (name, mode)
                row.update(host_over_matching=row["host_ms"] / ms, equal_to_host=True)
            print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
