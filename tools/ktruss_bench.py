"""k-truss and trussness (csrc/ktruss.hip) against the loop a caller writes with the library's operations:

  graphs     RMAT-14 and RMAT-16 (edge factor 16, seed 1, symmetrised), and a grid_edges graph (side 512)
  ktruss     api.ktruss for k = 3, 5, 8: ms per call, rounds, surviving edges
  op-by-op   the same truss by api.mxm under the survivors' mask (PlusMultiplies, the second operand transposed: read from
             the CSR, the graph is symmetric), api.select VALUEGE k - 2 and the values set back to 1 (api.apply, first(1, x)),
             a fresh product and a fresh selection per round: ms per loop, rounds, surviving edges, and the ratio
  trussness  api.trussness: ms per call and kmax

Each figure is the median of five calls after one warm call, timed with HIP events on the library's stream
(grb_timer_start / grb_timer_stop around the call).  The two trusses are compared entry for entry.

  python tools/ktruss_bench.py [--only rmat14,rmat16,grid] [--ks 3,5,8] [--reps 5]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def graph(name):
    from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges
    if name.startswith("rmat"):
        s, d, n = rmat_edges(int(name[4:]), 16, seed=1)
    else:
        s, d, n = grid_edges(512)
    gr = finalize_edges(np.asarray(s), np.asarray(d), n, symmetrize=True)
    ptr, ind = (np.asarray(x).astype(np.int32) for x in gr["csr"])
    return n, ptr, ind


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


def op_by_op(g, A, n, k, d_tran, d):
    """-> (the truss with its supports, rounds)"""
    cur, rounds = A, 0
    while True:
        rounds += 1
        P, K = g.Matrix(n, n, np.float32), g.Matrix(n, n, np.float32)
        assert g.mxm(P, cur, None, "PlusMultiplies", cur, cur, d_tran) == 0
        assert g.select(K, None, None, "valuege", P, k - 2, d) == 0
        if K.nvals() == cur.nvals() or K.nvals() == 0:
            return K, rounds
        info = g.apply(K, None, None, "bind_first", K, d, binop="first", scalar=1.0)   # the values back to 1
        if info != 0:
            raise SystemExit("apply on the selection returned %d" % info)
        cur = K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat14,rmat16,grid")
    ap.add_argument("--ks", default="3,5,8")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("ktruss_bench needs the GPU: " + g.device_info())
    d, d_tran = g.Descriptor(), g.Descriptor()
    assert d.loadArgs() == 0 and d_tran.loadArgs() == 0 and d_tran.toggle(g.GrB_INP1) == 0
    ok = True
    for name in a.only.split(","):
        n, ptr, ind = graph(name)
        A = g.Matrix(n, n, np.float32)
        assert A.build_csr(ptr, ind, np.ones(ind.size, np.float32)) == 0
        base = {"graph": name, "n": n, "edges": int(ind.size) // 2, "max_row": int(np.diff(ptr).max())}
        for k in (int(x) for x in a.ks.split(",")):
            Cm = g.Matrix(n, n, np.float32)
            ms, (info, res) = timed(g, lambda: g.ktruss(Cm, A, k, None), a.reps)
            assert info == 0
            ms_ops, (K, rounds) = timed(g, lambda: op_by_op(g, A, n, k, d_tran, d), a.reps)
            same = all(np.array_equal(x, y) for x, y in zip(Cm.host_csr(), K.host_csr()))
            ok = ok and same
            print(json.dumps(dict(base, k=k, ktruss_ms=ms, ktruss_loop_ms=res["loop_ms"], rounds=res["rounds"],
                                  surviving_edges=res["result_edges"], op_by_op_ms=ms_ops, op_by_op_rounds=rounds,
                                  op_by_op_surviving_edges=K.nvals() // 2, op_by_op_over_ktruss=ms_ops / ms, same=bool(same))),
                  flush=True)
        Tm = g.Matrix(n, n, np.int32)
        ms, (info, res) = timed(g, lambda: g.trussness(Tm, A, None), a.reps)
        assert info == 0
        print(json.dumps(dict(base, trussness_ms=ms, kmax=res["kmax"], rounds=res["rounds"], supports=res["supports"])), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
