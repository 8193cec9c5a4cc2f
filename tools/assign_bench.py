"""assign into a matrix (csrc/assign_matrix.hip) on RMAT-22 ef16 symmetrised, seed 1 (the bench's matrix; values 1, f32):

  sub_asc     C(S, S) = A, S a random half of the vertices in ascending order, A = extract(C, Q, Q) for another random
              half Q; no accum (what C stores inside S x S and A does not is deleted)
  sub_perm    the same with S in permuted order: T goes through the radix sort
  all_plus    C(ALL, ALL) += B with plus as the accum, B = C(p, p) for a random permutation p (a relabelled copy); against
              grb_matrix_eWiseAdd under PlusMultiplies on the same operands (the same merge: the natural yardstick)
  row / col   C(i, ALL) = u and C(ALL, j) = u for a dense u, i = j = the longest row
  const_mask  C<C>(K, K) = 1 for 4096 random vertices K under C itself as the mask

Per workload: a warm-up call, then the median of the timed calls end to end, each on a fresh device copy of C made outside
the timed region (every call returns with the device synchronised), by the host clock and by the library's HIP events.
scipy's host assignment, one core, for sub_asc (C - D C D + P A P^T, D the indicator of S, P its selection matrix) and
all_plus (C + B), with the ratio and a check of the device result against it.  One JSON line per workload.

  python tools/assign_bench.py [--reps 5] [--only sub_asc,...] [--no-scipy] [--scale 22]
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

ALL = "sub_asc,sub_perm,all_plus,row,col,const_mask"


def rmat(scale, seed):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=True)
    host = [tuple(x.cpu().numpy().astype(np.int32) for x in gr[k]) for k in ("csr", "csc")]
    del s, d, gr
    torch.cuda.empty_cache()
    return n, host[0], host[1]


def timed(g, fresh, call, reps):
    lib = g._lib.load()
    assert call(fresh()) == 0                             # warm-up
    host, dev = [], []
    Cm = None
    for _ in range(reps):
        Cm = fresh()
        ms = ctypes.c_float(0)
        assert lib.grb_timer_start() == 0
        t0 = time.perf_counter()
        assert call(Cm) == 0                              # returns with the device synchronised
        host.append(time.perf_counter() - t0)
        assert lib.grb_timer_stop(ctypes.byref(ms)) == 0
        dev.append(ms.value)
    return float(np.median(host)), float(np.median(dev)), Cm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=ALL)
    ap.add_argument("--scale", type=int, default=22)
    ap.add_argument("--no-scipy", action="store_true")
    a = ap.parse_args()
    import graphblast_amd as g
    n, csr, csc = rmat(a.scale, 1)
    one = np.ones(csr[1].size, np.float32)
    C0 = g.Matrix(n, n, np.float32)
    assert C0.build_csr(csr[0], csr[1], one, csc=(csc[0], csc[1], one)) == 0
    d = g.Descriptor()
    assert d.loadArgs() == 0
    dt = g.Descriptor()
    assert dt.loadArgs() == 0 and dt.toggle(g.GrB_INP0) == 0

    def fresh():                                          # a device copy of C0 with both orientations
        X = g.Matrix(n, n, np.float32)
        assert g.transpose(X, None, None, C0, dt) == 0
        return X

    r = np.random.default_rng(22)
    half = r.permutation(n)[:n // 2].astype(np.int32)
    other = np.sort(r.permutation(n)[:n // 2]).astype(np.int32)
    S = None
    if not a.no_scipy:
        import scipy.sparse as sp
        S = sp.csr_matrix((one, csr[1], csr[0]), shape=(n, n))
    ok = True
    for name in a.only.split(","):
        out = {"workload": name, "n": n, "nnz_C": int(csr[1].size), "calls": a.reps}
        if name in ("sub_asc", "sub_perm"):
            I = np.sort(half) if name == "sub_asc" else half
            A = g.Matrix(I.size, I.size, np.float32)
            assert g.extract(A, None, None, C0, other, other, d) == 0
            med, med_dev, Cm = timed(g, fresh, lambda X: g.assign_matrix(X, None, None, A, I, I, d), a.reps)
            out.update({"rows": int(I.size), "nnz_A": A.nvals(), "nnz_out": Cm.nvals()})
            if S is not None and name == "sub_asc":
                k = I.size
                t0 = time.perf_counter()
                ind = np.zeros(n, np.float32)
                ind[I] = 1
                D = sp.diags(ind)
                P = sp.csr_matrix((np.ones(k, np.float32), (I, np.arange(k))), shape=(n, k))
                W = (S - D @ S @ D + P @ S[other][:, other] @ P.T).tocsr()
                W.eliminate_zeros()
                out["scipy_1core_ms"] = 1e3 * (time.perf_counter() - t0)
                out["scipy_over_device"] = out["scipy_1core_ms"] / (1e3 * med)
                W.sort_indices()
                p, i, _ = Cm.host_csr()
                out["check"] = bool(np.array_equal(p, W.indptr) and np.array_equal(i, W.indices))
                ok = ok and out["check"]
        elif name == "all_plus":
            p = r.permutation(n).astype(np.int32)
            B = g.Matrix(n, n, np.float32)
            assert g.extract(B, None, None, C0, p, p, d) == 0
            med, med_dev, Cm = timed(g, fresh, lambda X: g.assign_matrix(X, None, "plus", B, None, None, d), a.reps)
            E = g.Matrix(n, n, np.float32)
            ew, ew_dev, _ = timed(g, lambda: E, lambda X: g.eWiseAdd(X, None, None, "PlusMultiplies", C0, B, d), a.reps)
            out.update({"nnz_B": B.nvals(), "nnz_out": Cm.nvals(), "eWiseAdd_ms": 1e3 * ew, "assign_over_eWiseAdd": med / ew})
            same = all(np.array_equal(x, y) for x, y in zip(Cm.host_csr(), E.host_csr()))
            out["check"] = bool(same)
            ok = ok and same
            if S is not None:
                t0 = time.perf_counter()
                W = (S + S[p][:, p]).tocsr()
                out["scipy_1core_ms"] = 1e3 * (time.perf_counter() - t0)
                out["scipy_over_device"] = out["scipy_1core_ms"] / (1e3 * med)
        elif name in ("row", "col"):
            j = int(np.argmax(np.diff(csr[0])))
            u = g.Vector(n, np.float32)
            assert u.build(np.full(n, 2, np.float32), n) == 0
            rc = (j, None) if name == "row" else (None, j)
            med, med_dev, Cm = timed(g, fresh, lambda X: g.assign_matrix(X, None, None, u, rc[0], rc[1], d), a.reps)
            out.update({"index": j, "nnz_out": Cm.nvals()})
        elif name == "const_mask":
            K = np.sort(r.permutation(n)[:4096]).astype(np.int32)
            med, med_dev, Cm = timed(g, fresh, lambda X: g.assign_matrix(X, C0, None, 1, K, K, d), a.reps)
            out.update({"rows": 4096, "nnz_out": Cm.nvals()})
        else:
            raise SystemExit("unknown workload " + name)
        out.update({"median_ms": 1e3 * med, "median_ms_hip_events": med_dev})
        print(json.dumps(out), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
