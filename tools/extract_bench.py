"""extract (csrc/extract.hip) on RMAT-22 ef16 symmetrised, seed 1 (the bench's matrix; values 1, f32):

  induced25 / induced1   the induced subgraph of a random 25 % / 1 % of the vertices: C = A(S, S), S ascending
  perm                   C = A(p, p) for a random permutation p: the lists are in no order, so the result is sorted
  all                    C = A(ALL, ALL), against grb_transpose under GrB_INP0 = GrB_TRAN (both give a copy of A)
  lists25                the induced25 lists on an EMPTY matrix of the same shape: what validating the lists, copying them
                         to the device and inverting them costs, with every fixed cost of a call, and nothing else

Per workload: a warm-up call, then the median of the timed calls end to end (every call returns with the device
synchronised; C reused), by the host clock and by the library's HIP events (grb_timer_start / grb_timer_stop around the
call); the compulsory bytes -- per orientation, the selected rows' indices and values read once and C's pointers, indices
and values written once -- and the call's rate over them as a share of 8 TB/s; a check against scipy's A[I][:, J].  The
split into symbolic and numeric kernels comes from a separate `rocprofv3 --kernel-trace --stats` run of the same command
(kernels: xt_*; xt_rows_kernel<G, 0> is the symbolic pass, <G, 1> and <G, 2> the numeric one).  torch, as a yardstick
only and in a child process under a time limit: torch.index_select twice on the sparse CSR tensor, then on the sparse
COO tensor; whichever this build does not support is reported by name, with its error.

  python tools/extract_bench.py [--reps 10] [--only induced25,...] [--no-torch] [--no-scipy]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
ALL = "induced25,induced1,perm,all,lists25"
SCALE = 22


def rmat(scale, seed):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=True)
    host = [tuple(x.cpu().numpy().astype(np.int32) for x in gr[k]) for k in ("csr", "csc")]
    del s, d, gr
    torch.cuda.empty_cache()
    return n, host[0], host[1]


def lists_of(name, n):
    r = np.random.default_rng(22)
    if name in ("induced25", "lists25"):
        s = np.sort(r.choice(n, n // 4, replace=False)).astype(np.int32)
        return s, s
    if name == "induced1":
        s = np.sort(r.choice(n, n // 100, replace=False)).astype(np.int32)
        return s, s
    if name == "perm":
        p = r.permutation(n).astype(np.int32)
        return p, p
    return None, None


def torch_child(name, scale):
    import torch
    n, csr, _ = rmat(scale, 1)
    rows, cols = lists_of(name, n)
    dev = torch.device("cuda", 0)
    ri = torch.from_numpy(rows.astype(np.int64)).to(dev)
    cj = torch.from_numpy(cols.astype(np.int64)).to(dev)
    val = torch.ones(csr[1].size, dtype=torch.float32)
    A = torch.sparse_csr_tensor(torch.from_numpy(csr[0].astype(np.int64)), torch.from_numpy(csr[1].astype(np.int64)), val,
                                size=(n, n), device=dev)
    out = {}
    for label, M in (("index_select x2 on sparse CSR", lambda: A), ("index_select x2 on sparse COO", lambda: A.to_sparse_coo())):
        try:
            X = M()
            f = lambda: torch.index_select(torch.index_select(X, 0, ri), 1, cj)   # noqa: E731
            C = f()
            torch.cuda.synchronize()
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                C = f()
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            out[label] = {"ms": 1e3 * float(np.median(ts)), "nnz": int(C._nnz())}
        except Exception as e:   # noqa: BLE001 -- the table names what this build does not support
            out[label] = "unsupported: " + str(e).strip().splitlines()[0][:160]
    print(json.dumps(out))


def timed(g, call, reps):
    lib = g._lib.load()
    assert call() == 0                                    # warm-up
    host, dev = [], []
    for _ in range(reps):
        ms = ctypes.c_float(0)
        assert lib.grb_timer_start() == 0
        t0 = time.perf_counter()
        assert call() == 0                                # returns with the device synchronised
        host.append(time.perf_counter() - t0)
        assert lib.grb_timer_stop(ctypes.byref(ms)) == 0
        dev.append(ms.value)
    return float(np.median(host)), float(np.median(dev))


def run(name, A, S, n, csr, reps, with_torch, with_scipy, scale):
    import graphblast_amd as g
    rows, cols = lists_of(name, n)
    ni = n if rows is None else rows.size
    nj = n if cols is None else cols.size
    d = g.Descriptor()
    assert d.loadArgs() == 0
    src = A
    if name == "lists25":
        src = g.Matrix(n, n, np.float32)
        z = np.zeros(n + 1, np.int32)
        assert src.build_csr(z, np.zeros(0, np.int32), np.zeros(0, np.float32), csc=(z, np.zeros(0, np.int32), np.zeros(0, np.float32))) == 0
    Cm = g.Matrix(ni, nj, np.float32)
    med, med_dev = timed(g, lambda: g.extract(Cm, None, None, src, rows, cols, d), reps)
    cp, ci, cv = Cm.host_csr()
    nnz_c = int(cp[-1])
    sel = np.arange(n) if rows is None else rows
    read_entries = 0 if name == "lists25" else int(np.diff(csr[0])[sel].sum())
    # the matrix is symmetric: the CSC side reads and writes as much as the CSR side
    bytes_ = 2 * (8 * read_entries + 4 * (ni + 1) + 8 * nnz_c)
    out = {"workload": name, "n": n, "nnz_A": int(csr[1].size), "rows": int(ni), "cols": int(nj), "nnz_C": nnz_c,
           "source_entries_read": read_entries, "max_row_C": int(np.diff(cp).max()) if ni else 0, "calls": reps,
           "median_ms": 1e3 * med, "median_ms_hip_events": med_dev, "compulsory_bytes": int(bytes_),
           "call_GBps": bytes_ / med / 1e9, "call_share_of_8TBps": bytes_ / med / HBM_BYTES_PER_S}
    ok = True
    if name == "all":
        T = g.Matrix(n, n, np.float32)
        dt = g.Descriptor()
        assert dt.loadArgs() == 0 and dt.toggle(g.GrB_INP0) == 0
        tr, tr_dev = timed(g, lambda: g.transpose(T, None, None, A, dt), reps)
        out.update({"transpose_tran_ms": 1e3 * tr, "extract_over_transpose": med / tr})
        ok = np.array_equal(cp, csr[0]) and np.array_equal(ci, csr[1])
        out["check"] = bool(ok)
    elif with_scipy and name != "lists25":
        t0 = time.perf_counter()
        W = S[rows][:, cols].tocsr()
        out["scipy_1core_ms"] = 1e3 * (time.perf_counter() - t0)
        W.sort_indices()
        ok = np.array_equal(cp, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(cv, W.data.astype(np.float32))
        out["check"] = bool(ok)
    if with_torch and name in ("induced25", "induced1"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", name, "--scale", str(scale)],
                               capture_output=True, text=True, timeout=300)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            out["torch"] = json.loads(line[-1]) if r.returncode == 0 and line else \
                "unavailable: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200]
        except subprocess.TimeoutExpired:
            out["torch"] = "unavailable (time limit)"
    print(json.dumps(out), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=ALL)
    ap.add_argument("--scale", type=int, default=SCALE)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--torch-child", default=None)
    a = ap.parse_args()
    if a.torch_child:
        torch_child(a.torch_child, a.scale)
        return 0
    import scipy.sparse as sp
    import graphblast_amd as g
    n, csr, csc = rmat(a.scale, 1)
    one = np.ones(csr[1].size, np.float32)
    A = g.Matrix(n, n, np.float32)
    assert A.build_csr(csr[0], csr[1], one, csc=(csc[0], csc[1], one)) == 0
    S = sp.csr_matrix((one, csr[1], csr[0]), shape=(n, n))
    ok = True
    for name in a.only.split(","):
        ok = run(name, A, S, n, csr, max(10, a.reps), not a.no_torch, not a.no_scipy, a.scale) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
