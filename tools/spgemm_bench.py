"""The unmasked product C = A (+.x) A (grb_mxm with a null mask, csrc/spgemm.hip) on three seeded workloads:
RMAT-14 and RMAT-16 (edge factor 16, symmetrised), the 4896^2 grid with 60 % of the edges kept (bench.py's road
stand-in) and a uniformly random 2^20 x 2^20 matrix with 16 entries per row (columns spread over the whole range).  Values are random integers 1..3 in f32.  Per workload: the median of the timed calls (after a warm-up,
device synchronised, the output object reused), products/s and outputs/s, the compulsory-bytes floor (read A, read
B once, write 8 B per output plus the row pointers, at 8 TB/s) and the fraction of it achieved, a sampled check of a
few hundred rows against scipy, and -- as a yardstick only, in a child process under a time limit -- torch's
sparse-CSR x sparse-CSR product on the same matrix if it runs on the device.

  python tools/spgemm_bench.py [--reps 5] [--only rmat14,rmat16,grid,random20] [--no-torch]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def workload(name):
    import torch
    from graphblast_amd.graphgen import rmat_edges, grid_edges, finalize_edges
    if name.startswith("rmat"):
        s, d, n = rmat_edges(int(name[4:]), 16, seed=2, device=torch.device("cuda", 0))
    elif name.startswith("random"):                   # 2^scale rows of 16 uniformly random columns: no locality at all
        n = 1 << int(name[6:])
        r = np.random.default_rng(5)
        s, d = np.repeat(np.arange(n), 16), r.integers(0, n, 16 * n)
        gr = finalize_edges(s, d, n, symmetrize=False, want_csc=False)
        ptr, ind = (np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x, dtype=np.int32) for x in gr["csr"])
        return n, ptr, ind, np.random.default_rng(7).integers(1, 4, ind.size).astype(np.float32)
    else:
        s, d, n = grid_edges(4896, keep=0.6, seed=3)
    gr = finalize_edges(s, d, n, symmetrize=True, want_csc=False)
    ptr, ind = (x.cpu().numpy().astype(np.int32) if hasattr(x, "cpu") else np.asarray(x, dtype=np.int32) for x in gr["csr"])
    val = np.random.default_rng(7).integers(1, 4, ind.size).astype(np.float32)
    return n, ptr, ind, val


def torch_child(name, reps):
    """the torch yardstick: runs in its own process (see main)"""
    import torch
    n, ptr, ind, val = workload(name)
    dev = torch.device("cuda", 0)
    A = torch.sparse_csr_tensor(torch.from_numpy(ptr.astype(np.int64)), torch.from_numpy(ind.astype(np.int64)),
                                torch.from_numpy(val), size=(n, n), device=dev)
    C = A @ A
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        C = A @ A
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    print(json.dumps({"torch_ms": 1e3 * float(np.median(ts)), "nnz": int(C._nnz())}))


def run(name, reps, with_torch):
    import scipy.sparse as sp
    import graphblast_amd as g
    n, ptr, ind, val = workload(name)
    A = g.Matrix(n, n, np.float32)
    assert A.build_csr(ptr, ind, val) == 0
    d = g.Descriptor()
    assert d.loadArgs() == 0
    Cm = g.Matrix(n, n, np.float32)
    products = int(np.diff(ptr)[ind].astype(np.int64).sum())
    info = g.mxm(Cm, None, None, "PlusMultiplies", A, A, d)           # warm-up
    assert info == 0, info
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert g.mxm(Cm, None, None, "PlusMultiplies", A, A, d) == 0   # returns with the device synchronised
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    cp, ci, cv = Cm.host_csr()
    nnz_c = int(cp[-1])
    # sampled check against scipy: the 50 longest rows of C and 250 random ones
    rng = np.random.default_rng(1)
    rows = np.unique(np.r_[np.argsort(-np.diff(cp), kind="stable")[:50], rng.choice(n, 250, replace=False)])
    S = sp.csr_matrix((val, ind, ptr), shape=(n, n))
    W = (S[rows] @ S).tocsr()
    W.sort_indices()
    ok = all(np.array_equal(ci[cp[r]:cp[r + 1]], W.indices[W.indptr[t]:W.indptr[t + 1]]) and
             np.array_equal(cv[cp[r]:cp[r + 1]], W.data[W.indptr[t]:W.indptr[t + 1]]) for t, r in enumerate(rows))
    floor_bytes = 2 * (8 * ind.size + 4 * (n + 1)) + 8 * nnz_c + 4 * (n + 1)
    floor_s = floor_bytes / HBM_BYTES_PER_S
    out = {"workload": name, "n": n, "nnz_A": int(ind.size), "products": products, "nnz_C": nnz_c,
           "max_row_C": int(np.diff(cp).max()), "median_ms": 1e3 * med, "calls": reps,
           "products_per_s": products / med, "outputs_per_s": nnz_c / med,
           "floor_ms": 1e3 * floor_s, "floor_fraction": floor_s / med, "sampled_rows": int(rows.size), "sampled_check": ok}
    if with_torch:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", name, "--reps", str(reps)],
                               capture_output=True, text=True, timeout=120)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode == 0 and line:
                t = json.loads(line[-1])
                out["torch_ms"] = t["torch_ms"]
                out["torch_over_ours"] = t["torch_ms"] / (1e3 * med)
                out["torch_nnz_agrees"] = t["nnz"] == nnz_c
            else:
                out["torch"] = "unavailable"
        except subprocess.TimeoutExpired:
            out["torch"] = "unavailable (time limit)"
    print(json.dumps(out), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="rmat14,rmat16,grid,random20")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--torch-child", default=None)
    a = ap.parse_args()
    if a.torch_child:
        torch_child(a.torch_child, a.reps)
        return 0
    ok = True
    for name in a.only.split(","):
        ok = run(name, max(5, a.reps), not a.no_torch) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
