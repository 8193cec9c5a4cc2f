"""Matrix eWiseAdd / eWiseMult and transpose (csrc/ewise_matrix.hip) on seeded workloads:

  rmat22_add / rmat22_mult   RMAT-22 ef16 symmetrised, seed 1 (+) / (x) seed 2
  rmat22_sym                 RMAT-22 ef16 directed, A + A^T (GrB_INP1 = GrB_TRAN)
  random20_add               two uniformly random 2^20 x 2^20 matrices of 16 entries per row, A + B
  tr_rmat16_prod             transpose of the RMAT-16 A.A product (CSR only: the device sort)
  tr_rmat22                  transpose of a built RMAT-22 matrix (both orientations: two copies)

Values are 1 (RMAT) or random integers 1..3 in f32, so results are exact.  Per workload: the median of the timed calls
end to end (both passes, the allocations, the host copy of the row pointers; every call returns with the device
synchronised; C reused), the compulsory bytes (each operand's CSR read once and C's CSR written once, plus the CSC side
when C gets one) and the whole call's rate over them as a share of 8 TB/s, a check against scipy, scipy's time on one
host core, and -- as a yardstick only, in a child process under a time limit -- torch's sparse CSR A + B on the device.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of the same command (kernels: ewm_*).

  python tools/ewise_bench.py [--reps 5] [--only rmat22_add,...] [--no-torch] [--no-scipy]
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
ALL = "rmat22_add,rmat22_mult,rmat22_sym,random20_add,tr_rmat16_prod,tr_rmat22"


def rmat(scale, seed, symmetrize):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=symmetrize)
    host = [tuple(x.cpu().numpy().astype(np.int32) for x in gr[k]) for k in ("csr", "csc")]
    return n, host[0], host[1]


def random_csr(n, seed):
    r = np.random.default_rng(seed)
    key = np.unique(np.repeat(np.arange(n, dtype=np.int64), 16) * n + r.integers(0, n, 16 * n))
    ptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(key // n, minlength=n), out=ptr[1:])
    return ptr, (key % n).astype(np.int32), r.integers(1, 4, key.size).astype(np.float32)


def operands(name):
    """-> n, [(ptr, ind, val, csc or None)] of the workload's operands"""
    if name.startswith("rmat22") or name == "tr_rmat22":
        if name == "rmat22_sym":
            n, csr, csc = rmat(22, 1, False)
            one = np.ones(csr[1].size, np.float32)
            return n, [(csr[0], csr[1], one, (csc[0], csc[1], one))]
        out = []
        for seed in ((1,) if name == "tr_rmat22" else (1, 2)):
            n, csr, csc = rmat(22, seed, True)
            one = np.ones(csr[1].size, np.float32)
            out.append((csr[0], csr[1], one, (csc[0], csc[1], one)))
        return n, out
    if name == "random20_add":
        n = 1 << 20
        return n, [random_csr(n, 5) + (None,), random_csr(n, 6) + (None,)]
    if name == "tr_rmat16_prod":
        n, csr, _ = rmat(16, 2, True)
        val = np.random.default_rng(7).integers(1, 4, csr[1].size).astype(np.float32)
        return n, [(csr[0], csr[1], val, None)]
    raise ValueError(name)


def csr_bytes(nrows, nnz):
    return 4 * (nrows + 1) + 8 * nnz


def torch_child(name, reps):
    """the torch yardstick: sparse CSR A + B (A * B for the intersection) on the device, in its own process (see run)"""
    import torch
    n, ops = operands(name)
    dev = torch.device("cuda", 0)
    ts = [torch.sparse_csr_tensor(torch.from_numpy(p.astype(np.int64)), torch.from_numpy(i.astype(np.int64)),
                                  torch.from_numpy(v), size=(n, n), device=dev) for p, i, v, _ in ops]
    A = ts[0]
    B = ts[1] if len(ts) > 1 else ts[0].t().to_sparse_csr()
    f = (lambda: A * B) if name.endswith("_mult") else (lambda: A + B)   # noqa: E731
    C = f()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        C = f()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    print(json.dumps({"torch_ms": 1e3 * float(np.median(times)), "nnz": int(C._nnz())}))


def run(name, reps, with_torch, with_scipy):
    import scipy.sparse as sp
    import graphblast_amd as g
    n, ops = operands(name)
    mats = []
    for p, i, v, csc in ops:
        M = g.Matrix(n, n, np.float32)
        assert M.build_csr(p, i, v, csc=csc) == 0
        mats.append(M)
    d = g.Descriptor()
    assert d.loadArgs() == 0
    S = [sp.csr_matrix((v, i, p), shape=(n, n)) for p, i, v, _ in ops]
    out = {"workload": name, "n": n, "nnz_in": [int(x[1].size) for x in ops]}
    Cm = g.Matrix(n, n, np.float32)
    if name.startswith("tr_"):
        src = mats[0]
        if name == "tr_rmat16_prod":                     # the product result: CSR only
            src = g.Matrix(n, n, np.float32)
            assert g.mxm(src, None, None, "PlusMultiplies", mats[0], mats[0], d) == 0
            pp, pi, pv = src.host_csr()
            W = sp.csr_matrix((pv, pi, pp), shape=(n, n))
            read = csr_bytes(n, W.nnz)
        else:
            W = S[0]
            read = 2 * csr_bytes(n, W.nnz)
        call = lambda: g.transpose(Cm, None, None, src, d)   # noqa: E731
        want = lambda: W.T.tocsr()                           # noqa: E731
        written = 2 * csr_bytes(n, W.nnz)
    else:
        add = not name.endswith("_mult")
        fn = g.eWiseAdd if add else g.eWiseMult
        if name == "rmat22_sym":
            A = B = mats[0]
            dd = g.Descriptor()
            assert dd.loadArgs() == 0 and dd.toggle(g.GrB_INP1) == 0
            call = lambda: fn(Cm, None, None, "PlusMultiplies", A, B, dd)   # noqa: E731
            want = lambda: S[0] + S[0].T                                   # noqa: E731
            read = 2 * csr_bytes(n, ops[0][1].size) * 2                    # both orientations of both operands
        else:
            A, B = mats
            call = lambda: fn(Cm, None, None, "PlusMultiplies", A, B, d)   # noqa: E731
            want = (lambda: S[0] + S[1]) if add else (lambda: S[0].multiply(S[1]))   # noqa: E731
            both_sides = all(x[3] is not None for x in ops)
            read = (2 if both_sides else 1) * sum(csr_bytes(n, x[1].size) for x in ops)
        written = None
    assert call() == 0                                    # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        assert call() == 0                                # returns with the device synchronised
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts))
    cp, ci, cv = Cm.host_csr()
    nnz_c = int(cp[-1])
    try:
        Cm.host_csc()
        has_csc = True
    except g._lib.GrbError:
        has_csc = False
    if written is None:
        written = (2 if has_csc else 1) * csr_bytes(n, nnz_c)
    t0 = time.perf_counter()
    W = sp.csr_matrix(want())
    scipy_s = time.perf_counter() - t0
    W.sort_indices()
    ok = np.array_equal(cp, W.indptr) and np.array_equal(ci, W.indices) and np.array_equal(cv, W.data.astype(np.float32))
    bytes_ = read + written
    out.update({"nnz_C": nnz_c, "max_row_C": int(np.diff(cp).max()), "C_has_csc": has_csc, "median_ms": 1e3 * med,
                "calls": reps, "compulsory_bytes": int(bytes_), "call_GBps": bytes_ / med / 1e9,
                "call_share_of_8TBps": bytes_ / med / HBM_BYTES_PER_S, "check": bool(ok)})
    if with_scipy:
        out["scipy_1core_ms"] = 1e3 * scipy_s
    if with_torch and not name.startswith("tr_"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", name, "--reps", str(reps)],
                               capture_output=True, text=True, timeout=240)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
            if r.returncode == 0 and line:
                t = json.loads(line[-1])
                out["torch_ms"] = t["torch_ms"]
                out["torch_over_ours"] = t["torch_ms"] / (1e3 * med)
                out["torch_nnz_agrees"] = t["nnz"] == nnz_c
            else:
                out["torch"] = "unavailable: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200]
        except subprocess.TimeoutExpired:
            out["torch"] = "unavailable (time limit)"
    print(json.dumps(out), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default=ALL)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-scipy", action="store_true")
    ap.add_argument("--torch-child", default=None)
    a = ap.parse_args()
    if a.torch_child:
        torch_child(a.torch_child, a.reps)
        return 0
    ok = True
    for name in a.only.split(","):
        ok = run(name, max(5, a.reps), not a.no_torch, not a.no_scipy) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
