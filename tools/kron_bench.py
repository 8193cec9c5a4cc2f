"""kronecker (csrc/kronecker.hip), f32 under PlusMultiplies:

  rmat10     C = A (x) A with A RMAT-10 ef16 symmetrised, seed 1: a 2^20 x 2^20 C, a hub row against a hub row
  seed_pow   a 3 x 3 seed raised to the 12th Kronecker power by repeated calls, P_k = P_(k-1) (x) S: the generator of
             Kronecker graphs.  The last step (P_11 (x) S, 531441 x 531441) is the one timed; the whole chain is timed too.

Per workload: a warm-up call, then the median of the timed calls end to end (every call returns with the device
synchronised; C reused), by the library's HIP events (grb_timer_start / grb_timer_stop around the call) and by the host
clock.  A call does both orientations of C, the allocations of the result, the host copy of its pointers and the CSC's
SpMV plan, so its time is what a caller pays, not a kernel's.  The bytes of C written, per orientation: the pointers and
8 bytes an entry (index and value); the call's rate over them, next to the 5.0 - 5.8 TB/s of the library's vector streaming
primitives.  The kernels' own times (kron_kernel<mul, type>, kron_ptr_kernel) come from a separate
`rocprofv3 --kernel-trace --stats` run of the same command.
Checks: nvals(C) = nvals(A) * nvals(B), and C's row lengths are the products of the operands'.

  python tools/kron_bench.py [--reps 10] [--only rmat10,seed_pow] [--scale 10] [--power 12]
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

STREAM_TBPS = (5.0, 5.8)                                  # the library's vector streaming primitives, for context
ALL = "rmat10,seed_pow"


def rmat(scale, seed):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    s, d, n = rmat_edges(scale, 16, seed=seed, device=torch.device("cuda", 0))
    gr = finalize_edges(s, d, n, symmetrize=True)
    ptr, ind = (x.cpu().numpy().astype(np.int32) for x in gr["csr"])
    del s, d, gr
    torch.cuda.empty_cache()
    return n, ptr, ind


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


def report(name, extra, m, n, nnz, reps, host_s, dev_ms, ok):
    # both orientations (the operands have their CSC, so C gets one): the pointers and 8 bytes an entry
    bytes_ = 4 * (m + 1) + 4 * (n + 1) + 2 * 8 * nnz
    out = {"workload": name, "rows_C": m, "cols_C": n, "nnz_C": nnz, "calls": reps, "median_ms_hip_events": dev_ms,
           "median_ms_host": 1e3 * host_s, "bytes_of_C_written": int(bytes_), "call_GBps": bytes_ / (dev_ms * 1e-3) / 1e9,
           "streaming_primitives_TBps": list(STREAM_TBPS),
           "share_of_streaming_primitives": [bytes_ / (dev_ms * 1e-3) / (t * 1e12) for t in STREAM_TBPS], "check": bool(ok)}
    out.update(extra)
    print(json.dumps(out), flush=True)
    return ok


def lens_ok(Cm, la, lb):
    return np.array_equal(np.diff(Cm.host_csr()[0]).astype(np.int64), np.repeat(la, lb.size) * np.tile(lb, la.size))


def run_rmat(g, scale, reps):
    n, ptr, ind = rmat(scale, 1)
    rng = np.random.default_rng(scale)
    A = g.Matrix(n, n, np.float32)
    assert A.build_csr(ptr, ind, rng.integers(1, 65, ind.size).astype(np.float32)) == 0
    d = g.Descriptor()
    assert d.loadArgs() == 0
    nnz = int(ind.size) ** 2
    if nnz > 2 ** 31 - 1:
        raise SystemExit("RMAT-%d squared has %d entries, more than an index holds" % (scale, nnz))
    Cm = g.Matrix(n * n, n * n, np.float32)
    host_s, dev_ms = timed(g, lambda: g.kronecker(Cm, None, None, "PlusMultiplies", A, A, d), reps)
    lens = np.diff(ptr).astype(np.int64)
    ok = Cm.nvals() == nnz and lens_ok(Cm, lens, lens)
    return report("rmat%d" % scale, {"nnz_A": int(ind.size), "max_row_A": int(lens.max()), "max_row_C": int(lens.max()) ** 2},
                  n * n, n * n, nnz, reps, host_s, dev_ms, ok)


def run_seed(g, power, reps):
    # the seed of a stochastic Kronecker graph's pattern: 5 of 9 entries (5^12 = 2.4e8 entries fit an index, 6^12 do not)
    sp, si = np.array([0, 2, 4, 5], np.int32), np.array([0, 1, 1, 2, 0], np.int32)
    sv = np.array([0.9, 0.6, 0.5, 0.3, 0.6], np.float32)
    seed_nnz = int(si.size)
    S = g.Matrix(3, 3, np.float32)
    assert S.build_csr(sp, si, sv) == 0
    d = g.Descriptor()
    assert d.loadArgs() == 0

    def chain(upto):
        P = S
        for k in range(2, upto + 1):
            Q = g.Matrix(3 ** k, 3 ** k, np.float32)
            if g.kronecker(Q, None, None, "PlusMultiplies", P, S, d) != 0:
                return None
            P = Q
        return P

    prev = chain(power - 1)
    assert prev is not None
    m = 3 ** power
    nnz = seed_nnz ** power
    Cm = g.Matrix(m, m, np.float32)
    host_s, dev_ms = timed(g, lambda: g.kronecker(Cm, None, None, "PlusMultiplies", prev, S, d), reps)
    ok = Cm.nvals() == nnz and lens_ok(Cm, np.diff(prev.host_csr()[0]).astype(np.int64), np.diff(sp).astype(np.int64))
    ok = report("seed_pow last step", {"power": power, "nnz_A": seed_nnz ** (power - 1), "nnz_B": seed_nnz}, m, m, nnz, reps, host_s, dev_ms, ok) and ok
    chain_s, chain_ms = timed(g, lambda: 0 if chain(power) is not None else 1, max(3, reps // 3))
    total = sum(seed_nnz ** k for k in range(2, power + 1))
    print(json.dumps({"workload": "seed_pow chain", "power": power, "calls_per_chain": power - 1, "nnz_written_per_chain": total,
                      "median_ms_hip_events": chain_ms, "median_ms_host": 1e3 * chain_s}), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default=ALL)
    ap.add_argument("--scale", type=int, default=10)
    ap.add_argument("--power", type=int, default=12)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("kron_bench needs the GPU: " + g.device_info())
    ok = True
    names = a.only.split(",")
    if "rmat10" in names:
        ok = run_rmat(g, a.scale, max(3, a.reps)) and ok
    if "seed_pow" in names:
        ok = run_seed(g, a.power, max(3, a.reps)) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
