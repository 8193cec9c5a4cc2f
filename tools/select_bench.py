"""select (csrc/select.hip) on RMAT-22 ef16 symmetrised, seed 1 (the bench's matrix) and on RMAT-16, f32 weights 1 .. 64
with a tenth of them replaced by stored zeros:

  tril       C = select(A, TRIL, 0): the lower triangle with the diagonal
  offdiag    C = select(A, OFFDIAG, 0): nearly everything is kept
  valuene0   C = select(A, VALUENE, 0): the injected zeros are dropped
  valuelt    C = select(A, VALUELT, the median weight)
  host_tril  grb_matrix_tril(C, A): the host loop that was the only way to the result of `tril` before select

Per workload: a warm-up call, then the median of the timed calls end to end (every call returns with the device
synchronised; C reused), by the library's HIP events (grb_timer_start / grb_timer_stop around the call) and by the host
clock.  A call does both orientations of C, the allocations of the result, the host copy of its pointers and the CSC's
SpMV plan, so its time is what a caller pays, not a kernel's.  The algorithmic bytes, per orientation: the pointers and
the indices read once (the values too for a value predicate), the new pointers and the kept indices and values written
once; the call's rate over them, next to the 5.0 - 5.8 TB/s of the library's vector streaming primitives.  The kernels'
own times (sel_kernel<op, type, write>) come from a separate `rocprofv3 --kernel-trace --stats` run of the same command.
Checks: `tril` has the CSR of host_tril bit for bit; every other result has numpy's count of kept entries.

  python tools/select_bench.py [--reps 10] [--scales 22,16] [--only tril,...] [--tril-reps 3]
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
ALL = "tril,offdiag,valuene0,valuelt,host_tril"


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


def kept_mask(name, rows, ind, val, thunk):
    if name in ("tril", "host_tril"):
        return ind <= rows
    if name == "offdiag":
        return ind != rows
    if name == "valuene0":
        return val != 0
    return val < np.float32(thunk)


def run_scale(g, scale, names, reps, tril_reps):
    n, ptr, ind = rmat(scale, 1)
    nnz = int(ind.size)
    rng = np.random.default_rng(scale)
    val = rng.integers(1, 65, nnz).astype(np.float32)
    val[rng.random(nnz) < 0.1] = 0.0
    median = float(np.median(val))
    A = g.Matrix(n, n, np.float32)
    assert A.build_csr(ptr, ind, val) == 0
    d = g.Descriptor()
    assert d.loadArgs() == 0
    rows = np.repeat(np.arange(n, dtype=np.int32), np.diff(ptr))
    ops = {"tril": ("tril", 0), "offdiag": ("offdiag", 0), "valuene0": ("valuene", 0), "valuelt": ("valuelt", median)}
    ok = True
    results = {}
    for name in names:
        Cm = g.Matrix(n, n, np.float32)
        if name == "host_tril":
            host_s, dev_ms = timed(g, lambda: g.tril(Cm, A, d), tril_reps)
            calls = tril_reps
        else:
            op, thunk = ops[name]
            host_s, dev_ms = timed(g, lambda: g.select(Cm, None, None, op, A, thunk, d), reps)
            calls = reps
        kept = int(Cm.nvals())
        want = int(np.count_nonzero(kept_mask(name, rows, ind, val, median)))
        value_op = name in ("valuene0", "valuelt")
        # both orientations (the matrix has its CSC, so C gets one): read ptr + ind (+ val), write ptr + kept (ind, val)
        bytes_ = 2 * (4 * (n + 1) + 4 * nnz * (2 if value_op else 1) + 4 * (n + 1) + 8 * kept)
        out = {"workload": name, "scale": scale, "n": n, "nnz_A": nnz, "max_row": int(np.diff(ptr).max()), "nnz_C": kept,
               "calls": calls, "median_ms_hip_events": dev_ms, "median_ms_host": 1e3 * host_s, "check_nvals": kept == want}
        if name != "host_tril":
            out.update({"algorithmic_bytes": int(bytes_), "call_GBps": bytes_ / (dev_ms * 1e-3) / 1e9,
                        "streaming_primitives_TBps": list(STREAM_TBPS),
                        "share_of_streaming_primitives": [bytes_ / (dev_ms * 1e-3) / (t * 1e12) for t in STREAM_TBPS]})
        ok = ok and kept == want
        if name in ("tril", "host_tril"):
            results[name] = (dev_ms, [x.copy() for x in Cm.host_csr()])
        print(json.dumps(out), flush=True)
    if "tril" in results and "host_tril" in results:
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(results["tril"][1], results["host_tril"][1]))
        ok = ok and same
        print(json.dumps({"workload": "tril vs host_tril", "scale": scale, "select_ms": results["tril"][0],
                          "host_tril_ms": results["host_tril"][0], "host_tril_over_select": results["host_tril"][0] / results["tril"][0],
                          "same_csr_bits": bool(same)}), flush=True)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--tril-reps", type=int, default=3)
    ap.add_argument("--scales", default="22,16")
    ap.add_argument("--only", default=ALL)
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("select_bench needs the GPU: " + g.device_info())
    ok = True
    for scale in (int(s) for s in a.scales.split(",")):
        ok = run_scale(g, scale, a.only.split(","), max(3, a.reps), max(1, a.tril_reps)) and ok
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
