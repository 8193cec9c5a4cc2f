"""Graph contraction (csrc/contract.hip: grb_relabel, grb_contract) on the bench shapes, with the op-by-op route on the same
library and torch's coalesce on the same device beside it:

  inputs     rmat16, rmat20 (edge factor 16, seed 1, symmetrised, f32 weights 1 .. 8), each contracted
               cdlp      by the labels of grb_cdlp (ten iterations) through grb_relabel, loops kept: the community graph
               matching  by the mate of grb_matching (hashed) through grb_relabel (GRB_RELABEL_MATE), loops dropped: one
                         coarsening step
               cc        by the labels of grb_cc through grb_relabel, loops kept: one giant cluster, the worst case
             drmat16 (the same edges, directed) by the labels of grb_scc, loops dropped: the condensation
             grid (a 1000 x 1000 grid, weights 1 .. 8) by 2 x 2 tiles, loops dropped.  rmatN, drmatN, gridN take any size
  contract   api.contract under "plus" with sizes: ms per call by HIP events around the call (the median of --reps after a
             warm one), the record, and bytes: a model of what the call moves (the keys kernel 24 B an entry of A, every
             8-bit digit of the sort 32 B an entry, heads + scan + starts + fold 48 B a surviving entry, the transposition
             of C 12 + 32 B a digit per entry of C) against the 12 B per kept entry it must at least read
  op-by-op   what a caller had before: the labels pulled to the host, S (n x nc) and S^T built from the host, two unmasked
             grb_mxm PLUS_MULTIPLIES (T = A S, C = S^T T), select OFFDIAG where loops are dropped, grb_transpose for the CSC.
             ms per call, wall clock (it has host parts), the median of --reps.  Its C is asserted equal to grb_contract's:
             pointers and indices exactly, values exactly wherever the exact sum is below 2^24 (above, the route's chain of
             f32 additions rounds and grb_contract's single rounding does not; the count of such entries is printed)
  torch      torch.sparse_coo_tensor(relabelled coordinates, values).coalesce() on the same device, by torch's events: an
             outside yardstick for the sort and the fold alone (no CSR, no CSC, no sizes)

  python tools/contract_bench.py [--only rmat16,rmat20,drmat16,grid] [--reps 5] [--no-torch]
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


def graph(name):
    """-> n, (ptr, ind, val), the partitions to run: (tag, loops)"""
    from graphblast_amd.graphgen import rmat_edges, finalize_edges
    rng = np.random.default_rng(7)
    if name.startswith("grid"):
        w = int(name[4:] or 1000)
        n = w * w
        idx = np.arange(n, dtype=np.int64).reshape(w, w)
        s = np.concatenate([idx[:, :-1].ravel(), idx[:-1, :].ravel()])
        d = np.concatenate([idx[:, 1:].ravel(), idx[1:, :].ravel()])
        ptr, ind = finalize_edges(s, d, n, symmetrize=True, want_csc=False)["csr"]
        parts = (("tiles", 0),)
    elif name.startswith("drmat"):
        s, d, n = rmat_edges(int(name[5:]), 16, seed=1)
        ptr, ind = finalize_edges(np.asarray(s, np.int64), np.asarray(d, np.int64), n, symmetrize=False, want_csc=False)["csr"]
        parts = (("scc", 0),)
    else:
        s, d, n = rmat_edges(int(name[4:]), 16, seed=1)
        ptr, ind = finalize_edges(np.asarray(s, np.int64), np.asarray(d, np.int64), n, symmetrize=True, want_csc=False)["csr"]
        parts = (("cdlp", 1), ("matching", 0), ("cc", 1))
    ptr, ind = np.asarray(ptr, I), np.asarray(ind, I)
    return n, (ptr, ind, rng.integers(1, 9, ind.size).astype(F)), parts


def partition(g, tag, A, n, desc):
    """-> the map as a library vector (dense ranks) and nc"""
    mp = g.Vector(n, I)
    if tag == "tiles":
        w = int(round(n ** 0.5))
        r, c = np.divmod(np.arange(n), w)
        m = (r // 2) * ((w + 1) // 2) + c // 2
        assert mp.build(m.astype(I), n) == 0
        return mp, int(m.max()) + 1
    lab = g.Vector(n, I)
    if tag == "cdlp":
        assert g.cdlp(lab, A, None, max_iter=10)[0] == 0
    elif tag == "cc":
        ptr, ind, _ = A.host_csr()                         # grb_cc takes a matrix of its vector's type
        Ai = g.Matrix(n, n, I)
        assert Ai.build_csr(ptr, ind, np.ones(ind.size, I)) == 0
        assert g.cc(lab, Ai, 0, desc)[0] == 0
    elif tag == "scc":
        assert g.scc(lab, A, None)[0] == 0
    else:
        assert g.matching(lab, None, A, 2, 1, None)[0] == 0
    info, nc = g.relabel(mp, lab, g.GRB_RELABEL_MATE if tag == "matching" else g.GRB_RELABEL_LABELS)
    assert info == 0
    return mp, nc


def timed_once(g, call):
    lib = g._lib.load()
    t = ctypes.c_float(0)
    assert lib.grb_timer_start() == 0
    out = call()
    assert lib.grb_timer_stop(ctypes.byref(t)) == 0
    return t.value, out


def op_by_op(g, A, mp, n, nc, loops, desc, tran):
    """the route a caller had before grb_contract; -> C (both orientations)"""
    m = mp.extractTuples()[1]                              # the labels go to the host
    v = np.flatnonzero(m >= 0).astype(I)
    S, St = g.Matrix(n, nc, F), g.Matrix(nc, n, F)
    sptr = np.zeros(n + 1, I)
    np.cumsum(m >= 0, out=sptr[1:])
    assert S.build_csr(sptr, m[v], np.ones(v.size, F)) == 0
    o = np.argsort(m[v], kind="stable")
    tptr = np.zeros(nc + 1, np.int64)
    np.cumsum(np.bincount(m[v], minlength=nc), out=tptr[1:])
    assert St.build_csr(tptr.astype(I), v[o], np.ones(v.size, F)) == 0
    T, Cm = g.Matrix(n, nc, F), g.Matrix(nc, nc, F)
    assert g.mxm(T, None, None, "PlusMultiplies", A, S, desc) == 0
    assert g.mxm(Cm, None, None, "PlusMultiplies", St, T, desc) == 0
    if not loops:
        assert g.select(Cm, None, None, "offdiag", Cm, 0, desc) == 0
    assert g.transpose(Cm, None, None, Cm, tran) == 0       # C = C under GrB_INP0 = GrB_TRAN: the CSC comes back
    return Cm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="rmat16,rmat20,drmat16,grid")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-route", action="store_true")
    a = ap.parse_args()
    import graphblast_amd as g
    if not g.device_info().startswith("gfx"):
        raise SystemExit("contract_bench needs the GPU: " + g.device_info())
    desc = g.Descriptor()
    assert desc.loadArgs() == 0
    tran = g.Descriptor()
    assert tran.loadArgs() == 0 and tran.set(g.GrB_INP0, g.GrB_TRAN) == 0
    for name in a.only.split(","):
        n, (ptr, ind, val), parts = graph(name)
        Z = int(ind.size)
        A = g.Matrix(n, n, F)
        assert A.build_csr(ptr, ind, val) == 0
        # every grb_contract call is timed before anything else runs on the device: the route's and torch's large
        # allocations, freed lazily, otherwise stand between its own (a first version measured 77 ms where 10 ms are due)
        done = []
        for tag, loops in parts:
            mp, nc = partition(g, tag, A, n, desc)
            Cm, sizes = g.Matrix(nc, nc, F), g.Vector(nc, I)

            def call():
                info, res = g.contract(Cm, sizes, A, mp, "plus", loops, None)
                assert info == 0, info
                return res

            timed_once(g, call)                            # warm
            first = [x.tobytes() for x in Cm.host_csr()]
            runs = [timed_once(g, call) for _ in range(max(1, a.reps))]
            assert [x.tobytes() for x in Cm.host_csr()] == first, (name, tag)     # the same bits every call
            ms, res = float(np.median([r[0] for r in runs])), runs[-1][1]
            cb = max(1, int(nc).bit_length())
            surv = res["kept"] - (0 if loops else res["loops"])
            digits, tdigits = (2 * cb + 7) // 8, (cb + 7) // 8
            model = 24 * Z + (32 * digits * Z + 48 * surv + (12 + 32 * tdigits) * res["entries"] if surv else 0)
            row = dict(graph=name, by=tag, loops=loops, n=n, nnz=Z, nc=nc, contract_ms=ms, loop_ms=res["loop_ms"], launches=res["launches"],
                       kept=res["kept"], loop_entries=res["loops"], entries=res["entries"], clusters=res["clusters"], largest=res["largest"],
                       model_bytes=model, floor_bytes=12 * res["kept"], bytes_over_floor=model / max(1, 12 * res["kept"]),
                       model_gbs=model / ms / 1e6)
            print(json.dumps(row), flush=True)
            csr = tuple(np.array(x) for x in Cm.host_csr())
            csc = tuple(np.array(x) for x in Cm.host_csc())
            done.append((tag, loops, mp, nc, row, csr, csc))
            del Cm, sizes
        for tag, loops, mp, nc, row, (cp, ci, cv), (xp, xi, xv) in done:
            ms = row["contract_ms"]
            if not a.no_route:
                try:
                    op_by_op(g, A, mp, n, nc, loops, desc, tran)  # warm
                    times = []
                    for _ in range(max(1, a.reps)):
                        t0 = time.perf_counter()
                        R = op_by_op(g, A, mp, n, nc, loops, desc, tran)
                        times.append(1e3 * (time.perf_counter() - t0))
                    rp, ri, rv = R.host_csr()
                    assert np.array_equal(rp, cp) and np.array_equal(ri, ci), (name, tag, "structure")
                    small = np.abs(cv.astype(np.float64)) < 2.0 ** 24
                    assert np.array_equal(rv[small], cv[small]), (name, tag, "values")
                    yp, yi, yv = R.host_csc()
                    assert np.array_equal(xp, yp) and np.array_equal(xi, yi) and np.array_equal(xv[np.abs(xv) < 2.0 ** 24], yv[np.abs(xv) < 2.0 ** 24])
                    row.update(route_ms=float(np.median(times)), route_over_contract=float(np.median(times)) / ms, equal_to_route=True,
                               entries_past_2_24=int((~small).sum()))
                    del R
                except AssertionError as e:
                    if e.args and isinstance(e.args[0], tuple):
                        raise
                    row.update(route_ms=None, route_error=repr(e))
            if not a.no_torch:
                import torch
                mh = mp.extractTuples()[1].astype(np.int64)
                rows = np.repeat(np.arange(n), np.diff(ptr))
                ra, rb = mh[rows], mh[ind]
                keep = (ra >= 0) & (rb >= 0) & ((ra != rb) | bool(loops))
                dev = torch.device("cuda")
                idx = torch.from_numpy(np.stack([ra[keep], rb[keep]])).to(dev)
                vals = torch.from_numpy(val[keep]).to(dev)
                times = []
                for k in range(max(1, a.reps) + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    out = torch.sparse_coo_tensor(idx, vals, (nc, nc)).coalesce()
                    e1.record()
                    torch.cuda.synchronize()
                    if k:
                        times.append(e0.elapsed_time(e1))
                assert out._nnz() == row["entries"], (name, tag, "torch")
                row.update(torch_ms=float(np.median(times)), torch_over_contract=float(np.median(times)) / ms)
                del idx, vals, out
            print(json.dumps(row), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
