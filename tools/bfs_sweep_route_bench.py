"""The queue's two ways of running K gathered traversals, side by side (docs/experiments.md R8.1):
python tools/bfs_sweep_route_bench.py [scale] [Ks, e.g. 2,4,8,12,16,20,24,32,48]
RMAT-<scale> with bench.py's 64 sources; for each K the K traversals are queued and waited for, once through the
co-scheduled launch (grb_bfs_set_sweep_from(0)) and once through the routed sweep (grb_bfs_set_sweep_from(2)), five
timed repetitions each after a warm-up: median (min-max) ms per traversal.  Every vector's labels and result blocks are
compared between the two."""
import sys, os, time, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import graphblast_amd as g
from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
dev = torch.device("cuda", 0)
scale = int(sys.argv[1]) if len(sys.argv) > 1 else 22
Ks = [int(x) for x in sys.argv[2].split(",")] if len(sys.argv) > 2 else [2, 4, 8, 12, 16, 20, 24, 32, 48]
s_, d_, n = rmat_edges(scale, 16, seed=1, device=dev)
gr = finalize_edges(s_, d_, n, symmetrize=True)
tptr, tind = gr["csr"]; nnz = gr["nnz"]
tval = torch.ones(nnz, dtype=torch.float32, device=dev)
A = g.Matrix(n, n)
assert A.build_device_csr(tptr.data_ptr(), tind.data_ptr(), tval.data_ptr(), nnz, tptr.data_ptr(), tind.data_ptr(), tval.data_ptr(), keep=(tptr, tind, tval)) == 0
ptr = tptr.cpu().numpy()
srcs = [int(np.argmax(np.diff(ptr)))] + random_sources(ptr, 63, seed=0)
desc = g.Descriptor(); desc.loadArgs(mxvmode=0, struconly=1, opreuse=1, earlyexit=1, edgeswitch=0.08)
vs = [g.Vector(n) for _ in range(max(Ks))]
v0 = g.Vector(n)
assert g.bfs(v0, A, srcs[0], desc, fused=True)[0] == 0      # the matrix's once-only preparation
kstar = g.bfs_set_sweep_from(-1)
def run(K):
    ts = [g.bfs_enqueue(vs[i], A, srcs[i % 64], desc)[1] for i in range(K)]
    return [g.bfs_wait(t)[1] for t in ts]
def timed(K, reps=5):
    run(K)
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        res = run(K)
        torch.cuda.synchronize(); out.append((time.perf_counter() - t0) / K * 1e3)
    return out, res
for K in Ks:
    row = {"K": K}
    got = {}
    for name, frm in (("coscheduled", 0), ("sweep", 2)):
        g.bfs_set_sweep_from(frm)
        c0 = g.bfs_sweep_counts()["sweeps"]
        ms, res = timed(K)
        swept = g.bfs_sweep_counts()["sweeps"] - c0
        assert swept == (6 if frm else 0), (name, K, swept)
        got[name] = ([(r["reached"], r["edges_traversed"], r["levels"]) for r in res], [v.extractTuples()[1] for v in vs[:K]])
        row[name] = {"median": round(float(np.median(ms)), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}
    assert got["coscheduled"][0] == got["sweep"][0], "result blocks differ between the two routes"
    assert all(np.array_equal(a, b) for a, b in zip(got["coscheduled"][1], got["sweep"][1])), "labels differ between the two routes"
    row["sweep_wins"] = row["sweep"]["max"] < row["coscheduled"]["min"]
    row["labels"] = "equal (all %d vectors)" % K
    print(json.dumps(row), flush=True)
g.bfs_set_sweep_from(kstar)
