#!/usr/bin/env python
"""The sweep's levels on the CPU, decided by csrc/batch_decide.hpp (tools/batch_rule_model.cpp): no GPU needed.

    python tools/batch_rule_model.py SCALE K [--seed S] [--symmetrize] [--finish-limit X] [--tail-edges E] [--switchpoint P]

RMAT-SCALE with edge factor 16 from graphgen.py's CPU generator, the sources chosen as bench.py chooses them (the
maximum-degree vertex, then random_sources(ptr, 63, seed=0)), the first K of them.  --finish-limit -1 is the rule off.
The lines it prints name the same masks and the same U as the library's GRB_BATCH_TRACE lines for the same graph."""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_model():
    exe = os.path.join(ROOT, "build", "batch_rule_model")
    src = os.path.join(ROOT, "tools", "batch_rule_model.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["c++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "graphblast_amd", "csrc"), src, "-o", exe])
    return exe


def write_graph(path, csr, csc, sources):
    with open(path, "wb") as f:
        np.asarray([csr[0].size - 1, csr[1].size, len(sources)], dtype=np.int64).tofile(f)
        np.asarray(sources, dtype=np.int32).tofile(f)
        for a in (csr[0], csr[1], csc[0], csc[1]):
            np.asarray(a, dtype=np.int32).tofile(f)


def run_model(csr, csc, sources, switchpoint=0.01, budget=0.15, finish_limit=0.01, tail_edges=1048576, max_niter=1 << 30):
    """the model's output lines for one sweep"""
    exe = build_model()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "graph.bin")
        write_graph(path, csr, csc, sources)
        return subprocess.run([exe, path, repr(switchpoint), repr(budget), repr(finish_limit), repr(float(tail_edges)), str(max_niter)],
                              capture_output=True, text=True, check=True).stdout.splitlines()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("scale", type=int)
    ap.add_argument("k", type=int)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--symmetrize", action="store_true")
    ap.add_argument("--finish-limit", type=float, default=0.01)
    ap.add_argument("--tail-edges", type=float, default=1048576)
    ap.add_argument("--switchpoint", type=float, default=0.01)
    ap.add_argument("--budget", type=float, default=0.15)
    args = ap.parse_args()
    from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
    s, d, n = rmat_edges(args.scale, 16, seed=args.seed)
    gr = finalize_edges(np.asarray(s), np.asarray(d), n, symmetrize=args.symmetrize)
    ptr = np.asarray(gr["csr"][0])
    sources = ([int(np.argmax(np.diff(ptr)))] + random_sources(ptr, 63, seed=0))[:args.k]
    print("n %d nvals %d k %d" % (n, gr["nnz"], len(sources)))
    for line in run_model(gr["csr"], gr["csc"], sources, args.switchpoint, args.budget, args.finish_limit, args.tail_edges):
        print(line)


if __name__ == "__main__":
    main()
