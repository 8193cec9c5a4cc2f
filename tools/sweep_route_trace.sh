#!/bin/sh
# Kernel trace of a ROUTED sweep of K queued traversals on RMAT-22 (the queue's route, grb_bfs_set_sweep_from(2)):
#   tools/sweep_route_trace.sh K [out-dir]
# One rocprofv3 --kernel-trace run over tools/bfs_sweep_route_bench.py 22 K, nothing else traced; the table of the last
# sweep (tools/sweep_trace_table.py) goes to <out-dir>/sweep_trace_k<K>.txt and to the terminal.
set -e
K=${1:-32}
root=$(cd "$(dirname "$0")/.." && pwd)
out=${2:-$root/profiles/trace}
mkdir -p "$out"
tmp=$(mktemp -d)
trap 'rm -rf "$tmp"' EXIT
cd "$root"
timeout -k 10 240 rocprofv3 --kernel-trace --output-format csv -d "$tmp/kt" -o b -- python tools/bfs_sweep_route_bench.py 22 "$K" > "$out/sweep_trace_k$K.log" 2>&1
f=$(find "$tmp/kt" -name "b_kernel_trace.csv" | head -1)
[ -n "$f" ] && [ -s "$f" ] || { echo "no kernel trace was written: see $out/sweep_trace_k$K.log" >&2; exit 1; }
python tools/sweep_trace_table.py "$f" | tee "$out/sweep_trace_k$K.txt"
