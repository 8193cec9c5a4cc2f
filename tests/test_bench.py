"""bench.py's plain run and --dump-outputs: the files hold what the last timed step computed (checked against the
oracle's SimpleReferenceBfs restatement on the same seeded graph), and a larger label vector is sampled at fixed
seeded vertices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_samples_a_large_label_vector_at_fixed_vertices(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_VERTICES", 1000)
    depth = np.arange(5000, dtype=np.int32)
    last = {"reached": 4999, "edges_traversed": 123456789012, "levels": 7}
    ids = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), depth, last)
        got = np.load(tmp_path / d / "bfs_depth.npy")
        ids.append(np.load(tmp_path / d / "bfs_depth_vertices.npy"))
        assert got.dtype == np.float32 and got.size == 1000 and ids[-1].dtype == np.float64
        assert np.array_equal(got, ids[-1]) and np.all(np.diff(ids[-1]) > 0)
        step = np.load(tmp_path / d / "bfs_last_step.npy")
        assert step.dtype == np.float64 and step.tolist() == [4999, 123456789012, 7]
    assert np.array_equal(ids[0], ids[1])


class _Ring:
    """grb_bfs_fused_enqueue / grb_bfs_wait as the library keeps them: 256 tickets at most (GRB_INSUFFICIENT_SPACE = 11
    beyond), a vector untouched until its ticket has been waited for, tickets waited for once."""

    def __init__(self):
        self.out, self.next, self.calls = {}, 0, []

    def bfs_enqueue(self, v, A, s, desc):
        self.calls.append("q")
        if len(self.out) == 256:
            return 11, None
        assert all(v is not w for w, _ in self.out.values()), "a vector queued again before its ticket was waited for"
        self.next += 1
        self.out[self.next] = (v, s)
        return 0, self.next

    def bfs_wait(self, t):
        self.calls.append("w")
        v, s = self.out.pop(t)
        return 0, {"source": s}


@pytest.mark.parametrize("steps", [1, 20, 256, 257, 1000])
def test_queued_steps_stay_within_the_ticket_ring(steps):
    import bench
    ring = _Ring()
    vecs = [object() for _ in range(min(steps, bench.QUEUE_DEPTH))]
    srcs = [i % 64 for i in range(steps)]
    stamps = []
    res = bench.queue_bfs(ring, vecs, None, srcs, None, stamps)
    assert [r["source"] for r in res] == srcs and len(stamps) == steps and not ring.out
    if steps <= bench.QUEUE_DEPTH:                          # all queued before the first wait, as the timed region always did
        assert ring.calls == ["q"] * steps + ["w"] * steps


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_last_one(tmp_path):
    import torch
    from graphblast_amd.graphgen import rmat_edges, finalize_edges, random_sources
    from oracle import simple_reference as sr
    steps, scale = 300, 14                                  # more steps than tickets may be outstanding
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "2",
                          "--scale", str(scale), "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["value"] > 0 and line["ms_per_step"] > 0 and line["unit"] == "TEPS"
    assert line["roofline"] is None and "cpu_baseline" not in line and "blocking_loop" not in line
    assert sorted(os.listdir(tmp_path)) == ["bfs_depth.npy", "bfs_last_step.npy"]
    # the bench's input, generated the same way (seeded, on the device)
    s, d, n = rmat_edges(scale, 16, seed=1, device=torch.device("cuda", 0))
    ptr, ind = (x.cpu().numpy() for x in finalize_edges(s, d, n, symmetrize=True)["csr"])
    deg = np.diff(ptr)
    sources = [int(np.argmax(deg))] + random_sources(ptr, 63, seed=0)
    src = sources[(steps - 1) % len(sources)]
    want = sr.bfs(ptr, ind, src)[0]
    depth = np.load(tmp_path / "bfs_depth.npy")
    assert depth.dtype == np.float32 and np.array_equal(depth, want)
    reached, edges, levels = np.load(tmp_path / "bfs_last_step.npy").tolist()
    assert (reached, edges) == (np.count_nonzero(want), deg[want != 0].sum())
    import graphblast_amd as g
    A = g.Matrix(n, n)
    assert A.build_csr(ptr, ind, np.ones(ind.size, dtype=np.float32)) == 0
    desc = g.Descriptor()
    assert desc.loadArgs(mxvmode=0, struconly=1, opreuse=1, earlyexit=1, edgeswitch=0.08) == 0
    info, res = g.bfs(g.Vector(n), A, src, desc, fused=True)
    assert info == 0 and (res["reached"], res["edges_traversed"], res["levels"]) == (reached, edges, levels)
