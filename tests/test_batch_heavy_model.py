"""The sweep's heavy-level rule and its stash (graphblast_amd/csrc/batch_decide.hpp, bfs_batch.hip).

A host level is heavy when the pushed sources bring more out-edges than half the vertices.  The totals kernel decides it
from the INTEGER sum of the pushed sources' out-degrees, the host (the sweep's first level, the level after a light-level
hand-back) from a sum of doubles: the header's one predicate must give both the same answer, on either side of 0.5 n by
one.  The header is compiled by the host compiler alone into a small driver; the same driver is built once more with
-fsanitize=address,undefined and run as a program of its own.

On a heavy level the pull pass stores `newb | (seen & P)` into the level's words, the push kernels claim in `seen` alone,
and the commit pass computes old = w & P, pb = seen & P & ~old, w' = (w & ~P) | pb.  A numpy model of the three steps
must return exactly seen_after & ~seen_before & P as the pushed discoveries and leave no P bit that is not one."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphblast_amd", "csrc")

DRIVER = r"""
#include "batch_decide.hpp"
#include <cstdio>
int main() {
  grb::BatchRule r; int left; double sw;
  while (scanf("%d %lld %lld %d %lf %lf %lf %d", &r.k, &r.n, &r.nvals, &r.mode, &sw, &r.budget, &r.tail_limit, &left) == 8) {
    unsigned long long nf[64] = {0}, mf[64] = {0};
    r.switchpoint = (float)sw;
    for (int s = 0; s < r.k; ++s) if (scanf("%llu %llu", &nf[s], &mf[s]) != 2) return 2;
    // the host's way: batch_decide sums doubles
    const grb::BatchDecision d = grb::batch_decide(nf, mf, r, left != 0);
    // the totals kernel's way: the masks per source, the pushed out-edges as an integer sum, turned into a double once
    unsigned long long under = 0, q = 0, p = 0, pushed = 0;
    for (int s = 0; s < 64; ++s) if (grb::batch_decide_under(nf, s, r)) under |= 1ull << s;
    for (int s = 0; s < 64; ++s) {
      const int w = grb::batch_decide_source(nf, mf, s, r, under);
      if (w == 2) q |= 1ull << s;
      if (w == 1) { p |= 1ull << s; pushed += mf[s]; }
    }
    const int kind = grb::batch_decide_kind(q, p, (double)pushed, r, left != 0);
    const unsigned long long stash = grb::batch_decide_stash(p, (double)pushed, r.n, kind);
    if (q != d.qmask || p != d.pmask || kind != d.kind) return 3;
    printf("%llu %llu %d %llu %llu %llu %d\n", d.qmask, d.pmask, d.kind, d.stash, stash, pushed,
           (int)grb::batch_decide_heavy((double)pushed, r.n));
  }
  return 0;
}
"""

HOST = 2
PUSHPULL, PUSHONLY = 0, 1


def make_cases():
    rng = random.Random(13)
    cases = []
    for i in range(3000):
        k = rng.choice([1, 2, 3, 20, 33, 63, 64])
        n = rng.choice([3, 4, 1000, 8193, 32769, 1 << 22, (1 << 22) + 1])
        nvals = 4 * rng.choice([25, 1000, 1 << 20, 1 << 25])
        mode = rng.choice([PUSHPULL, PUSHPULL, PUSHONLY])
        sw = rng.choice([0.01, 0.08, 2.0])
        budget = rng.choice([0.15, 1.0, 64.0])
        left = 0 if rng.random() < 0.05 else 1
        tail = rng.choice([0, 64, 1048576])
        nf = [0 if rng.random() < 0.2 else rng.randint(1, max(1, n // 200)) for _ in range(k)]
        mf = [rng.randint(0, max(1, n // k)) for _ in range(k)]
        live = [s for s in range(k) if nf[s] > 0]
        if live and i % 2 == 0:
            # the pushed sum lands on 0.5 n exactly (n even), one below, one above: the first live source takes the rest
            want = n // 2 + rng.choice([-1, 0, 1])
            rest = sum(mf[s] for s in live[1:])
            if want - rest >= 0:
                mf[live[0]] = want - rest
        cases.append((nf, mf, k, n, nvals, mode, sw, budget, float(tail), left))
    return cases


def build(tmp, flags, name):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    src = tmp / "driver.cpp"
    src.write_text(DRIVER)
    exe = tmp / name
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC] + flags + [str(src), "-o", str(exe)])
    return str(exe)


def run(driver, cases):
    lines = []
    for nf, mf, k, n, nvals, mode, sw, budget, tail, left in cases:
        lines.append("%d %d %d %d %.9g %.17g %.17g %d" % (k, n, nvals, mode, float(np.float32(sw)), budget, tail, left))
        lines.append(" ".join("%d %d" % (nf[s], mf[s]) for s in range(k)))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    rows = [[int(x) for x in line.split()] for line in out.stdout.split("\n") if line]
    assert len(rows) == len(cases)
    return rows


def check(rows, cases):
    heavy_n = light_n = edge = 0
    for (q, p, kind, stash_host, stash_dev, pushed, heavy), c in zip(rows, cases):
        nf, mf, k, n = c[0], c[1], c[2], c[3]
        assert pushed == sum(mf[s] for s in range(k) if (p >> s) & 1)
        assert heavy == (2 * pushed > n), (c, pushed)                  # pushed > 0.5 n, in integers
        want = p if (kind == HOST and p and 2 * pushed > n) else 0
        assert stash_host == want and stash_dev == want, (c, stash_host, stash_dev, want)
        heavy_n += want != 0
        light_n += want == 0 and kind == HOST and p != 0
        edge += abs(2 * pushed - n) <= 2 and p != 0
    assert heavy_n > 100 and light_n > 100 and edge > 100, (heavy_n, light_n, edge)   # both sides, and the boundary


def test_heavy_from_integer_sum_equals_host_double_sum(tmp_path):
    cases = make_cases()
    check(run(build(tmp_path, [], "driver"), cases), cases)


def test_driver_under_address_and_undefined_sanitizers(tmp_path):
    """the same driver as a stand-alone program built with the sanitizers: no report, the same answers"""
    cases = make_cases()[:600]
    exe = build(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "driver_san")
    check_rows = run(exe, cases)
    plain = run(build(tmp_path, [], "driver"), cases)
    assert check_rows == plain


def stash_then_commit(seen_before, pull_new, push_claims, P, Q):
    """the three device steps on whole arrays: -> (the level's words after the commit, the pushed discoveries it counts,
    seen after the level)"""
    assert not (P & Q)
    Pm, Qm = np.uint64(P), np.uint64(Q)
    newb = pull_new & Qm & ~seen_before                                  # batch_pull_kernel: need = ~seen & qmask
    w = newb | (seen_before & Pm)                                       # ... fnext[v] = newb | (seen[v] & stash)
    seen = seen_before | newb
    seen = seen | (push_claims & Pm)                                    # the push kernels: atomicOr into seen, nothing else
    old = w & Pm                                                        # batch_push_commit_kernel
    pb = seen & Pm & ~old
    store = (old | pb) != 0
    w = np.where(store, (w & ~Pm) | pb, w)
    return w, pb, seen


@pytest.mark.parametrize("k", [2, 24, 33, 64])
def test_stash_then_commit_model(k):
    rng = np.random.default_rng(k)
    n = 4099
    full = (1 << k) - 1
    for trial in range(40):
        P = int(rng.integers(0, 1 << 62)) & full if trial % 5 else full     # Q == 0: every live source pushed
        if trial % 7 == 0:
            P |= 1 << (k - 1)                                               # the top column (bit 63 at k = 64)
        Q = int(rng.integers(0, 1 << 62)) & full & ~P if trial % 5 else 0

        def bits64():
            return rng.integers(0, 1 << 32, n, dtype=np.uint64) << np.uint64(32) | rng.integers(0, 1 << 32, n, dtype=np.uint64)

        def rnd(sparse):                                                    # half, or an eighth, of the k columns' bits set
            return bits64() & (bits64() & bits64() if sparse else ~np.uint64(0)) & np.uint64(full)

        seen_before = rnd(trial % 2)
        pull_new, claims = rnd(1), rnd(trial % 3 == 0)
        w, pb, seen_after = stash_then_commit(seen_before, pull_new, claims, P, Q)
        Pm, Qm = np.uint64(P), np.uint64(Q)
        assert np.array_equal(pb, seen_after & ~seen_before & Pm)
        assert np.array_equal(w & Pm, pb)                                   # no P bit left that is not a discovery
        assert np.array_equal(w, seen_after & ~seen_before)                 # the words ARE the level's discoveries
        assert not np.any(w & ~(Pm | Qm))
