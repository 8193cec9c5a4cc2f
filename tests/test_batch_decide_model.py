"""The sweep's direction rule (graphblast_amd/csrc/batch_decide.hpp) against a restatement of the serial rule it
replaced: sort the live sources by mf descending (source index ascending among equals), sum the out-edges of those under
the switch point, walk the order and pull while that running sum is over the budget.  The header is compiled by the host
compiler alone -- it must not need HIP -- into a small driver that reads cases and prints decisions."""
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
    const grb::BatchDecision d = grb::batch_decide(nf, mf, r, left != 0);
    // the per-source form and the whole must agree
    unsigned long long under = 0;
    for (int s = 0; s < 64; ++s) if (grb::batch_decide_under(nf, s, r)) under |= 1ull << s;
    for (int s = 0; s < 64; ++s) {
      const int w = grb::batch_decide_source(nf, mf, s, r, under);
      if (((d.qmask >> s) & 1ull) != (unsigned long long)(w == 2) || ((d.pmask >> s) & 1ull) != (unsigned long long)(w == 1)) return 3;
    }
    printf("%llu %llu %.17g %d\n", d.qmask, d.pmask, d.pushed_edges, d.kind);
  }
  return 0;
}
"""

DONE, LIGHT, HOST = 0, 1, 2
PUSHPULL, PUSHONLY, PULLONLY = 0, 1, 2


def serial_rule(nf, mf, k, n, nvals, mode, sw, budget, tail, left):
    live = [s for s in range(k) if nf[s] > 0]
    q = p = 0
    if mode == PULLONLY:
        for s in live:
            q |= 1 << s
    elif mode == PUSHONLY:
        for s in live:
            p |= 1 << s
    else:
        order = sorted(live, key=lambda s: (-mf[s], s))
        point = float(np.float32(sw)) * float(n)
        pushed = 0.0
        for s in order:
            if float(nf[s]) <= point:
                pushed += float(mf[s])
        for s in order:
            pull = float(nf[s]) > point
            if not pull and pushed > budget * float(nvals):
                pull = True
                pushed -= float(mf[s])
            if pull:
                q |= 1 << s
            else:
                p |= 1 << s
    pe = 0.0
    for s in range(k):
        if (p >> s) & 1:
            pe += float(mf[s])
    if not live or not left:
        kind = DONE
    elif tail > 0 and q == 0 and p != 0 and pe <= tail:
        kind = LIGHT
    else:
        kind = HOST
    return q, p, pe, kind


def make_cases():
    rng = random.Random(7)
    cases = []
    for i in range(4000):
        k = rng.choice([1, 2, 3, 20, 33, 63, 64]) if i % 3 else rng.randint(1, 64)
        n = rng.choice([3, 1000, 8193, 1 << 22])
        nvals = 4 * rng.choice([1, 25, 1000, 1 << 20, 1 << 25])
        mode = rng.choice([PUSHPULL, PUSHPULL, PUSHPULL, PUSHONLY, PULLONLY])
        sw = rng.choice([0.01, 0.08, 0.5, 2.0])
        budget = rng.choice([0.15, 0.25, 0.0, 1.0])
        left = 0 if rng.random() < 0.1 else 1
        point = float(np.float32(sw)) * n
        nf, mf = [], []
        small = rng.random() < 0.5                           # few distinct mf values: ties
        for s in range(k):
            r = rng.random()
            if r < 0.2:
                nf.append(0)                                 # a dead source (its mf may still be anything)
                mf.append(rng.choice([0, 5]))
                continue
            # at, below and above the switch point
            nf.append(max(1, int(point) + rng.choice([-1, 0, 1, 2])) if r < 0.5 else rng.randint(1, max(1, n)))
            mf.append(rng.choice([0, 1, 2, 3]) * max(1, nvals // 16) if small else rng.randint(0, max(1, nvals // max(1, k // 2))))
        if i % 4 == 0 and budget in (0.25, 0.15):
            # the out-edges under the switch point cross the budget exactly: equal to it, one above, one below
            under = [s for s in range(k) if 0 < nf[s] <= point]
            if under:
                want = int(budget * nvals) + rng.choice([-1, 0, 1])
                rest = sum(mf[s] for s in under[1:])
                if want - rest >= 0:
                    mf[under[0]] = want - rest
        pushable = sum(mf[s] for s in range(k) if nf[s] > 0)
        tail = rng.choice([0, 64, 1048576, pushable, pushable + 1, max(0, pushable - 1)])   # the light limit at, above, below
        cases.append((nf, mf, k, n, nvals, mode, sw, budget, float(tail), left))
    return cases


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("decide")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    return str(exe)


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "batch_decide.hpp")).read()
    assert "#include" not in text


def test_decide_matches_serial_rule(driver):
    cases = make_cases()
    lines = []
    for nf, mf, k, n, nvals, mode, sw, budget, tail, left in cases:
        lines.append("%d %d %d %d %.9g %.17g %.17g %d" % (k, n, nvals, mode, float(np.float32(sw)), budget, tail, left))
        lines.append(" ".join("%d %d" % (nf[s], mf[s]) for s in range(k)))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    kinds = [0, 0, 0]
    pulled_by_budget = 0
    for i, c in enumerate(cases):
        q, p, pe, kind = out[i].split()
        want = serial_rule(*c)
        got = (int(q), int(p), float(pe), int(kind))
        assert got == want, (i, c, got, want)
        kinds[want[3]] += 1
        point = float(np.float32(c[6])) * c[3]
        pulled_by_budget += any((want[0] >> s) & 1 and c[0][s] <= point for s in range(c[2])) and c[5] == PUSHPULL
    assert min(kinds) > 50 and pulled_by_budget > 50, (kinds, pulled_by_budget)   # the cases reach every branch
