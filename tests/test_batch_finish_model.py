"""The sweep's finishing rule (graphblast_amd/csrc/batch_decide.hpp, batch_decide_finish) against a Python restatement.
After the per-source decisions: push-pull mode, somebody pulled, somebody pushed, U (the in-edges the level before left
open) known and complete, U <= finish_limit * nvals -- then every pushed source is pulled as well, and kind and stash are
computed from the result.  U unknown, the rule switched off, or BatchRule's new field left alone: the base rule, bit for
bit.  The header is compiled by the host compiler alone into a driver that reads cases and prints decisions; the same
driver is built once more with -fsanitize=address,undefined and run as a program of its own."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from test_batch_decide_model import serial_rule, DONE, LIGHT, HOST, PUSHPULL, PUSHONLY, PULLONLY

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphblast_amd", "csrc")

# per case: the rule, the sources, then four decisions -- the old call (no U argument, the new field as the struct leaves
# it), U unknown with the field set, the full call, and the full call again from the device's pieces (the per-source
# form, batch_decide_finish, batch_decide_kind, batch_decide_stash), which must agree with it
DRIVER = r"""
#include "batch_decide.hpp"
#include <cstdio>
static void show(const grb::BatchDecision& d) { printf("%llu %llu %.17g %d %llu\n", d.qmask, d.pmask, d.pushed_edges, d.kind, d.stash); }
int main() {
  int k, mode, left; long long n, nvals, open_u; double sw, budget, tail, limit;
  while (scanf("%d %lld %lld %d %lf %lf %lf %d %lf %lld", &k, &n, &nvals, &mode, &sw, &budget, &tail, &left, &limit, &open_u) == 10) {
    unsigned long long nf[64] = {0}, mf[64] = {0};
    for (int s = 0; s < k; ++s) if (scanf("%llu %llu", &nf[s], &mf[s]) != 2) return 2;
    grb::BatchRule old;                                     // as tests/test_batch_decide_model.py fills it: the new field untouched
    old.k = k; old.n = n; old.nvals = nvals; old.mode = mode; old.switchpoint = (float)sw; old.budget = budget; old.tail_limit = tail;
    show(grb::batch_decide(nf, mf, old, left != 0));
    if (old.finish_limit >= 0) return 4;                    // the default means "off"
    show(grb::batch_decide(nf, mf, old, left != 0, open_u));
    grb::BatchRule r = old;
    r.finish_limit = limit;
    show(grb::batch_decide(nf, mf, r, left != 0));
    const grb::BatchDecision d = grb::batch_decide(nf, mf, r, left != 0, open_u);
    show(d);
    unsigned long long under = 0, q = 0, p = 0, pushed = 0;
    for (int s = 0; s < 64; ++s) if (grb::batch_decide_under(nf, s, r)) under |= 1ull << s;
    for (int s = 0; s < 64; ++s) {
      const int w = grb::batch_decide_source(nf, mf, s, r, under);
      if (w == 2) q |= 1ull << s;
      if (w == 1) { p |= 1ull << s; pushed += mf[s]; }
    }
    if (grb::batch_decide_finish(q, p, r, open_u)) { q |= p; p = 0; pushed = 0; }
    const int kind = grb::batch_decide_kind(q, p, (double)pushed, r, left != 0);
    if (q != d.qmask || p != d.pmask || kind != d.kind || grb::batch_decide_stash(p, (double)pushed, n, kind) != d.stash) return 3;
  }
  return 0;
}
"""


def finish_rule(nf, mf, k, n, nvals, mode, sw, budget, tail, left, limit, open_u):
    """(q, p, pushed edges, kind, stash) with the finishing rule on top of the serial restatement of the base rule"""
    q, p, pe, _ = serial_rule(nf, mf, k, n, nvals, mode, sw, budget, tail, left)
    if mode == PUSHPULL and q != 0 and p != 0 and open_u >= 0 and limit >= 0 and float(open_u) <= limit * float(nvals):
        q, p, pe = q | p, 0, 0.0
    if not left or (q | p) == 0:
        kind = DONE
    elif tail > 0 and q == 0 and pe <= tail:
        kind = LIGHT
    else:
        kind = HOST
    stash = p if kind == HOST and p != 0 and pe > 0.5 * float(n) else 0
    return q, p, pe, kind, stash


def make_cases():
    rng = random.Random(14)
    cases = []
    for i in range(5000):
        k = (1, 64, 2, 20, 33)[i % 5] if i % 2 else rng.randint(1, 64)
        n = rng.choice([3, 1000, 8193, 1 << 22])
        nvals = 4 * rng.choice([1, 25, 1000, 1 << 20, 1 << 25])
        mode = rng.choice([PUSHPULL, PUSHPULL, PUSHPULL, PUSHPULL, PUSHONLY, PULLONLY])
        sw = rng.choice([0.01, 0.08, 0.5])
        budget = rng.choice([0.15, 0.25, 0.0, 1.0])
        left = 0 if rng.random() < 0.1 else 1
        point = float(np.float32(sw)) * n
        nf, mf = [], []
        shape = rng.random()                                 # everybody over the point (base p = 0), everybody under it (base q = 0), a mix
        for s in range(k):
            if rng.random() < 0.15:
                nf.append(0)
                mf.append(rng.choice([0, 5]))
                continue
            over = shape < 0.2 or (shape >= 0.4 and rng.random() < 0.5)
            nf.append(int(point) + 1 + rng.randint(0, 3) if over else max(1, min(int(point), rng.randint(1, 4))))
            mf.append(rng.randint(0, max(1, nvals // max(1, 4 * k))))
        limit = rng.choice([0.01, 0.01, 0.002, 0.05, 0.0, -1.0, 1.0])
        at = int(limit * nvals) if limit > 0 else 0          # the largest integer U the limit admits is floor(limit * nvals)
        while float(at + 1) <= limit * float(nvals):
            at += 1
        while at > 0 and float(at) > limit * float(nvals):
            at -= 1
        r = rng.random()
        # unknown (the level before pushed something, was the first, or ran in the light-level launch), equal to the
        # limit, one above it, anything
        open_u = -1 if r < 0.25 else at if r < 0.45 else at + 1 if r < 0.65 else rng.randint(0, nvals)
        pushable = sum(mf[s] for s in range(k) if nf[s] > 0)
        tail = rng.choice([0, 64, 1048576, pushable, pushable + 1])
        cases.append((nf, mf, k, n, nvals, mode, sw, budget, float(tail), left, limit, open_u))
    return cases


def compile_driver(d, flags):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    src = d / "finish_driver.cpp"
    src.write_text(DRIVER)
    exe = d / ("finish_driver" + ("_san" if flags else ""))
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-I" + CSRC] + flags + [str(src), "-o", str(exe)])
    return str(exe)


def case_text(cases):
    lines = []
    for nf, mf, k, n, nvals, mode, sw, budget, tail, left, limit, open_u in cases:
        lines.append("%d %d %d %d %.9g %.17g %.17g %d %.17g %d" % (k, n, nvals, mode, float(np.float32(sw)), budget, tail, left, limit, open_u))
        lines.append(" ".join("%d %d" % (nf[s], mf[s]) for s in range(k)))
    return "\n".join(lines) + "\n"


@pytest.fixture(scope="module")
def cases():
    return make_cases()


def parse(line):
    q, p, pe, kind, stash = line.split()
    return int(q), int(p), float(pe), int(kind), int(stash)


def test_finish_rule_matches_restatement(tmp_path, cases):
    exe = compile_driver(tmp_path, [])
    out = subprocess.run([exe], input=case_text(cases), capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(out) >= 4 * len(cases)
    seen = dict(fired=0, unknown=0, base_q0=0, base_p0=0, at_limit=0, over_limit=0, pushonly=0, pullonly=0, no_left=0, k1=0, k64=0, off=0,
                fired_stash_gone=0)
    for i, c in enumerate(cases):
        nf, mf, k, n, nvals, mode, sw, budget, tail, left, limit, open_u = c
        old, unknown_field, unknown_u, full = [parse(out[4 * i + j]) for j in range(4)]
        base = finish_rule(nf, mf, k, n, nvals, mode, sw, budget, tail, left, -1.0, -1)
        want = finish_rule(*c)
        # the old call, the field left at its default, and U unknown: the base rule, bit for bit
        assert old == base and unknown_field == base and unknown_u == base, (i, c, old, unknown_field, unknown_u, base)
        assert base[:4] == serial_rule(nf, mf, k, n, nvals, mode, sw, budget, tail, left)
        assert full == want, (i, c, full, want)
        fired = want != base
        if fired:
            assert want[1] == 0 and want[2] == 0.0 and want[4] == 0 and want[0] == base[0] | base[1] and want[3] == (HOST if left else DONE), (i, want, base)
            assert mode == PUSHPULL and base[0] and base[1] and 0 <= open_u and float(open_u) <= limit * float(nvals)
        seen["fired"] += fired
        seen["fired_stash_gone"] += fired and base[4] != 0
        seen["unknown"] += open_u < 0 and mode == PUSHPULL and base[0] != 0 and base[1] != 0 and limit > 0
        seen["off"] += limit < 0 and open_u == 0 and base[0] != 0 and base[1] != 0
        seen["base_q0"] += base[0] == 0 and base[1] != 0 and open_u == 0 and limit > 0 and mode == PUSHPULL
        seen["base_p0"] += base[1] == 0 and base[0] != 0 and open_u == 0 and limit > 0 and mode == PUSHPULL
        live_mix = mode == PUSHPULL and base[0] != 0 and base[1] != 0 and limit > 0
        if live_mix and open_u >= 0 and float(open_u) <= limit * float(nvals) < float(open_u + 1):
            seen["at_limit"] += 1
            assert fired, (i, c)
        if live_mix and open_u >= 1 and float(open_u - 1) <= limit * float(nvals) < float(open_u):
            seen["over_limit"] += 1
            assert not fired, (i, c)
        seen["pushonly"] += mode == PUSHONLY and open_u == 0 and limit > 0
        seen["pullonly"] += mode == PULLONLY and open_u == 0 and limit > 0
        seen["no_left"] += (not left) and open_u >= 0 and limit > 0
        seen["k1"] += k == 1
        seen["k64"] += k == 64 and fired
    assert min(seen.values()) >= 5, seen                     # the cases reach every branch


def test_nothing_changes_while_the_rule_cannot_fire(cases):
    """the restatement itself: outside push-pull mode, without an iteration left, with one source, the decision is the base rule's"""
    for c in cases:
        nf, mf, k, n, nvals, mode, sw, budget, tail, left, limit, open_u = c
        if mode != PUSHPULL or k == 1 or limit < 0 or open_u < 0:
            assert finish_rule(*c) == finish_rule(nf, mf, k, n, nvals, mode, sw, budget, tail, left, -1.0, -1), c
        if not left:
            assert finish_rule(*c)[3] == DONE


def test_driver_under_sanitizers(tmp_path, cases):
    """the same driver with AddressSanitizer and UndefinedBehaviorSanitizer, a program of its own, on the same cases"""
    exe = compile_driver(tmp_path, ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    plain = compile_driver(tmp_path, [])
    text = case_text(cases)
    a = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert a.returncode == 0, a.stderr[-2000:]
    b = subprocess.run([plain], input=text, capture_output=True, text=True, check=True)
    assert a.stdout == b.stdout


def test_header_keeps_no_include():
    assert "#include" not in open(os.path.join(CSRC, "batch_decide.hpp")).read()
