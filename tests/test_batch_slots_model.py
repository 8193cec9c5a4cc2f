"""The word-slot bookkeeping of the bit-parallel sweep (graphblast_amd/csrc/batch_slots.hpp) over scripted sweeps: the
header is compiled by the host compiler alone -- it must not need HIP -- into a small driver that reads
`nstore first_plain c0 c1 c2 c3` and then events, and prints every choice it makes:

  H            a host level: planned, then committed
  A 1 / A 0    the next level planned ahead, then committed as a host level / dropped
  L done st    a light-level launch that ran `done` levels and ended with status `st`

After every event it prints the class's answers (frontier, kept levels, clean flags, the plan and the light-level
launch's arrays it would choose next).  This file keeps a record of its own of which arrays were written and which are
all-zero, and holds the driver's lines against it."""
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphblast_amd", "csrc")

DRIVER = r"""
#include "batch_slots.hpp"
#include <cstdio>
static void state(const grb::BatchSlots& s, int nstore) {
  printf("S f=%d ad=%d lv=", s.frontier(), (int)s.any_direct());
  for (int i = 0; i < s.nkept(); ++i) printf("%s%d", i ? "," : "", s.kept_level(i));
  printf(" cl=");
  for (int i = 0; i < 4; ++i) printf("%d", (int)s.clean(nstore + 1 + i));
  printf(" fl=");
  for (int i = 0; i < 4; ++i) printf("%d", (int)s.clean_flags()[i]);
  const grb::SlotPlan p = s.plan();
  int x[3];
  s.light_pick(x);
  printf(" plan=%d:%d light=%d,%d,%d\n", (int)p.keep, p.slot, x[0], x[1], x[2]);
}
int main() {
  int nstore, first_plain, c[4];
  if (scanf("%d %d %d %d %d %d", &nstore, &first_plain, &c[0], &c[1], &c[2], &c[3]) != 6) return 2;
  const bool clean[4] = {c[0] != 0, c[1] != 0, c[2] != 0, c[3] != 0};
  grb::BatchSlots s;
  s.begin(nstore, clean);
  if (first_plain) s.first_plain();
  state(s, nstore);
  int iter = 1;
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'H' || what == 'A') {
      int commit = 1;
      if (what == 'A' && scanf("%d", &commit) != 1) return 2;
      const grb::SlotPlan p = s.plan();
      if (what == 'A') printf("A keep=%d write=%d\n", (int)p.keep, p.slot);
      if (commit) {
        const grb::SlotPlan now = s.plan();                 // what the iteration itself would plan
        printf("H it=%d read=%d keep=%d write=%d now=%d:%d\n", iter, s.frontier(), (int)p.keep, p.slot, (int)now.keep, now.slot);
        s.commit(p, iter);
        ++iter;
      }
    } else if (what == 'L') {
      int done, status, x[3];
      if (scanf("%d %d", &done, &status) != 2 || done < 1) return 2;
      s.light_pick(x);
      printf("L it=%d read=%d x=%d,%d,%d memset=%d%d%d\n", iter, s.frontier(), x[0], x[1], x[2], (int)!s.clean(x[0]), (int)!s.clean(x[1]),
             (int)!s.clean(x[2]));
      s.light_done(x, done, status);
      iter += done;
    } else {
      return 2;
    }
    state(s, nstore);
  }
  return 0;
}
"""


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("batch_slots")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, str(src), "-o", str(exe)])
    return str(exe)


def fields(line):
    return dict(t.split("=") for t in line.split()[1:])


def ints(text):
    return [int(x) for x in text.split(",")] if text else []


def check_sweep(driver, nstore, first_plain, clean, events):
    """runs one scripted sweep and holds every line against this function's own record; -> that record"""
    text = "%d %d %s\n%s\n" % (nstore, int(first_plain), " ".join(str(int(c)) for c in clean), "\n".join(events))
    lines = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    rot = list(range(nstore + 1, nstore + 5))
    zero = {s: bool(c) for s, c in zip(rot, clean)}         # the rotating arrays that are all-zero
    kept = {} if first_plain else {0: 0}                    # kept slot -> the iteration that wrote it
    frontier = -1 if first_plain else 0
    direct = bool(first_plain)
    it = 1
    at = 0

    def state():
        nonlocal at
        assert lines[at].startswith("S "), lines[at]
        s = fields(lines[at])
        at += 1
        assert int(s["f"]) == frontier and bool(int(s["ad"])) == direct, (s, frontier, direct)
        assert ints(s["lv"]) == [kept[i] for i in range(len(kept))], (s, kept)      # kept slot i is the i-th taken
        assert s["cl"] == s["fl"]
        for slot, c in zip(rot, s["cl"]):
            assert c == "0" or zero[slot], (s, zero)        # reported clean: all-zero in the record
        return s

    last = state()
    for ev in events:
        if ev[0] in "HA":
            commit = ev == "H" or ev.split()[1] == "1"
            if ev[0] == "A":
                a = fields(lines[at])
                at += 1
                assert lines[at - 1].startswith("A ") and "%s:%s" % (a["keep"], a["write"]) == last["plan"]
            if commit:
                assert lines[at].startswith("H "), lines[at]
                h = fields(lines[at])
                at += 1
                read, write, keep = int(h["read"]), int(h["write"]), h["keep"] == "1"
                assert int(h["it"]) == it and read == frontier
                assert h["now"] == "%s:%s" % (h["keep"], h["write"])       # planned ahead or now: the same plan
                assert write != read
                assert keep == (len(kept) <= nstore), (h, kept)
                if keep:
                    assert 0 <= write <= nstore and write not in kept
                    kept[write] = it
                else:
                    assert write in rot
                    dirty = [s for s in rot if s != read and not zero[s]]
                    assert not dirty or write in dirty, (h, zero)           # the clean stay clean
                    zero[write] = False
                    direct = True
                if first_plain and it == 1:
                    assert keep and write == 0 and kept == {0: 1}
                frontier = write
                it += 1
                last = state()
            else:
                s = state()
                assert s == last, (s, last)                                # a dropped plan changes no answer
        else:
            _, done, status = ev.split()
            done, status = int(done), int(status)
            assert lines[at].startswith("L "), lines[at]
            l = fields(lines[at])
            at += 1
            x = ints(l["x"])
            assert int(l["it"]) == it and int(l["read"]) == frontier
            assert ints(last["light"]) == x
            assert len(set(x)) == 3 and all(s in rot for s in x) and frontier not in x
            for s, m in zip(x, l["memset"]):
                assert (m == "1") == (not zero[s]), (l, zero)              # memset exactly the arrays that are not zero
            spare = [s for s in rot if s != frontier and s not in x]
            assert all(zero[s] for s in x) or not any(zero[s] for s in spare)   # clean ones first
            for s in x:
                zero[s] = True                              # the launch leaves its arrays all-zero ...
            frontier = x[(done - 1) % 3]
            if status != 0:
                zero[frontier] = False                      # ... but the last level's words when it found anything
            direct = True
            it += done
            last = state()
    assert at == len(lines)
    return [zero[s] for s in rot]


def scripts(seed, count, length, first_plain):
    rng = random.Random(seed)
    for _ in range(count):
        ev = ["H"] if first_plain else []
        lights = 0
        while len(ev) < length:
            r = rng.random()
            if r < 0.35:
                ev.append("H")
            elif r < 0.6:
                ev.append("A 1")
            else:
                if r < 0.8:
                    ev.append("A 0")
                ev.append("L %d 2" % rng.randint(1, 7))
                lights += 1
        yield ev[:length], lights


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "batch_slots.hpp")).read()
    assert re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, flags=re.M) == []
    user = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".hpp")) and '"batch_slots.hpp"' in open(os.path.join(CSRC, f)).read()]
    assert user == ["bfs_batch.hip"]


@pytest.mark.parametrize("nstore", [1, 16])
@pytest.mark.parametrize("first_plain", [False, True])
def test_scripted_sweeps(driver, nstore, first_plain):
    most = 0
    for clean in ((0, 0, 0, 0), (1, 1, 1, 1), (0, 1, 0, 1), (1, 0, 0, 0)):
        for ev, lights in scripts(7 * nstore + int(first_plain), 6, 40, first_plain):
            check_sweep(driver, nstore, first_plain, clean, ev)
            most = max(most, lights)
    assert most >= 5


@pytest.mark.parametrize("nstore", [1, 16])
def test_four_and_five_light_launches_and_the_next_sweep(driver, nstore):
    """levels up to and beyond the kept slots, light launches between them with every length mod 3, one that ends the
    sweep; the next sweep starts from the flags the first one left"""
    for nlight in (4, 5):
        ev = []
        for j in range(nlight - 1):
            ev += ["H"] * (1 + 5 * j) + ["A 1", "A 0", "L %d 2" % (j + 1)]
        for last in ("L 3 0", "L 2 1"):
            left = check_sweep(driver, nstore, False, (0, 0, 0, 0), ev + ["A 1", "A 0", last])
            assert sum(left) >= 3 if last.endswith("0") else sum(left) >= 2
            check_sweep(driver, nstore, True, left, ["H", "A 0", "L 1 2", "A 1", "H", "L 4 0"])


def test_second_level_rotates_when_one_level_is_kept(driver):
    check_sweep(driver, 1, False, (1, 1, 1, 1), ["H", "H", "H", "A 1", "A 0", "L 2 2", "H"])
    text = "1 0 1 1 1 1\nH\nH\nH\n"
    out = subprocess.run([driver], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    writes = [int(fields(l)["write"]) for l in out if l.startswith("H ")]
    assert writes[0] == 1 and writes[1] >= 2 and writes[2] >= 2 and writes[1] != writes[2]   # kept, then two rotating in turn
