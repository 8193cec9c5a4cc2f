"""The launch rule of the partitioned traversals (graphblast_amd/csrc/part_driver.hpp) over a scripted mailbox: the
header is compiled by the host compiler alone -- it must not need HIP -- into a small driver whose mail word is a list
that the read callable steps through (it stays on the last entry), with no device, no threads and no sleeping.  The
driver prints what happened in order: r<word> for a read, L<k> for launch k going out, S for the stall callable."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "graphblast_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")

DRIVER = r"""
#include "part_driver.hpp"
#include <cstdio>
#include <vector>
int main() {
  char what;
  while (scanf(" %c", &what) == 1) {
    if (what == 'D') {                       // D word: decode
      unsigned long long g;
      if (scanf("%llu", &g) != 1) return 2;
      const grb::PartMailWord m = grb::part_mail_decode(g);
      printf("%d %d\n", m.launches_done, m.done_at);
    } else if (what == 'E') {                // E k done_at bad: encode
      int k, done_at, bad;
      if (scanf("%d %d %d", &k, &done_at, &bad) != 3) return 2;
      printf("%llu\n", grb::part_mail_encode(k, done_at, bad != 0));
    } else if (what == 'R') {                // R limit_seconds one_shot nwords words...: run the loop
      int limit, one_shot, nwords;
      if (scanf("%d %d %d", &limit, &one_shot, &nwords) != 3 || nwords < 1) return 2;
      std::vector<unsigned long long> words(nwords);
      for (auto& w : words) if (scanf("%llu", &w) != 1) return 2;
      size_t at = 0;
      int launches = -1;
      const grb_info info = grb::part_drive(
          [&] {
            const unsigned long long w = words[at];
            if (at + 1 < words.size()) ++at;
            printf("r%llu ", w);
            return w;
          },
          [&](int k) -> grb_info { printf("L%d ", k); return GRB_SUCCESS; },
          [&]() -> grb_info { printf("S "); return GRB_SUCCESS; }, limit, one_shot != 0, &launches);
      printf("| %s %d\n", info == GRB_SUCCESS ? "ok" : info == GRB_PANIC ? "panic" : "other", launches);
    } else {
      return 2;
    }
  }
  return 0;
}
"""

DISTRESS = 0xFFFFFFFF


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("part_driver")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, "-I" + INCLUDE, str(src), "-o", str(exe)])
    return str(exe)


def ask(driver, lines):
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout
    return out.strip().split("\n")


def run_loop(driver, words, limit=3600, one_shot=False):
    """-> (events, outcome, launches): events are ('r', word), ('L', k) and ('S',) in order"""
    line, = ask(driver, ["R %d %d %d %s" % (limit, int(one_shot), len(words), " ".join(str(w) for w in words))])
    ev, tail = line.split("|")
    outcome, launches = tail.split()
    events = [(t[0], int(t[1:])) if len(t) > 1 else (t,) for t in ev.split()]
    return events, outcome, int(launches)


def word(launches_done, ended_by=None):
    return ((0 if ended_by is None else ended_by + 1) << 32) | launches_done


def script(e, repeat):
    """what the host may read while launch e ends the traversal: nothing yet, then the report of launch 0, 1, ... e + 1
    (launch j says `ended by e` from j = e on), each seen `repeat` times"""
    words = [0] * repeat
    for j in range(e + 2):
        words += [word(j + 1, e if j >= e else None)] * repeat
    return words


def check_order(events):
    """launch k goes out only after a word with launches_done >= k - 1 was read; launches go out in order, once each"""
    seen = 0
    nxt = 0
    for ev in events:
        if ev[0] == "r":
            seen = max(seen, ev[1] & 0xFFFFFFFF)
        elif ev[0] == "L":
            assert ev[1] == nxt, events
            assert ev[1] < 2 or seen >= ev[1] - 1, (ev, events)
            nxt += 1
    return nxt


def test_header_needs_no_hip():
    text = open(os.path.join(CSRC, "part_driver.hpp")).read()
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", text, flags=re.M)
    assert sorted(includes) == ["chrono", "grb_hip.h"], includes          # the standard clock and the library's C header
    public = open(os.path.join(INCLUDE, "grb_hip.h")).read()
    assert not re.search(r"#\s*include\s*[<\"]hip", public)


@pytest.mark.parametrize("e", range(6))
def test_traversal_that_launch_e_ends_takes_e_plus_2_launches(driver, e):
    for repeat in (1, 2, 5):
        events, outcome, launches = run_loop(driver, script(e, repeat))
        assert outcome == "ok" and launches == e + 2, (e, repeat, events)
        assert check_order(events) == e + 2
        assert ("S",) not in events
    # the device ran ahead: the first word the host sees is already that of launch 1, the last one it has enqueued
    words = [word(j + 1, e if j >= e else None) for j in range(1, e + 2)]
    events, outcome, launches = run_loop(driver, words)
    assert outcome == "ok" and launches == e + 2 and check_order(events) == e + 2, (e, events)


def test_distress_is_panic_and_nothing_more_goes_out(driver):
    for bad_after in range(1, 5):                       # the report of launch bad_after - 1 carries the distress value
        words = [0] + [word(j + 1) for j in range(bad_after - 1)] + [(DISTRESS << 32) | bad_after]
        events, outcome, launches = run_loop(driver, words)
        assert outcome == "panic", events
        sent = check_order(events)
        first_bad = next(i for i, ev in enumerate(events) if ev[0] == "r" and ev[1] >> 32 == DISTRESS)
        assert not any(ev[0] == "L" for ev in events[first_bad:]), events
        assert sent == bad_after + 1                   # it was read while waiting to send launch bad_after + 1


def test_one_shot_is_one_launch_and_never_reads(driver):
    events, outcome, launches = run_loop(driver, [word(1, 0)], one_shot=True)
    assert (events, outcome, launches) == ([("L", 0)], "ok", 1)


def test_mailbox_that_never_advances_stalls_once_then_panics(driver):
    events, outcome, launches = run_loop(driver, [0], limit=0)
    assert outcome == "panic"
    assert events.count(("S",)) == 1
    assert [ev for ev in events if ev[0] == "L"] == [("L", 0), ("L", 1)]
    assert events[-1][0] == "r" and events.index(("S",)) > 2        # reads on both sides of the one stall
    # ... and one that advances only behind the stall (the stream had been slow, not stuck) goes on
    words = [0] * 5000 + script(1, 1)
    events, outcome, launches = run_loop(driver, words, limit=0)
    assert outcome == "ok" and launches == 3 and events.count(("S",)) == 1 and check_order(events) == 3


def test_mail_word_decoding(driver):
    asks, want = ["D 0"], ["0 -1"]
    for e in range(6):
        for k in (1, 2, 7, (1 << 28) + 1):
            asks.append("D %d" % (((e + 1) << 32) | k))
            want.append("%d %d" % (k, e))
            asks.append("D %d" % ((DISTRESS << 32) | k))
            want.append("%d -2" % k)
    assert ask(driver, asks) == want
    # what a launch writes is what the host decodes
    asks, want = [], []
    for k in (0, 1, 6):
        for done_at, bad in ((-1, 0), (0, 0), (k, 0), (3, 1)):
            asks.append("E %d %d %d" % (k, done_at, bad))
            want.append(str(((DISTRESS if bad else done_at + 1) << 32) | (k + 1)))
    assert ask(driver, asks) == want
