"""The prefix sums batch_first_level_kernel's grid is built from (csrc/batch_decide.hpp: first_level_pieces), compiled with
a host compiler: source s owns pieces pre[s] .. pre[s + 1], ceil(deg / 256) of them; an empty row none; a vertex named
twice has its pieces twice; the entries behind k all hold the total (the kernel's search may read them)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphblast_amd", "csrc")

DRIVER = r'''
#include <cstdio>
#include <vector>
#include "batch_decide.hpp"
int main() {
  int n, k, piece;
  while (scanf("%d %d %d", &n, &k, &piece) == 3) {
    std::vector<int> ptr(n + 1), src(k > 0 ? k : 1);
    for (int i = 0; i <= n; ++i) if (scanf("%d", &ptr[i]) != 1) return 1;
    for (int i = 0; i < k; ++i) if (scanf("%d", &src[i]) != 1) return 1;
    unsigned int pre[65];
    grb::first_level_pieces(ptr.data(), src.data(), k, piece, pre);
    for (int i = 0; i <= 64; ++i) printf("%u%c", pre[i], i == 64 ? '\n' : ' ');
  }
  return 0;
}
'''


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("pieces")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + CSRC, str(src), "-o", str(exe)])
    return str(exe)


def test_pieces_prefix(driver):
    rng = np.random.default_rng(5)
    degs = np.array([0, 1, 255, 256, 257, 511, 512, 513, 1025, 4097, 100000] + list(rng.integers(0, 3000, 40)))
    ptr = np.concatenate([[0], np.cumsum(degs)])
    n = degs.size
    cases = [(k, [int(x) for x in rng.integers(0, n, k)]) for k in (0, 1, 2, 31, 32, 33, 64)]
    cases.append((11, list(range(11))))
    cases.append((3, [4, 4, 4]))                                    # the same vertex three times
    cases.append((64, [0] * 64))                                    # nothing but empty rows
    lines = []
    for k, src in cases:
        lines.append("%d %d 256" % (n, k))
        lines.append(" ".join(str(int(x)) for x in ptr))
        lines.append(" ".join(str(x) for x in src))
    out = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(cases)
    for (k, src), line in zip(cases, out):
        got = [int(x) for x in line.split()]
        want = [0]
        for s in src:
            want.append(want[-1] + (int(degs[s]) + 255) // 256)
        assert got[:k + 1] == want, (k, src)
        assert got[k:] == [want[-1]] * (65 - k), (k, got)
