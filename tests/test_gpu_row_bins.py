"""The row-bin pipeline that eWise, extract and assign share (csrc/row_bins.hpp) past one tile of the bin kernel: 4099 rows
are two full 2048-row tiles and a three-row one, each workgroup's lists appended behind the other's.  Every full tile holds
every bin of both threshold sets; the partial tile begins and ends with a hub row (three rows cannot hold four kinds; for
extract, whose bins follow the row list, four more output rows make the last tile hold all of them).  Integer values, so
every comparison with scipy is exact.  (The kernel's grid-stride step starts above 2048 * 2048 rows: not reached here.)"""
import numpy as np
import pytest
import scipy.sparse as sp

import test_gpu_assign as asg
import test_gpu_ewise_matrix as ewm
import test_gpu_extract as xt
from backends import HipBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
TILE = 2048
M, N = 2 * TILE + 3, 4000
HUB = 1500


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


def _lengths():
    r = np.arange(M)
    lens = np.array([0, 5, 40])[r % 3]
    lens[r % 64 == 63] = HUB
    lens[[TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, M - 1]] = HUB          # the tile edges and the last row
    return lens


def _bins(lens, short, seg):
    """-1 none, 0 short, 1 wave, 2 hub: row_bin_of"""
    return np.where(lens <= 0, -1, np.where(lens <= short, 0, np.where(lens <= seg, 1, 2)))


def _assert_tiles(lens, short, seg, last_tile):
    """every full tile holds every kind of row, the last one at least `last_tile` and a hub row at its end; hub rows have
    two segments"""
    bins = _bins(lens, short, seg)
    assert lens.size > 2 * TILE and lens.size % TILE != 0
    for t in range(0, lens.size, TILE):
        kinds = set(bins[t:t + TILE].tolist())
        assert kinds >= ({-1, 0, 1, 2} if t + TILE <= lens.size else last_tile), (t, kinds)
    assert bins[-1] == 2
    assert (-(-lens[bins == 2] // seg) == 2).all()


@pytest.fixture(scope="module")
def case():
    rng = np.random.default_rng(97)
    lens = _lengths()
    ptr = np.r_[0, np.cumsum(lens)].astype(np.int32)
    ai = np.concatenate([np.sort(rng.choice(N, k, replace=False)) for k in lens]).astype(np.int32)
    bi = np.concatenate([np.sort(rng.choice(N, k, replace=False)) for k in lens]).astype(np.int32)
    av, bv = rng.integers(1, 4, ai.size), rng.integers(1, 4, bi.size)
    # extract: a permutation of the rows, then an empty, a short, a wave row and row 4098 twice more
    rows = np.r_[rng.permutation(M), 0, 1, 2, M - 1, M - 1].astype(np.int32)
    cols = np.sort(rng.choice(N, N // 2, replace=False)).astype(np.int32)
    assert (rows == M - 1).sum() == 3
    _assert_tiles(lens[rows], 16, 1024, {-1, 0, 1, 2})                   # extract: the source row's length
    _assert_tiles(2 * lens, 32, 2048, {1, 2})                            # eWise and assign: the merged length
    assert set(_bins(2 * lens, 32, 2048)[2 * TILE:].tolist()) == {1, 2} and _bins(2 * lens, 32, 2048)[2 * TILE] == 2
    out = {"ptr": ptr, "ai": ai, "bi": bi, "rows": rows, "cols": cols}
    for dt in (F, I):
        SA = sp.csr_matrix((av.astype(dt), ai, ptr), shape=(M, N))
        SB = sp.csr_matrix((bv.astype(dt), bi, ptr), shape=(M, N))
        want = {"add": (SA + SB).tocsr(), "mult": SA.multiply(SB).tocsr(), "extract": SA[rows][:, cols].tocsr()}
        for W in want.values():
            W.sort_indices()
            assert W.dtype == dt and (W.data != 0).all()                 # nothing scipy would have dropped or widened
        out[dt] = (av.astype(dt), bv.astype(dt), want)
    return out


def _csr(W):
    return W.indptr.astype(np.int32), W.indices.astype(np.int32), W.data


@pytest.mark.parametrize("dt", [F, I])
def test_ewise_across_tiles(hb, case, dt):
    g = hb.g
    av, bv, want = case[dt]
    A, B = ewm._mat(g, M, N, case["ptr"], case["ai"], av), ewm._mat(g, M, N, case["ptr"], case["bi"], bv)
    for name, fn in (("add", g.eWiseAdd), ("mult", g.eWiseMult)):
        Cm = g.Matrix(M, N, dt)
        assert fn(Cm, None, None, "PlusMultiplies", A, B, hb.descriptor()) == 0, name
        asg._same(Cm.host_csr(), _csr(want[name]), name)
        ewm._check_csc(Cm, M, N, name)


@pytest.mark.parametrize("dt", [F, I])
def test_extract_across_tiles(hb, case, dt):
    g = hb.g
    av, _, want = case[dt]
    rows, cols = case["rows"], case["cols"]
    A = xt._mat(g, M, N, case["ptr"], case["ai"], av)
    Cm = g.Matrix(rows.size, cols.size, dt)
    assert g.extract(Cm, None, None, A, rows, cols, hb.descriptor()) == 0
    xt._same(Cm.host_csr(), _csr(want["extract"]))
    xt._check_csc(Cm, rows.size, cols.size)


@pytest.mark.parametrize("dt", [F, I])
def test_assign_across_tiles(hb, case, dt):
    """C holds B; C(:, :) += A is the union with sums where both store an entry.  The empty rows of A are copied rows."""
    g = hb.g
    av, bv, want = case[dt]
    A = asg._mat(g, M, N, case["ptr"], case["ai"], av)
    Cm = asg._mat(g, M, N, case["ptr"], case["bi"], bv)
    assert g.assign_matrix(Cm, None, "plus", A, None, None, hb.descriptor()) == 0
    p, i, v = Cm.host_csr()
    asg._same((p, i, v), _csr(want["add"]))
    asg._same(Cm.host_csc(), asg._transpose(M, N, p, i, v))
