"""The host reference of tests/spmv_long_cases.py against the oracle's mxv / vxm, which fold every row sequentially
(oracle/ops.py): the 13 commutative semirings, both types, both orientations, none / mask / scmp / accum, on the
plain and the wide matrix.  The data are exact, so the order of a fold is free and the comparison is bit for bit.
No GPU."""
import numpy as np
import pytest

import spmv_long_cases as slc
from oracle import ops
from oracle.semiring import Semiring

VARIANTS = ["none", "mask", "scmp", "accum"]


def _oracle(case, A, tran, sr_name, dtype, u, w0, mask, variant):
    use_mask, scmp, accum = slc.VARIANTS[variant]
    d = ops.Descriptor()
    d.loadArgs(mxvmode=2, fusedmask=0)
    if scmp:
        d.set(ops.GrB_MASK, ops.GrB_SCMP)
    nin, nout = (case.nrows, case.ncols) if tran else (case.ncols, case.nrows)
    uv, w = ops.Vector(nin, dtype), ops.Vector(nout, dtype)
    uv.build_dense(u)
    w.build_dense(w0)
    mk = None
    if use_mask:
        mk = ops.Vector(nout, dtype)
        mk.build_dense(mask)
    sr = Semiring(sr_name, dtype)
    if tran:
        assert ops.vxm(w, mk, accum or None, sr, uv, A, d) == 0
    else:
        assert ops.mxv(w, mk, accum or None, sr, A, uv, d) == 0
    return w.extractTuples_dense()


def _compare(case, mats, tran, sr, dtype, variant):
    vals, u, w0, mask = slc.operands(case, tran, sr)
    key = (sr == "MultipliesMultiplies", dtype)
    if key not in mats:
        mats[key] = ops.Matrix(case.nrows, case.ncols, dtype)
        mats[key].build_csr(case.ptr, case.ind, vals.astype(dtype))
    use_mask, scmp, accum = slc.VARIANTS[variant]
    got = slc.want(case, tran, sr, dtype, vals, u, mask if use_mask else None, scmp, accum, w0)
    ref = _oracle(case, mats[key], tran, sr, dtype, u, w0, mask, variant)
    assert got.dtype == ref.dtype and np.array_equal(got, ref), (case.name, tran, sr, dtype.__name__, variant)


def test_conditions_of_the_three_matrices():
    """what routes the kernels depend on (asserted inside the builders too): distinct columns, hot share, the column
    of rank 32768, the flat matrix's nhot == 0 arithmetic, the long rows and the empty tile"""
    W, N, P = slc.wide(), slc.flat(), slc.plain()
    assert (W.nrows, W.ncols) == (3000, 40000) and (N.nrows, N.ncols) == (1500, 300000) and (P.nrows, P.ncols) == (1000, 1000)
    assert np.count_nonzero(W.col_count) > slc.HOT and W.hot_refs(0) * 8 >= W.nvals
    assert np.sort(W.col_count)[::-1][slc.HOT] >= 1
    assert W.nrows <= slc.HOT                                   # vxm on W: the whole vector in LDS ...
    assert len(slc.wave_tiles(W.tptr)) >= 100                   # ... over a hundred tiles or so, hub columns sliced
    assert any(s for _, _, s in slc.wave_tiles(W.tptr))
    assert N.nvals == 300000 and N.hot_refs(0) * 8 == 262144 < N.nvals
    lens = np.diff(W.ptr)
    assert lens.max() == 1300 and 512 in lens and 513 in lens and lens[0] == 0 and lens[-1] == 0
    # the transposed orientation is the transpose: same entries
    for c in (W, N, P):
        rows = np.repeat(np.arange(c.nrows), np.diff(c.ptr))
        cols = np.repeat(np.arange(c.ncols), np.diff(c.tptr))
        assert np.array_equal(np.sort(rows * c.ncols + c.ind), np.sort(c.tind.astype(np.int64) * c.ncols + cols))


def test_operands_stay_exact():
    """every sum below 2^24 in any order (asserted by want() on every call): all semirings, both orientations, with
    the accumulation, on all three matrices and their iso twins"""
    for name, build in slc.CASES.items():
        case = build()
        for sr in slc.COMMUTATIVE:
            for tran in (0, 1):
                if name == "N" and tran and sr != "PlusMultiplies":
                    continue
                for iso in (False, True):
                    vals, u, w0, mask = slc.operands(case, tran, sr, iso)
                    assert (np.unique(vals).size == 1) == iso or sr == "MultipliesMultiplies"
                    for dtype in slc.DTYPES:
                        slc.want(case, tran, sr, dtype, vals, u, mask, 1, 1, w0)
    # MultipliesMultiplies is no constant: ones, twos (or more) and zeros all occur among W's results
    W = slc.wide()
    vals, u, w0, mask = slc.operands(W, 1, "MultipliesMultiplies")
    res = slc.want(W, 1, "MultipliesMultiplies", np.int32, vals, u)
    assert np.any(res == 0) and np.any(res == 1) and np.any(res > 1)


@pytest.mark.parametrize("dtype", slc.DTYPES, ids=["f32", "i32"])
def test_reference_equals_the_oracle_on_the_plain_matrix(dtype):
    """P: int32 in full (the oracle folds integers with reduceat); float32 sums go through the oracle's row loop, so
    each semiring takes two of the eight (orientation, variant) pairs, dealt round-robin"""
    case, mats = slc.plain(), {}
    pairs = [(t, v) for t in (0, 1) for v in VARIANTS]
    for k, sr in enumerate(slc.COMMUTATIVE):
        todo = pairs if dtype is np.int32 else [pairs[k % 8], pairs[(k + 5) % 8]]
        for tran, variant in todo:
            _compare(case, mats, tran, sr, dtype, variant)


@pytest.mark.parametrize("dtype", slc.DTYPES, ids=["f32", "i32"])
def test_reference_equals_the_oracle_on_the_wide_matrix(dtype):
    """W, rectangular: int32 in full; float32 one (orientation, variant) pair per semiring, dealt round-robin"""
    case, mats = slc.wide(), {}
    pairs = [(t, v) for t in (0, 1) for v in VARIANTS]
    for k, sr in enumerate(slc.COMMUTATIVE):
        todo = pairs if dtype is np.int32 else [pairs[(3 * k + 1) % 8]]
        for tran, variant in todo:
            _compare(case, mats, tran, sr, dtype, variant)
