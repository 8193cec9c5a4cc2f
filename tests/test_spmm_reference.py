"""The host references of tests/spmm_cases.py against something independent of them: the stacked column-by-column
reference against a sparse (or dense) matrix product in int64 / float64, the fold by position against the plain loop
over a row's entries, and the tile census every case exists for.  No GPU."""
import numpy as np
import pytest

import spmm_cases as sc
from oracle.semiring import Semiring

IDS = ["f32", "i32"]


def _product(ptr, ind, val, nrows, ncols, B):
    """A @ B in the wide type, by scipy where it is installed"""
    try:
        import scipy.sparse as sp
    except ImportError:
        dense = np.zeros((nrows, ncols), dtype=val.dtype)
        dense[np.repeat(np.arange(nrows), np.diff(ptr)), ind] = val
        return dense @ B
    return np.asarray(sp.csr_matrix((val, ind, ptr), shape=(nrows, ncols)) @ B)


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["P", "R", "T"])
def test_plus_multiplies_equals_the_matrix_product(name, dtype):
    wide_t = np.float64 if dtype is np.float32 else np.int64
    case = sc.CASES[name]()
    vals = sc.matrix_values(case, "PlusMultiplies")
    for tran in (0, 1):
        ptr, ind, v, nout, nin = case.arrays(tran, vals)
        B = sc.rhs(case, tran, "PlusMultiplies")
        assert B.shape == (nin, sc.KMAX)
        got = sc.expected(case, tran, "PlusMultiplies", dtype, sc.KMAX)
        ref = _product(ptr, ind, v.astype(wide_t), nout, nin, B.astype(wide_t))
        assert got.shape == (nout, sc.KMAX) and got.dtype == dtype
        assert np.array_equal(got.astype(wide_t), ref), (name, tran)
        for k in (1, 17, 129):                                          # a narrower product is the leading columns
            assert np.array_equal(sc.expected(case, tran, "PlusMultiplies", dtype, k), got[:, :k])
    # the two orientations are each other's transpose: A B and A' B' share the entries
    dense = np.zeros((case.nrows, case.ncols), dtype=np.int64)
    dense[np.repeat(np.arange(case.nrows), np.diff(case.ptr)), case.ind] = vals
    assert np.array_equal(sc.expected(case, 1, "PlusMultiplies", np.int32, 5),
                          dense.T @ sc.rhs(case, 1, "PlusMultiplies")[:, :5])


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("sr_name", ["PlusMultiplies", "MinimumPlus", "GreaterPlus", "NotEqualToPlus"])
def test_fold_by_position_equals_the_loop_over_entries(sr_name, dtype):
    from test_gpu_spmm import dense_ref
    case, k = sc.plain(), 7
    sr = Semiring(sr_name, dtype)
    for tran in (0, 1):
        ptr, ind, v, nout, nin = case.arrays(tran, sc.matrix_values(case, sr_name))
        B = sc.rhs(case, tran, sr_name)[:, :k].astype(dtype)
        ref = dense_ref(sr, ptr, ind, v.astype(dtype), B, dtype)
        got = sc.fold_in_order(sr, ptr, ind, v, B, dtype)
        assert got.dtype == ref.dtype and np.array_equal(got, ref), (sr_name, tran)
        rows, part = sc.expected_in_order(case, tran, sr_name, dtype, k) if sr_name in sc.ORDERED else (None, None)
        if rows is not None:
            assert np.array_equal(part[rows], ref[rows])
            left_out = np.setdiff1d(np.arange(nout), rows)
            assert left_out.size <= 8 and np.all(np.diff(ptr)[left_out] > sc.TILE)


@pytest.mark.parametrize("name", ["P", "R", "T"])
def test_exact_data_make_the_order_free(name):
    """all 13 commutative semirings: the fold in CSR order, in the type itself, equals the wide fold by reduceat on
    every row, the sliced ones included"""
    case = sc.CASES[name]()
    for sr_name in sc.COMMUTATIVE:
        for tran in (0, 1):
            for dtype in sc.DTYPES:
                ptr, ind, v, nout, nin = case.arrays(tran, sc.matrix_values(case, sr_name))
                got = sc.fold_in_order(Semiring(sr_name, dtype), ptr, ind, v, sc.rhs(case, tran, sr_name), dtype)
                assert np.array_equal(got, sc.expected(case, tran, sr_name, dtype, sc.KMAX)), (name, sr_name, tran, dtype)


def test_the_ordered_semirings_depend_on_the_order():
    """... which is why they have a reference of their own: folded backwards, the rows give other results.  (GreaterPlus
    does not on these data: with positive products, identity > x and then 0 > x are false whatever the order, so every
    non-empty row is 0.  It still tells a written row from an unwritten one and an empty row's identity.)"""
    case = sc.plain()
    for sr_name in ("CustomLessPlus", "NotEqualToPlus", "CustomLessLess"):
        sr = Semiring(sr_name, np.int32)
        ptr, ind, v, nout, nin = case.arrays(0, sc.matrix_values(case, sr_name))
        B = sc.rhs(case, 0, sr_name)[:, :5]
        rev = np.concatenate([np.arange(ptr[r], ptr[r + 1])[::-1] for r in range(nout)]) if nout else np.zeros(0, int)
        fwd = sc.fold_in_order(sr, ptr, ind, v, B, np.int32)
        bwd = sc.fold_in_order(sr, ptr, ind[rev], v[rev], B, np.int32)
        assert not np.array_equal(fwd, bwd), sr_name


def test_stride_reference():
    """S: the fold by position equals the wide fold column by column (two columns of it)"""
    case = sc.stride()
    for sr_name in ("PlusMultiplies", "MinimumPlus"):
        got = sc.expected_stride(sr_name, np.float32, 70)
        assert got.shape == (8300, 70)
        vals, B = sc.matrix_values(case, sr_name), sc.rhs(case, 0, sr_name, 70)
        for c in (0, 69):
            assert np.array_equal(got[:, c], sc.want(case, 0, sr_name, np.float32, vals, B[:, c])), (sr_name, c)


def test_real_bound_separates_a_dropped_entry():
    """the bound of the float test is below one product (>= 0.25) on every row: n <= 1025 entries below 1 give at most
    1025^2 * 2^-24 = 0.063 on the longest row, and 1e-5 on a row of a dozen entries"""
    case = sc.wide()
    for tran in (0, 1):
        vals, B = sc.real_values("R"), sc.real_rhs("R", tran, 17)
        exact, bound = sc.real_product(case, tran, vals, B)
        assert bound.max() < 1025 * 2.0 ** -24 * 1.001 * exact.max() and bound.max() < 0.25 / 3
        assert np.median(bound[bound > 0]) < 0.25 / 10000
        # the float32 fold in CSR order stays inside it
        ptr, ind, v, nout, nin = case.arrays(tran, vals)
        f32 = sc.fold_in_order(Semiring("PlusMultiplies", np.float32), ptr, ind, v, B, np.float32)
        assert np.all(np.abs(f32.astype(np.float64) - exact) <= bound)


def test_tile_census_of_every_case():
    """the paths of spmm_tile_kernel each case exists for (the builders assert most of it again)"""
    cs = {(n, t): sc.census(b().tptr if t else b().ptr) for n, b in sc.CASES.items() for t in (0, 1)}
    P, R, T = sc.plain(), sc.wide(), sc.tall()
    lens = np.diff(P.ptr)
    assert lens[7] == 1000 and lens[11] == 512 and lens[12] == 513 and lens[0] == 0 and lens[-1] == 0
    assert cs["P", 0]["slice_lens"] == [512, 488, 512, 1] and cs["P", 0]["nempty_full"] >= 1
    assert sorted(P.col_count[P.col_count > sc.TILE].tolist(), reverse=True) == [839, 739, 640, 537]
    assert cs["P", 1]["nlong"] == 4 and cs["P", 1]["nslices"] == 8
    assert (R.nrows, R.ncols, R.nvals) == (900, 1300, 7170) and (T.nrows, T.ncols, T.nvals) == (1300, 900, 8446)
    assert cs["R", 0]["slice_lens"][:3] == [512, 512, 1] and cs["R", 1]["nlong"] == 3
    assert np.diff(T.ptr)[7] == 700 and max(-(-n // sc.TILE) for n in T.col_count) == 3
    for name in "PRT":
        for t in (0, 1):
            assert cs[name, t]["nslices"] >= 2, (name, t)
        assert cs[name, 0]["nempty_full"] >= 1                          # a run of 64 empty rows in a tile of its own
    assert cs["E", 0]["ntiles"] == cs["E", 0]["nempty"] and sc.empty().nvals == 0
    assert cs["One", 0]["slice_lens"] == [512, 88] and cs["One", 1]["nslices"] == 0 and cs["OneT", 1]["nslices"] == 2
    assert cs["First", 0]["nempty_at_end"] == 4 and cs["Last", 0]["nempty_full"] == 4
    assert cs["S", 0]["ntiles"] == 8300 > sc.GRID_WAVES and cs["S", 0]["nslices"] == 0
    # every case's second orientation is the transpose of the first
    for b in sc.CASES.values():
        c = b()
        rows = np.repeat(np.arange(c.nrows), np.diff(c.ptr))
        cols = np.repeat(np.arange(c.ncols), np.diff(c.tptr))
        assert np.array_equal(np.sort(rows * c.ncols + c.ind), np.sort(c.tind.astype(np.int64) * c.ncols + cols))
