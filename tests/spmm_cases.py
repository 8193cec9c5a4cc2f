"""Matrices, right-hand sides and the host references for the SpMM tests (tests/test_gpu_spmm_shapes.py on the GPU,
tests/test_spmm_reference.py on the CPU).

grb_spmm (csrc/spmm.hip) walks the wave tiles of the matrix's SpMV plan: a tile of whole rows (<= 512 entries, <= 64
rows) writes C itself, a row of more than 512 entries is cut into slices that write partial vectors, folded by a second
kernel.  The right-hand side's k columns are served by one of three instantiations (16, 32 or 64 columns per lane
group), picked per launch of 64 columns.  tran = 1 runs the same kernels on the CSC arrays, so the roles of nrows and
ncols swap.  The matrices below reach all of that with a few thousand entries each:

  P    plain    1000 x 1000   tests/spmv_long_cases.py's: rows of 1000 / 512 / 513 entries, an all-empty tile, empty ends
  R    wide      900 x 1300   the same skeleton, row 7 with 1025 entries = slices of 512, 512 and ONE entry
  T    tall     1300 x  900   its transposed orientation has columns of three slices
  E    empty     200 x  150   nvals == 0: spmm_empty_kernel
  One            1 x  700     one row of 600 entries (two slices); transposed: 700 rows of at most one entry
  OneT         700 x    1     the same entries stored the other way round
  First        257 x  200     entries in row 0 only: four all-empty tiles that start AT the end of the arrays
  Last         257 x  200     entries in the last row only: four all-empty tiles, then a tile of one row
  S    stride  8300 x  600    257 entries in every row: one row per tile, 8300 tiles > the 8192 waves of a full grid

Case, wave_tiles, values, vector, want, COMMUTATIVE and DTYPES are those of tests/spmv_long_cases.py: the data are
small integers (dyadic quotients for PlusDivides, mostly ones for MultipliesMultiplies), every partial sum in any order
is exact in float32 and int32 (want() asserts it on every call), and the comparison is bit for bit.  Column c of B is
vector(case, tran, sr, attempt=c).  Every builder asserts in numpy the conditions it exists for, so that a change of
seed cannot silently leave a path."""
import functools

import numpy as np

import spmv_long_cases as slc
from oracle.semiring import Semiring
from spmv_long_cases import COMMUTATIVE, DTYPES, TILE, TILE_ROWS, Case, values, vector, want, wave_tiles  # noqa: F401

KMAX = 130                      # widest right-hand side of the tests: two full launches of 64 columns and one of 2
GRID_WAVES = 2048 * 4           # stream_grid's cap (common.hpp) times kWavesPerBlock: more tiles take the grid stride
# the comparison "monoids": add(acc, x) is acc > x, acc < x or acc != x, which is neither associative nor commutative,
# so only the kernel's contract -- a row is folded in CSR order, starting from the identity -- defines the result
ORDERED = ["GreaterPlus", "CustomLessPlus", "NotEqualToPlus", "CustomLessLess"]


def census(ptr):
    """what build_spmv_plan makes of these row pointers: tiles, slice tiles, sliced rows, the slices' lengths,
    all-empty tiles and those of them that start at the end of the arrays"""
    ptr = np.asarray(ptr, dtype=np.int64)
    tiles = wave_tiles(ptr)
    lens = np.diff(ptr)
    long_rows = np.nonzero(lens > TILE)[0]
    slice_lens = [int(min(TILE, lens[r] - s)) for r in long_rows for s in range(0, int(lens[r]), TILE)]
    empty = [(a, b) for a, b, s in tiles if not s and ptr[a] == ptr[b]]
    return dict(ntiles=len(tiles), nslices=sum(1 for _, _, s in tiles if s), nlong=int(long_rows.size),
                slice_lens=slice_lens, nempty=len(empty),
                nempty_at_end=sum(1 for a, _ in empty if ptr[a] == ptr[-1] and ptr[-1] > 0),
                nempty_full=sum(1 for a, b in empty if b - a == TILE_ROWS))


def _assert_rectangular(case):
    """what R and T are for, on top of _skewed's own assertions"""
    assert case.nrows != case.ncols
    for tran in (0, 1):
        assert census(case.arrays(tran, np.zeros(case.nvals))[0])["nslices"] >= 2, (case.name, tran)
    assert any(1 in census(p)["slice_lens"] for p in (case.ptr, case.tptr)), case.name


plain = slc.plain


# _skewed is imported under its private name on purpose: R and T are the SpMV cases' skeleton at other shapes, and its
# assertions (rows of long_len / 512 / 513, empty ends, an all-empty 64-row tile, sliced hub columns) hold for them too
@functools.lru_cache(maxsize=None)
def wide():
    c = slc._skewed("R", 900, 1300, 1025, 130, 8, 5, seed=1)
    _assert_rectangular(c)
    assert census(c.ptr)["slice_lens"] == [512, 512, 1, 512, 1]         # row 7, then row 12 (513 entries)
    assert sorted(c.col_count[c.col_count > TILE].tolist(), reverse=True) == [741, 634, 582]
    return c


@functools.lru_cache(maxsize=None)
def tall():
    c = slc._skewed("T", 1300, 900, 700, 130, 8, 5, seed=1)
    _assert_rectangular(c)
    assert sorted(c.col_count[c.col_count > TILE].tolist(), reverse=True)[:3] == [1128, 970, 884]
    assert 3 in [-(-int(n) // TILE) for n in c.col_count]              # a column of three slices
    return c


@functools.lru_cache(maxsize=None)
def empty():
    c = Case("E", 200, 150, np.zeros(201, dtype=np.int64), np.zeros(0, dtype=np.int64))
    assert c.nvals == 0
    return c


@functools.lru_cache(maxsize=None)
def one():
    rng = np.random.default_rng(20250)
    cols = np.sort(rng.choice(700, 600, replace=False))
    c = Case("One", 1, 700, np.array([0, 600]), cols)
    assert c.nrows == 1 and census(c.ptr)["slice_lens"] == [512, 88]
    assert c.col_count.max() == 1 and np.count_nonzero(c.col_count == 0) == 100    # transposed: 700 rows of <= 1 entry
    return c


@functools.lru_cache(maxsize=None)
def one_transposed():
    o = one()
    c = Case("OneT", 700, 1, o.tptr, o.tind)
    assert c.ncols == 1 and c.nvals == 600 and census(c.tptr)["slice_lens"] == [512, 88]
    return c


def _single_row(name, row):
    nrows, ncols, n = 4 * TILE_ROWS + 1, 200, 100
    rng = np.random.default_rng(20251)
    ptr = np.zeros(nrows + 1, dtype=np.int64)
    ptr[row + 1:] = n
    c = Case(name, nrows, ncols, ptr, np.sort(rng.choice(ncols, n, replace=False)))
    assert np.count_nonzero(np.diff(c.ptr)) == 1 and np.diff(c.ptr)[row] == n
    return c


@functools.lru_cache(maxsize=None)
def first_row_only():
    c = _single_row("First", 0)
    cs = census(c.ptr)
    assert cs["ntiles"] == 5 and cs["nempty"] == 4 and cs["nempty_at_end"] == 4, cs   # the "cnt > 0" special case
    return c


@functools.lru_cache(maxsize=None)
def last_row_only():
    c = _single_row("Last", 4 * TILE_ROWS)
    cs = census(c.ptr)
    assert cs["ntiles"] == 5 and cs["nempty"] == 4 and cs["nempty_full"] == 4 and cs["nempty_at_end"] == 0, cs
    assert wave_tiles(c.ptr)[-1] == (c.nrows - 1, c.nrows, False)       # every tile before the last row's is empty
    return c


@functools.lru_cache(maxsize=None)
def stride():
    nrows, ncols, per = 8300, 600, 257
    rng = np.random.default_rng(20252)
    ind = np.sort(np.argpartition(rng.random((nrows, ncols)), per - 1, axis=1)[:, :per], axis=1)
    c = Case("S", nrows, ncols, np.arange(nrows + 1, dtype=np.int64) * per, ind.ravel())
    assert 2 * per > TILE                                               # two rows do not fit one tile
    assert len(wave_tiles(c.ptr)) == nrows and len(wave_tiles(c.ptr)) > GRID_WAVES
    assert per * 4 * 1000 < slc.EXACT                                   # values <= 4, B <= 1000: every sum is exact
    return c


CASES = {"P": plain, "R": wide, "T": tall, "E": empty, "One": one, "OneT": one_transposed, "First": first_row_only,
         "Last": last_row_only, "S": stride}


# ---- operands ------------------------------------------------------------------------------------------------------
def _kind(sr):
    """the semirings that draw their own data: PlusDivides its vector, MultipliesMultiplies values and vector"""
    return sr if sr in ("PlusDivides", "MultipliesMultiplies") else "any"


@functools.lru_cache(maxsize=None)
def _values(name, kind):
    v = values(CASES[name](), kind, False)
    v.setflags(write=False)
    return v


def matrix_values(case, sr):
    """the stored values as integers (CSR order); one set for MultipliesMultiplies, one for everything else"""
    return _values(case.name, "MultipliesMultiplies" if sr == "MultipliesMultiplies" else "any")


@functools.lru_cache(maxsize=None)
def _rhs(name, tran, kind, k):
    case = CASES[name]()
    B = np.stack([vector(case, tran, kind, attempt=c) for c in range(k)], axis=1).astype(np.int64)
    B.setflags(write=False)
    return B


def rhs(case, tran, sr, k=KMAX):
    """B as integers, [rows of the input, k]: column c is vector(case, tran, sr, attempt=c)"""
    return _rhs(case.name, int(tran), _kind(sr), k)


# ---- references ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _expected(name, tran, sr, dtype):
    case = CASES[name]()
    vals, B = matrix_values(case, sr), rhs(case, tran, sr)
    out = np.stack([want(case, tran, sr, dtype, vals, B[:, c]) for c in range(KMAX)], axis=1)
    out.setflags(write=False)
    return out


def expected(case, tran, sr, dtype, k):
    """C = op(A) (+.x) B[:, :k] by slc.want column by column (rows folded in float64 / int64, exactness asserted):
    computed once at k = 130 per (case, orientation, semiring, type) and sliced"""
    assert 1 <= k <= KMAX
    return np.ascontiguousarray(_expected(case.name, int(tran), sr, dtype)[:, :k])


def fold_in_order(sr, ptr, ind, val, B, dtype, rows=None):
    """The kernel's contract for a row that fits a tile: acc = add(acc, mul(a, b)) over the row's entries in CSR
    order, from the identity, in the type itself -- vectorised over the rows by position in the row.  `rows` limits
    the fold to these rows; the others keep the identity."""
    ptr = np.asarray(ptr, dtype=np.int64)
    lens = np.diff(ptr)
    val, B = np.asarray(val).astype(dtype), np.asarray(B).astype(dtype)
    out = np.full((lens.size, B.shape[1]), sr.identity(), dtype=dtype)
    rows = np.arange(lens.size) if rows is None else np.asarray(rows)
    rows = rows[np.argsort(-lens[rows], kind="stable")]                 # longest first: the rows with len > p lead
    neg = -lens[rows]
    for p in range(int(lens[rows].max()) if rows.size else 0):
        act = rows[:np.searchsorted(neg, -p, side="left")]
        q = ptr[act] + p
        out[act] = sr.add_op(out[act], sr.mul_op(val[q][:, None], B[ind[q]]))
    return out


def tile_rows(ptr):
    """the rows of at most 512 entries: those a tile folds whole, in CSR order"""
    return np.nonzero(np.diff(np.asarray(ptr, dtype=np.int64)) <= TILE)[0]


@functools.lru_cache(maxsize=None)
def _expected_in_order(name, tran, sr, dtype):
    case = CASES[name]()
    vals, B = matrix_values(case, sr), rhs(case, tran, sr)
    ptr, ind, v, nout, nin = case.arrays(tran, vals)
    rows = tile_rows(ptr)
    # A row of more than 512 entries is folded slice by slice and the slices' partial results are folded again; with
    # an add that is not associative no reference defines that value, so those rows are left out of the comparison.
    if name in ("P", "R", "T"):
        assert rows.size >= nout - 8, (name, tran, rows.size)
    out = fold_in_order(Semiring(sr, dtype), ptr, ind, v, B, dtype, rows)
    out.setflags(write=False)
    return rows, out


def expected_in_order(case, tran, sr, dtype, k):
    """(rows compared, C) of the sequential fold; C's other rows are meaningless"""
    assert 1 <= k <= KMAX
    rows, out = _expected_in_order(case.name, int(tran), sr, dtype)
    return rows, np.ascontiguousarray(out[:, :k])


def expected_stride(sr, dtype, k):
    """S: every row has 257 entries, so the fold by position is 257 steps over all rows at once"""
    case = stride()
    return fold_in_order(Semiring(sr, dtype), case.ptr, case.ind, matrix_values(case, sr), rhs(case, 0, sr, 70)[:, :k], dtype)


# ---- real values (the one place where sums round) ------------------------------------------------------------------
def _uniform(seed, shape):
    x = (0.5 + 0.5 * np.random.default_rng(seed).random(shape)).astype(np.float32)
    x = np.minimum(x, np.float32(1 - 2.0 ** -24))                       # a draw that rounds up to 1.0 stays below it
    assert x.min() >= 0.5 and x.max() < 1
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def real_values(name):
    """stored values (CSR order) as float32, uniform in [0.5, 1)"""
    return _uniform(slc._seed(name, "real values"), CASES[name]().nvals)


@functools.lru_cache(maxsize=None)
def real_rhs(name, tran, k):
    """B as float32, uniform in [0.5, 1): every product with a stored value is at least 0.25"""
    case = CASES[name]()
    return _uniform(slc._seed(name, "real rhs", tran, k), (case.nrows if tran else case.ncols, k))


def real_product(case, tran, vals, B):
    """(the product in float64, the bound of its float32 evaluation in ANY order, with or without FMA):
    |err| <= gamma_n * sum |a b|,  gamma_n = n u / (1 - n u),  u = 2^-24,  n = the row's length (Higham, Accuracy and
    Stability of Numerical Algorithms, 2nd ed., (3.5) with the n products' own roundings absorbed: n - 1 additions and
    one multiplication make at most n roundings on any path from a product to the root)"""
    ptr, ind, v, nout, nin = case.arrays(tran, np.asarray(vals))
    ptr = ptr.astype(np.int64)
    prod = v.astype(np.float64)[:, None] * np.asarray(B, dtype=np.float64)[ind]
    exact = np.zeros((nout, B.shape[1]))
    nz = np.diff(ptr) > 0
    exact[nz] = np.add.reduceat(prod, ptr[:-1][nz], axis=0)             # all products positive: this is sum |a b| too
    n = np.diff(ptr).astype(np.float64)[:, None]
    u = 2.0 ** -24
    return exact, n * u / (1 - n * u) * exact
