"""GPU suite (-m gpu): grb_spmm (csrc/spmm.hip) where its paths part -- rows cut into slices, the three column-group
instantiations and every width at which run_tiles changes its launches, rectangular matrices in both orientations,
all-empty tiles, an empty matrix, more tiles than a full grid has waves -- against the host references of
tests/spmm_cases.py (pinned without a GPU by tests/test_spmm_reference.py).

The data are exact in float32 and int32 in any order of summation, so everything but the one test on real values is
compared bit for bit.  B and C lie between guard elements; C is filled, payload included, with a sentinel that no
expected value takes, so an element the kernels fail to write cannot pass for a result left over from another call."""
import numpy as np
import pytest
import torch

import spmm_cases as sc
from oracle.semiring import Semiring

pytestmark = pytest.mark.gpu
IDS = ["f32", "i32"]
GUARD = 64                                  # elements before and after each payload
NAN_BITS = 0x7FC12345                       # f32 sentinel: a quiet NaN with a payload of its own
INT_SENTINEL = -123456789                   # i32 sentinel
WIDTHS = [5, 17, 32, 33, 81, 130]


def _sentinel_bits(dtype):
    return NAN_BITS if dtype is np.float32 else INT_SENTINEL


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Buffers:
    """B and C on the device, each with GUARD sentinel elements on both sides"""

    def __init__(self, B, nout, k, dtype):
        dev = torch.device("cuda", 0)
        B = np.ascontiguousarray(B, dtype=dtype)
        assert B.ndim == 2 and B.shape[1] == k
        self.dtype, self.nout, self.k, self.nb = dtype, nout, k, B.size
        self.fill = _sentinel_bits(dtype)
        host_b = np.full(B.size + 2 * GUARD, self.fill, dtype=np.int32)
        host_b[GUARD:GUARD + B.size] = _bits(B).ravel()
        self.b_bits = host_b
        self.tb = torch.from_numpy(host_b).to(dev)
        self.tc = torch.full((nout * k + 2 * GUARD,), self.fill, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        self.pb = self.tb.data_ptr() + 4 * GUARD
        self.pc = self.tc.data_ptr() + 4 * GUARD

    def result(self, what):
        """C's payload after the call; both guards of C, and all of B, must be as they were"""
        torch.cuda.synchronize()
        c = self.tc.cpu().numpy()
        assert np.all(c[:GUARD] == self.fill) and np.all(c[-GUARD:] == self.fill), ("C's guards were written", what)
        assert np.array_equal(self.tb.cpu().numpy(), self.b_bits), ("B was written", what)
        return c[GUARD:GUARD + self.nout * self.k].reshape(self.nout, self.k)

    def untouched(self, what):
        assert np.all(self.result(what) == self.fill), ("C was written", what)


def spmm_bits(g, A, sr, B, nout, tran, dtype, what):
    """the bits of C = op(A) (+.x) B, return code, sentinel and guards checked"""
    bufs = Buffers(B, nout, B.shape[1], dtype)
    info = g.spmm(sr, A, bufs.pb, bufs.pc, B.shape[1], None, tran=bool(tran))
    assert info == 0, (info, what)
    got = bufs.result(what)
    left = np.argwhere(got == bufs.fill)
    assert left.size == 0, ("%d elements of C were never written, first (row, column) %s" % (len(left), left[:4].tolist()), what)
    return got


def check(g, A, sr, B, want, tran, dtype, what, rows=None):
    """C against `want`, bit for bit (on `rows` only, if given)"""
    want = np.ascontiguousarray(want, dtype=dtype)
    if dtype is np.int32:
        assert not np.any(want == INT_SENTINEL), what
    else:
        assert not np.any(np.isnan(want)), what
    got = spmm_bits(g, A, sr, B, want.shape[0], tran, dtype, what)
    wb = _bits(want)
    if rows is not None:
        got, wb, want = got[rows], wb[rows], want[rows]
    bad = np.argwhere(got != wb)
    assert bad.size == 0, "%s: %d elements differ, first (row, column) %s: got %s, want %s" % (
        what, len(bad), bad[:4].tolist(), got.view(dtype)[tuple(bad[:4].T)], want[tuple(bad[:4].T)])


@pytest.fixture(scope="module")
def g():
    import graphblast_amd
    return graphblast_amd


@pytest.fixture(scope="module")
def mats(g):
    """one Matrix per (case, set of values, type), built on first use"""
    made = {}

    def get(case, sr, dtype):
        vals = sc.matrix_values(case, sr)
        key = (case.name, sr == "MultipliesMultiplies", dtype)
        if key not in made:
            A = g.Matrix(case.nrows, case.ncols, dtype)
            assert A.build_csr(case.ptr, case.ind, vals.astype(dtype)) == 0
            made[key] = A
        return made[key]
    return get


def shapes(case, tran):
    """(rows of C, rows of B): B has ncols rows for tran = 0 and nrows rows for tran = 1, C the other count"""
    return (case.ncols, case.nrows) if tran else (case.nrows, case.ncols)


def check_exact_case(g, mats, case, sr, dtype, widths, trans=(0, 1)):
    A = mats(case, sr, dtype)
    for tran in trans:
        nout, nin = shapes(case, tran)
        B = sc.rhs(case, tran, sr)
        assert B.shape[0] == nin
        for k in widths:
            want = sc.expected(case, tran, sr, dtype, k)
            assert want.shape == (nout, k)
            check(g, A, sr, B[:, :k], want, tran, dtype, (case.name, sr, dtype.__name__, "tran=%d" % tran, "k=%d" % k))


# ---- 1. every semiring on long rows -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("sr", sc.COMMUTATIVE)
@pytest.mark.parametrize("name", ["P", "R", "T"])
def test_every_semiring_on_sliced_rows(g, mats, name, sr, dtype):
    """rows of 1000 / 1025 / 700, 512 and 513 entries and the hub columns of the transposed orientation (slices, the
    partial vectors and their fold), an all-empty tile, empty first and last rows; R and T are rectangular, so a
    mix-up of nrows and ncols under tran = 1 reads or writes the wrong count of rows"""
    check_exact_case(g, mats, sc.CASES[name](), sr, dtype, WIDTHS)


# ---- 2. every width at which run_tiles changes its launches -----------------------------------------------------------
# k               launches (KG, col0) of run_tiles
# 1, 15, 16       (16, 0)                                  four lane groups, four rows at a time
# 17, 31, 32      (32, 0)                                  two lane groups, two rows at a time
# 33, 48, 63      (64, 0)                                  one group, lanes k .. 63 idle
# 64              (64, 0)
# 65, 80          (64, 0) (16, 64)                         remainder 1 / 16
# 81, 96          (64, 0) (32, 64)                         remainder 17 / 32
# 97, 127         (64, 0) (64, 64)                         remainder 33 / 63: the second launch partly filled
# 128             (64, 0) (64, 64)
# 129, 130        (64, 0) (64, 64) (16, 128)               remainder 1 / 2
BOUNDARY_WIDTHS = [1, 15, 16, 17, 31, 32, 33, 48, 63, 64, 65, 80, 81, 96, 97, 127, 128, 129, 130]


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("sr", ["PlusMultiplies", "MinimumPlus", "LogicalOrAnd"])
def test_every_width_boundary(g, mats, sr, dtype):
    check_exact_case(g, mats, sc.wide(), sr, dtype, BOUNDARY_WIDTHS)


# ---- 3. the order-dependent "monoids" ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("sr", sc.ORDERED)
@pytest.mark.parametrize("name", ["P", "R"])
def test_ordered_semirings_fold_in_csr_order(g, mats, name, sr, dtype):
    """add = greater / less / not_equal_to: the rows a tile folds whole are compared with the sequential fold in CSR
    order.  The rows of more than 512 entries are left out (expected_in_order says why); at least nrows - 8 remain."""
    case = sc.CASES[name]()
    A = mats(case, sr, dtype)
    for tran in (0, 1):
        nout, nin = shapes(case, tran)
        B = sc.rhs(case, tran, sr)
        for k in (5, 17, 70, 81):
            rows, want = sc.expected_in_order(case, tran, sr, dtype, k)
            assert want.shape == (nout, k) and rows.size >= nout - 8
            check(g, A, sr, B[:, :k], want, tran, dtype, (name, sr, dtype.__name__, "tran=%d" % tran, "k=%d" % k), rows)


# ---- 4. degenerate shapes ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
def test_empty_matrix_gives_the_identity(g, mats, dtype):
    case = sc.empty()
    A = mats(case, "PlusMultiplies", dtype)
    assert A.nvals() == 0
    for sr in ("PlusMultiplies", "MinimumPlus", "MultipliesMultiplies"):       # identities 0, the type's maximum, 1
        ident = Semiring(sr, dtype).identity()
        for tran in (0, 1):
            nout, nin = shapes(case, tran)
            for k in (1, 40):
                B = sc.rhs(case, tran, sr, 40)[:, :k]
                check(g, A, sr, B, np.full((nout, k), ident, dtype=dtype), tran, dtype, ("E", sr, tran, k))
    assert len({float(Semiring(s, dtype).identity()) for s in ("PlusMultiplies", "MinimumPlus", "MultipliesMultiplies")}) == 3


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["One", "OneT", "First", "Last"])
def test_single_rows(g, mats, name, dtype):
    """One: nrows = 1, a row of two slices; transposed (and OneT the other way round) 700 rows of at most one entry.
    First / Last: entries in the first / the last row only -- all-empty tiles that start at the end of the arrays,
    and four all-empty tiles before the only entries."""
    for sr in ("PlusMultiplies", "MinimumPlus", "MultipliesMultiplies"):
        check_exact_case(g, mats, sc.CASES[name](), sr, dtype, (1, 17, 70))


# ---- 5. more tiles than the grid has waves -----------------------------------------------------------------------------
@pytest.mark.parametrize("sr", ["PlusMultiplies", "MinimumPlus"])
def test_grid_stride(g, mats, sr):
    """S: 8300 tiles for the 8192 waves of the largest grid, so the first 108 waves take a second tile"""
    case, dtype = sc.stride(), np.float32
    assert len(sc.wave_tiles(case.ptr)) > sc.GRID_WAVES
    A = mats(case, sr, dtype)
    B = sc.rhs(case, 0, sr, 70)
    for k in (5, 70):
        check(g, A, sr, B[:, :k], sc.expected_stride(sr, dtype, k), 0, dtype, ("S", sr, k))


# ---- 6. real values ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def real_matrix(g):
    case = sc.wide()
    A = g.Matrix(case.nrows, case.ncols, np.float32)
    assert A.build_csr(case.ptr, case.ind, sc.real_values("R")) == 0
    return A


@pytest.mark.parametrize("k", [17, 81])
def test_real_values_plus_multiplies_within_the_rounding_bound(g, real_matrix, k):
    """f32 values and B uniform in [0.5, 1) against the float64 product.  The bound is derived, not measured: any order
    of summation of n rounded products, with or without FMA, satisfies |err| <= gamma_n * sum |a b| with gamma_n =
    n u / (1 - n u), u = 2^-24, n the row's length (sc.real_product).  Every product is at least 0.25, so a dropped or a
    doubled entry is far outside it."""
    case, vals = sc.wide(), sc.real_values("R")
    for tran in (0, 1):
        B = sc.real_rhs("R", tran, k)
        exact, bound = sc.real_product(case, tran, vals, B)
        # the bound tells a wrong result from a right one: one entry dropped from every non-empty row is outside it
        ptr, ind, v, nout, nin = case.arrays(tran, vals)
        nz = np.nonzero(np.diff(ptr))[0]
        dropped = exact.copy()
        dropped[nz] -= v[ptr[nz]].astype(np.float64)[:, None] * B[ind[ptr[nz]]].astype(np.float64)
        assert np.all(np.abs(dropped.astype(np.float32).astype(np.float64) - exact)[nz] > 3 * bound[nz])
        got = spmm_bits(g, real_matrix, "PlusMultiplies", B, nout, tran, np.float32, ("real", tran, k)).view(np.float32)
        err = np.abs(got.astype(np.float64) - exact)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print("real values, tran=%d k=%d: largest error %.3g, bound there %.3g" % (tran, k, err[worst], bound[worst]))
        assert np.all(err <= bound), (tran, k, worst, got[worst], exact[worst], bound[worst])


@pytest.mark.parametrize("k", [17, 81])
def test_real_values_min_and_max_are_exact(g, real_matrix, k):
    """minimum and maximum do not round, so a + b and a * b taken in float32 on the host give the result in any order;
    MinimumPlus also with a tenth of B at +inf"""
    case, vals = sc.wide(), sc.real_values("R")
    for tran in (0, 1):
        ptr, ind, v, nout, nin = case.arrays(tran, vals)
        B = sc.real_rhs("R", tran, k)
        Binf = B.copy()
        Binf[np.random.default_rng(k + tran).random(B.shape) < 0.1] = np.inf
        for sr, rhs in (("MinimumPlus", B), ("MaximumMultiplies", B), ("MinimumPlus", Binf)):
            want = sc.fold_in_order(Semiring(sr, np.float32), ptr, ind, v, rhs, np.float32)
            check(g, real_matrix, sr, rhs, want, tran, np.float32, ("real", sr, tran, k, "inf" if rhs is Binf else ""))


# ---- 7. results of other operations as the left operand ----------------------------------------------------------------
def _random_csr(rng, nrows, ncols, per_row):
    ind = np.sort(np.argpartition(rng.random((nrows, ncols)), per_row - 1, axis=1)[:, :per_row], axis=1)
    return np.arange(nrows + 1, dtype=np.int32) * per_row, ind.ravel().astype(np.int32)


def _check_host_copy(g, M, dtype, k, what):
    """spmm on M against the fold over M's own host copy; small integers, so exact in any order"""
    ptr, ind, val = M.host_csr()
    rng = np.random.default_rng(77)
    B = rng.integers(0, 4, (M.ncols(), k))
    rows = np.repeat(np.arange(M.nrows()), np.diff(ptr))
    assert np.bincount(rows, np.abs(val.astype(np.float64)) * 3, minlength=M.nrows()).max() < sc.slc.EXACT
    for sr in ("PlusMultiplies", "MinimumPlus"):
        want = sc.fold_in_order(Semiring(sr, dtype), ptr, ind, val, B, dtype)
        check(g, M, sr, B.astype(dtype), want, 0, dtype, (what, sr, k))
    return ptr


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
def test_on_the_result_of_a_masked_mxm(g, dtype):
    """C<P> = A (+.x) B has P's structure (rows of 1000, 513 and 512 entries) and CSR only: its plan is built by the
    first product that needs it, and the transposed product has nothing to run on"""
    P = sc.plain()
    rng = np.random.default_rng(41)
    n = P.nrows
    d = g.Descriptor()
    assert d.loadArgs() == 0
    Mk, A, Bm, Cm = (g.Matrix(n, n, dtype) for _ in range(4))
    assert Mk.build_csr(P.ptr, P.ind, np.ones(P.nvals, dtype=dtype)) == 0
    for X in (A, Bm):
        ptr, ind = _random_csr(rng, n, n, 30)
        assert X.build_csr(ptr, ind, rng.integers(1, 4, ind.size).astype(dtype)) == 0
    assert g.mxm(Cm, Mk, None, "PlusMultiplies", A, Bm, d) == 0
    for k in (17, 70):
        ptr = _check_host_copy(g, Cm, dtype, k, "mxm result")
        assert np.array_equal(ptr, P.ptr)
    assert np.count_nonzero(Cm.host_csr()[2]) > P.nvals // 4               # the product is not all zeros
    bufs = Buffers(np.ones((n, 5), dtype=dtype), n, 5, dtype)
    assert g.spmm("PlusMultiplies", Cm, bufs.pb, bufs.pc, 5, None, tran=True) == g.GrB_INVALID_OBJECT
    bufs.untouched("tran = 1 without a CSC")


@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
def test_on_the_result_of_transpose(g, mats, dtype):
    R = sc.wide()
    d = g.Descriptor()
    assert d.loadArgs() == 0
    Tr = g.Matrix(R.ncols, R.nrows, dtype)
    assert g.transpose(Tr, None, None, mats(R, "PlusMultiplies", dtype), d) == 0
    for k in (17, 70):
        ptr = _check_host_copy(g, Tr, dtype, k, "transpose result")
        assert np.array_equal(ptr, R.tptr)


# ---- 8. argument checks ------------------------------------------------------------------------------------------------
def test_argument_checks_leave_c_alone(g, mats):
    """return codes on valid memory: nothing here passes a bad device pointer"""
    case, dtype = sc.wide(), np.float32
    A = mats(case, "PlusMultiplies", dtype)
    unbuilt = g.Matrix(case.nrows, case.ncols, dtype)
    bufs = Buffers(np.ones((case.ncols, 5), dtype=dtype), case.nrows, 5, dtype)
    sr = "PlusMultiplies"
    for k in (0, -1):
        assert g.spmm(sr, A, bufs.pb, bufs.pc, k, None) == g.GrB_INVALID_VALUE
        bufs.untouched(("k", k))
    assert g.spmm(sr, A, None, bufs.pc, 5, None) == g.GrB_UNINITIALIZED_OBJECT
    bufs.untouched("null B")
    assert g.spmm(sr, A, bufs.pb, None, 5, None) == g.GrB_UNINITIALIZED_OBJECT
    bufs.untouched("null C")
    assert g.spmm(sr, None, bufs.pb, bufs.pc, 5, None) == g.GrB_UNINITIALIZED_OBJECT
    bufs.untouched("null matrix")
    assert g.spmm(sr, unbuilt, bufs.pb, bufs.pc, 5, None) == g.GrB_UNINITIALIZED_OBJECT
    bufs.untouched("unbuilt matrix")
    # the same buffers still serve a good call
    assert g.spmm(sr, A, bufs.pb, bufs.pc, 5, None) == 0
    assert not np.any(bufs.result("good call") == bufs.fill)
