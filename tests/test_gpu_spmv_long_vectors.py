"""The generic SpMV (csrc/spmv.hip k_spmv) on input vectors longer than its LDS prefix of 32768 values, through
grb_mxv / grb_vxm, against the host reference of tests/spmv_long_cases.py: every commutative semiring, float32 and
int32, mask / scmp / accumulate with a float and an integer mask, on each route the kernel choice can take --

  route 1  vector <= 32768: whole vector in LDS, natural column ids          P, and vxm on W
  route 2  longer, skewed: columns renamed by rank, hot prefix + cold gathers  mxv on W, format 0 (CSR kernel)
  route 3  longer, flat: every gather cold, natural ids (nhot == 0)           mxv on N
  route 4  as 2 in the column-sorted format (spmv_cband.hpp)                   mxv on W, format 1; vxm, format 2

Each test asserts the route it means to take (spmv_plan_info / spmv_format_info) next to the values.  The data are
exact in float32 and int32 in any order of summation, so everything is compared bit for bit; the one float case
says so.  The settings of the format and of its amortisation rule are restored by a fixture whatever happens."""
import numpy as np
import pytest

import spmv_long_cases as slc

pytestmark = pytest.mark.gpu
IDS = ["f32", "i32"]
GrB_MASK, GrB_SCMP = 0, 0                   # graphblast_amd.api: descriptor field and value


@pytest.fixture
def fmt():
    """sets grb_spmv_set_format / grb_spmv_set_reuse_threshold for one test and puts both back"""
    import graphblast_amd as g
    before = (g.spmv_set_format(-1), g.spmv_set_reuse_threshold(-1))

    def choose(setting, threshold=None):
        g.spmv_set_format(setting)
        if threshold is not None:
            g.spmv_set_reuse_threshold(threshold)
        return g
    yield choose
    g.spmv_set_format(before[0])
    g.spmv_set_reuse_threshold(before[1])


@pytest.fixture(scope="module")
def mats():
    """matrices on the device, built once per (pattern, semiring, type, purpose): a matrix keeps the state of its
    plans (renamed columns, the column-sorted copy, the product counter), so every test that asserts a route has
    its own"""
    import graphblast_amd as g
    made = {}

    def get(case, sr, dtype, purpose, iso=False):
        key = (case.name, sr, dtype, purpose, iso)
        if key not in made:
            A = g.Matrix(case.nrows, case.ncols, dtype)
            assert A.build_csr(case.ptr, case.ind, slc.values(case, sr, iso).astype(dtype)) == 0
            made[key] = A
        return made[key]
    return get


def product(g, A, case, tran, sr, dtype, u, variant="none", mask=None, mask_dtype=np.float32, w0=None):
    """w = A u (tran = 0, grb_mxv) or u A (tran = 1, grb_vxm) on the pull path, w starting from w0"""
    use_mask, scmp, accum = slc.VARIANTS[variant]
    nin, nout = (case.nrows, case.ncols) if tran else (case.ncols, case.nrows)
    d = g.Descriptor()
    assert d.loadArgs(mxvmode=2, fusedmask=0) == 0
    if scmp:
        assert d.set(GrB_MASK, GrB_SCMP) == 0
    uv, w = g.Vector(nin, dtype), g.Vector(nout, dtype)
    assert uv.build(np.asarray(u).astype(dtype), nin) == 0
    assert w.build((np.full(nout, -7) if w0 is None else np.asarray(w0)).astype(dtype), nout) == 0
    mk = None
    if use_mask:
        mk = g.Vector(nout, mask_dtype)
        assert mk.build(np.asarray(mask).astype(mask_dtype), nout) == 0
    acc = "accum" if accum else None
    info = g.vxm(w, mk, acc, sr, uv, A, d) if tran else g.mxv(w, mk, acc, sr, A, uv, d)
    assert info == 0, info
    assert d.lastmxv_ == 12                                     # GrB_PULLONLY: the SpMV, not the push
    info, got = w.extractTuples()
    assert info == 0
    return got


def check(g, A, case, tran, sr, dtype, variants, iso=False, what=""):
    """every (variant, mask type) against the reference, bit for bit"""
    vals, u, w0, mask = slc.operands(case, tran, sr, iso)
    for variant in variants:
        use_mask, scmp, accum = slc.VARIANTS[variant]
        for mask_dtype in ((np.float32, np.int32) if use_mask else (np.float32,)):
            got = product(g, A, case, tran, sr, dtype, u, variant, mask, mask_dtype, w0)
            ref = slc.want(case, tran, sr, dtype, vals, u, mask if use_mask else None, scmp, accum, w0)
            bad = np.nonzero(got != ref)[0]
            assert got.dtype == ref.dtype
            assert bad.size == 0, "%s: %s %s %s %s %s, %s mask, %s: %d rows differ, first %s: got %s, want %s" % (
                what, case.name, "vxm" if tran else "mxv", sr, dtype.__name__, variant, mask_dtype.__name__,
                "iso" if iso else "valued", bad.size, bad[:4], got[bad[:4]], ref[bad[:4]])


ALL_VARIANTS = ["none", "mask", "scmp", "accum", "scmp+accum"]


# ---- route 2 (and 1 as the control): the CSR kernel ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", slc.DTYPES, ids=IDS)
@pytest.mark.parametrize("sr", slc.COMMUTATIVE)
def test_csr_kernel_hot_prefix_and_cold_gathers(fmt, mats, sr, dtype):
    """format 0.  mxv on W: columns renamed by rank, 32768 values in LDS, the rest gathered from memory; vxm on W
    and both products on P: the whole vector in LDS.  Long-row slices (1300 = 512 + 512 + 276, 513, the hub columns
    of the transposed orientation), a row of exactly 512, empty rows at both ends, an all-empty tile."""
    g = fmt(0)
    W, P = slc.wide(), slc.plain()
    A_w, A_p = mats(W, sr, dtype, "csr"), mats(P, sr, dtype, "csr")
    info = g.spmv_plan_info(A_w, 0, warm=True)
    assert info["nhot"] == slc.HOT and info["bands"] == 1, info
    assert g.spmv_plan_info(A_w, 1, warm=True)["nhot"] == W.nrows
    assert g.spmv_plan_info(A_p, 0, warm=True)["nhot"] == P.ncols and g.spmv_plan_info(A_p, 1, warm=True)["nhot"] == P.nrows
    for case, A in ((P, A_p), (W, A_w)):
        for tran in (0, 1):
            check(g, A, case, tran, sr, dtype, ALL_VARIANTS, what="csr kernel")
            assert g.spmv_format_info(A, tran)["in_use"] == 0


# ---- the two ways of ranking the columns -------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", slc.DTYPES, ids=IDS)
def test_ranking_by_transposed_pointers_and_by_histogram(fmt, dtype):
    """device_rank_columns counts a column's references from the row pointers of the other orientation when the
    matrix has one (build_csr: ops.hip passes other_ptr) and by a histogram of the column ids when it has not
    (build_device_csr without a CSC); ties may rank differently, the products may not"""
    g = fmt(0)
    W = slc.wide()

    def on_device(a):                       # caller-owned device storage: a dense vector's buffer
        v = g.Vector(a.size, a.dtype.type)
        assert v.build(a, a.size) == 0
        return v, v.device_ptrs()[2]
    for sr in ("PlusMultiplies", "MinimumPlus", "PlusMinus"):
        vals = slc.values(W, sr, False).astype(dtype)
        both = g.Matrix(W.nrows, W.ncols, dtype)
        assert both.build_csr(W.ptr, W.ind, vals) == 0
        keep, ptrs = zip(*(on_device(a) for a in (W.ptr, W.ind, vals)))
        only = g.Matrix(W.nrows, W.ncols, dtype)
        assert only.build_device_csr(ptrs[0], ptrs[1], ptrs[2], W.nvals, keep=keep) == 0
        for A, how in ((both, "pointers"), (only, "histogram")):
            info = g.spmv_plan_info(A, 0, warm=True)
            assert info["nhot"] == slc.HOT and info["bands"] == 1, (how, info)
            check(g, A, W, 0, sr, dtype, ["none", "scmp+accum"], what=how)


# ---- route 3: flat column counts ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [0, 1], ids=["csr", "auto"])
@pytest.mark.parametrize("dtype", slc.DTYPES, ids=IDS)
def test_flat_matrix_gathers_everything_cold(fmt, mats, dtype, setting):
    """N: the 32768 most referenced columns hold 32768 of 300000 entries, less than 1/8: no renaming, nhot == 0,
    and `auto` leaves such an orientation to the CSR kernel however often it is multiplied"""
    g = fmt(setting, 0)
    N = slc.flat()
    A = mats(N, "PlusMultiplies", dtype, ("flat", setting))
    assert g.spmv_plan_info(A, 0, warm=True)["nhot"] == 0
    for sr in slc.COMMUTATIVE:
        B = A if sr != "MultipliesMultiplies" else mats(N, sr, dtype, ("flat", setting))
        check(g, B, N, 0, sr, dtype, ["none", "scmp+accum"], what="flat")
        assert g.spmv_plan_info(B, 0)["nhot"] == 0 and g.spmv_format_info(B, 0)["in_use"] == 0
    check(g, A, N, 1, "PlusMultiplies", dtype, ["none", "scmp+accum"], what="flat, transposed")
    assert g.spmv_plan_info(A, 1)["nhot"] == N.nrows


# ---- route 4: the column-sorted kernels --------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", slc.DTYPES, ids=IDS)
@pytest.mark.parametrize("sr", slc.COMMUTATIVE)
def test_column_sorted_kernels(fmt, mats, sr, dtype):
    """`auto` at the first product: spmv_cband_kernel<SR, T, iso> on W for every commutative semiring -- four of them
    with a multiply whose operand order matters, the iso variant rebuilding the matrix operand from one value --
    then the transposed orientation forced into the format (format 2) through vxm"""
    g = fmt(1, 0)
    W = slc.wide()
    variants = ["none", "mask", "scmp+accum"]
    twins = [(iso, mats(W, sr, dtype, "cband", iso)) for iso in (False, True)]
    for iso, A in twins:
        check(g, A, W, 0, sr, dtype, variants[:1], iso, what="column-sorted, first product")
        info = g.spmv_format_info(A, 0)
        assert info["in_use"] == 1 and info["iso"] == int(iso), info
        check(g, A, W, 0, sr, dtype, variants[1:], iso, what="column-sorted")
        assert g.spmv_format_info(A, 1)["in_use"] == 0          # vxm's orientation has a short vector: not `auto`'s
    fmt(2)
    for iso, A in twins:
        check(g, A, W, 1, sr, dtype, variants, iso, what="column-sorted, transposed")
        info = g.spmv_format_info(A, 1)
        assert info["in_use"] == 1 and info["iso"] == int(iso), info


# ---- the switch from the CSR kernel to the format ----------------------------------------------------------------------
def test_switch_after_the_threshold_counts_each_orientation_alone(fmt):
    """format `auto`, threshold 3: three products through the CSR kernel (renamed columns), the fourth prepares the
    column-sorted copy and frees the renamed ids; same values on both sides.  The counter is the orientation's own:
    W' (40000 x 3000, W's CSC as its CSR) has the long vector on the vxm side -- products of the other orientation
    do not count towards it, and it switches after three vxm of its own."""
    g = fmt(1, 3)
    W = slc.wide()
    sr, dtype = "PlusMinus", np.float32
    vals, u, w0, mask = slc.operands(W, 0, sr)
    ref = slc.want(W, 0, sr, dtype, vals, u, mask, 0, 1, w0)
    A = g.Matrix(W.nrows, W.ncols, dtype)
    assert A.build_csr(W.ptr, W.ind, vals.astype(dtype)) == 0
    for launch in range(1, 6):
        got = product(g, A, W, 0, sr, dtype, u, "mask+accum", mask, np.int32, w0)
        assert np.array_equal(got, ref), launch
        assert g.spmv_format_info(A, 0)["in_use"] == (1 if launch >= 4 else 0), launch
        assert g.spmv_format_info(A, 1)["in_use"] == 0
    # the transposed twin: mxv has the short vector, vxm the long one
    T = slc.Case("W'", W.ncols, W.nrows, W.tptr, W.tind)
    B = g.Matrix(T.nrows, T.ncols, dtype)
    assert B.build_csr(T.ptr, T.ind, vals[W.perm].astype(dtype)) == 0
    ut = slc.vector(W, 1, sr)
    ref_mxv = slc.want(W, 1, sr, dtype, vals, ut)               # W' ut == ut W
    for _ in range(4):
        assert np.array_equal(product(g, B, T, 0, sr, dtype, ut), ref_mxv)
    assert g.spmv_format_info(B, 0)["in_use"] == 0 and g.spmv_format_info(B, 1)["in_use"] == 0
    assert g.spmv_plan_info(B, 1, warm=True)["nhot"] == slc.HOT
    for launch in range(1, 6):
        got = product(g, B, T, 1, sr, dtype, u, "mask+accum", mask, np.float32, w0)
        assert np.array_equal(got, ref), launch
        assert g.spmv_format_info(B, 1)["in_use"] == (1 if launch >= 4 else 0), launch
        assert g.spmv_format_info(B, 0)["in_use"] == 0


# ---- the one float case -------------------------------------------------------------------------------------------------
def test_real_valued_sums_on_both_formats(fmt):
    """PlusMultiplies on W with uniform random float32 values and vector against the float64 reference at the
    project's bar (rtol 1e-5, atol 1e-6), through the CSR kernel and through the column-sorted one;
    the CSR kernel sums in a fixed order: a repeat is bit-equal"""
    W = slc.wide()
    rng = np.random.default_rng(6)
    vals = rng.random(W.nvals, dtype=np.float32) + np.float32(0.25)
    u = rng.random(W.ncols, dtype=np.float32)
    ref = np.add.reduceat(np.append(vals.astype(np.float64) * u.astype(np.float64)[W.ind], 0.0), W.ptr[:-1])
    ref[np.diff(W.ptr) == 0] = 0.0
    for setting, in_use in ((0, 0), (1, 1)):
        g = fmt(setting, 0)
        A = g.Matrix(W.nrows, W.ncols, np.float32)
        assert A.build_csr(W.ptr, W.ind, vals) == 0
        got = product(g, A, W, 0, "PlusMultiplies", np.float32, u)
        assert g.spmv_format_info(A, 0)["in_use"] == in_use
        assert g.spmv_plan_info(A, 0)["nhot"] == slc.HOT
        rel = np.abs(got - ref)[ref != 0] / np.abs(ref[ref != 0])
        print("format %d: largest relative error %.3g (bar 1e-5)" % (setting, rel.max()))
        assert np.allclose(got, ref, rtol=1e-5, atol=1e-6), setting
        if setting == 0:
            again = product(g, A, W, 0, "PlusMultiplies", np.float32, u)
            assert np.array_equal(got.view(np.int32), again.view(np.int32))
