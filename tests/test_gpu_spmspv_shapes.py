"""The push product (csrc/spmspv.hip on csrc/push_common.hpp) through grb_vxm / grb_mxv across the sizes at which its
stages change behaviour, against the host reference of tests/spmspv_cases.py (tied to the oracle on the CPU by
tests/test_spmspv_reference.py).  The patterns, and the boundary each one crosses:

  S        one scan tile (the tile-sum scan is skipped), one chunk, one bitmap tile
  E0, E1   chunk edges: a running total of exactly 2048 at a row boundary, a hub over two whole chunks, a hub of exactly
           one chunk, a chunk whose frontier range is longer than the 2048 staged entries (the search per edge), a scan
           tile of sum 0, a scan-tile boundary inside a staged chunk, three bitmap tiles with a partial last word; the
           last chunk full (E0) or of one edge (E1)
  T        more than 256 scan tiles: the carry loop of push_scan_tiles_kernel
  B        more than 256 bitmap tiles: the same loop in the compaction, the last word with one valid bit
  D        more than 2048 chunks: lb_expand_kernel's workgroups take a second chunk; 2100 combines into every output
  Z        one entry, one empty row, only empty rows

S and E run the 13 commutative semirings, both types, both orientations, every mask and both result modes; T, B and D
one semiring for each combine of atomic_combine (atomicAdd, atomicMin, atomicMax, plain store, CAS loop).  The data
are exact in float32 and int32 in any order, so indices, values and nvals are compared for equality, never within a
tolerance; every call also asserts sparse result storage and that the push ran.

Out of scope: the grid loop of push_partition_kernel (more than 262 144 chunks), 32-bit overflow of the expanded-edge
total, NaN / Inf data, the four order-dependent comparison semirings."""
import numpy as np
import pytest

import spmspv_cases as sc

pytestmark = pytest.mark.gpu
IDS = ["f32", "i32"]


def matrix(g, case, orient, vals, dtype):
    """A = M for vxm (the push walks A's CSR), A = M' for mxv (it walks the CSC the library derives)"""
    nrows, ncols, ptr, ind, v = case.matrix_arrays(orient, vals)
    A = g.Matrix(nrows, ncols, dtype)
    assert A.build_csr(ptr, ind, v) == 0
    return A


def push(g, A, case, orient, sr, dtype, fval, mask_name, mask, sparse_mask, struconly):
    """(nvals, indices, values) of w = u A (vxm) or A u (mxv) with a sparse u under mxvmode = 1.  The mask is a float
    vector for vxm and an integer one for mxv."""
    mask_kind, scmp = sc.MASK_ARGS[mask_name]
    mask_dtype = np.float32 if orient == "vxm" else np.int32
    d = g.Descriptor()
    assert d.loadArgs(mxvmode=1, struconly=struconly) == 0
    if scmp:
        assert d.set(g.GrB_MASK, g.GrB_SCMP) == 0
    u, w = g.Vector(case.nrows, dtype), g.Vector(case.ncols, dtype)
    assert u.build(case.fidx, fval, case.nf, None) == 0
    mk = None
    if mask_kind == "dense":
        mk = g.Vector(case.ncols, mask_dtype)
        assert mk.build(mask.astype(mask_dtype), case.ncols) == 0
    elif mask_kind == "sparse":
        mk = g.Vector(case.ncols, mask_dtype)
        assert mk.build(sparse_mask[0], sparse_mask[1].astype(mask_dtype), sparse_mask[0].size, None) == 0
    info = g.vxm(w, mk, None, sr, u, A, d) if orient == "vxm" else g.mxv(w, mk, None, sr, A, u, d)
    assert info == 0, info
    assert w.getStorage() == g.GrB_SPARSE and d.lastmxv_ == g.GrB_PUSHONLY
    nvals = w.nvals()
    info, idx, val = w.extractTuples(sparse=True)
    assert info == 0 and idx.size == nvals
    return nvals, idx, val


def check(g, case, orient, sr, dtype, mask_names, prepared=None):
    """every (mask, result mode) of one matrix against the reference: nvals, indices and values equal"""
    (vals, fval, mask, sparse_mask), folded = prepared or sc.prepared(case, sr, dtype)
    A = matrix(g, case, orient, vals, dtype)
    for mask_name in mask_names:
        mask_kind, scmp = sc.MASK_ARGS[mask_name]
        for struconly in (0, 1):
            what = "%s %s %s %s, mask %s, struconly %d" % (case.name, orient, sr, dtype.__name__, mask_name, struconly)
            nvals, idx, val = push(g, A, case, orient, sr, dtype, fval, mask_name, mask, sparse_mask, struconly)
            ref_i, ref_v = sc.want(case, orient, sr, dtype, vals, case.fidx, fval, mask_kind, mask, scmp, struconly, folded)
            assert nvals == ref_i.size, "%s: nvals %d, want %d" % (what, nvals, ref_i.size)
            assert np.array_equal(idx, ref_i), "%s: indices differ, first at %s" % (what, np.nonzero(idx != ref_i)[0][:4])
            if not struconly:
                bad = np.nonzero(val != ref_v)[0]
                assert val.dtype == ref_v.dtype
                assert bad.size == 0, "%s: %d values differ, first at outputs %s: got %s, want %s" % (
                    what, bad.size, idx[bad[:4]], val[bad[:4]], ref_v[bad[:4]])
    return A


# ---- kept state: first in the file, so that B's 2 200 001 outputs are what grows the bitmap and the accumulator ------
def test_bitmap_and_accumulator_survive_growth_and_changes_of_identity_and_type(hip):
    """The touched bitmap (scratch slot 4) and the accumulator (slot 5) are cleaned by the compaction, not per call,
    and refilled only on growth, on a change of identity or of type.  One sequence on the process's context; every
    step is compared with the reference, so a stray bit or a stale value left by one step shows in the next."""
    g = hip
    S, B, E = sc.small(), sc.many_bitmap_tiles(), sc.chunk_edges_0()
    f32, i32 = np.float32, np.int32

    def step(case, orient, sr, dtype, mask_name, struconly):
        vals, fval, mask, sparse_mask = sc.operands(case, sr, dtype)
        mask_kind, scmp = sc.MASK_ARGS[mask_name]
        A = matrix(g, case, orient, vals, dtype)
        nvals, idx, val = push(g, A, case, orient, sr, dtype, fval, mask_name, mask, sparse_mask, struconly)
        ref_i, ref_v = sc.want(case, orient, sr, dtype, vals, case.fidx, fval, mask_kind, mask, scmp, struconly)
        assert nvals == ref_i.size and np.array_equal(idx, ref_i), (case.name, sr, struconly)
        if not struconly:
            assert val.dtype == ref_v.dtype and np.array_equal(val, ref_v), (case.name, sr)
        return nvals

    step(S, "vxm", "MinimumPlus", f32, "none", 0)               # 1  accumulator: FLT_MAX, float
    step(B, "mxv", "PlusMultiplies", i32, "none", 0)            # 2  both slots grow; identity 0, int
    step(S, "vxm", "PlusMultiplies", f32, "none", 1)            # 3  structure only: the bitmap alone
    step(S, "vxm", "MaximumMultiplies", f32, "none", 0)         # 4  int to float under a capacity far larger than needed
    kept = step(E, "vxm", "PlusMultiplies", f32, "dense+scmp", 0)       # 5  same identity and type: no refill
    vals, fval, mask, _ = sc.operands(E, "PlusMultiplies", f32)
    passing = sc.want(E, "vxm", "PlusMultiplies", f32, vals, E.fidx, fval, "dense", mask, 1, 1)[0].size
    assert kept < passing                                       #    ... and its zero-prune dropped entries
    step(S, "vxm", "PlusMultiplies", f32, "none", 1)            # 6  structure only
    step(S, "vxm", "MinimumPlus", f32, "none", 0)               # 7  step 1 again: the identity alone changes, 0 to FLT_MAX


# ---- S and E: everything -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["S", "E0", "E1"])
def test_every_semiring_mask_and_mode(hip, name, dtype):
    """13 semirings x both orientations x none / dense / dense + scmp / sparse mask x key-value / structure-only"""
    case = sc.CASES[name]()
    for sr in sc.COMMUTATIVE:
        prepared = sc.prepared(case, sr, dtype)
        for orient in sc.ORIENTS:
            check(hip, case, orient, sr, dtype, sc.MASKS, prepared)


# ---- T, B, D: one semiring for each combine ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name,orient", [("T", "vxm"), ("B", "mxv"), ("D", "vxm"), ("D", "mxv")])
def test_carry_loops_and_the_grid_cap(hip, name, orient, dtype):
    """T: 294 scan tiles; B: 269 bitmap tiles; D: 2154 chunks on 2048 workgroups.  No mask and dense + scmp, key-value
    and structure-only; the reference is folded once for each semiring (D: as a dense product)."""
    case = sc.CASES[name]()
    for sr in sc.COMBINES:
        check(hip, case, orient, sr, dtype, ["none", "dense+scmp"])


# ---- Z ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", sc.DTYPES, ids=IDS)
def test_degenerate_frontiers(hip, dtype):
    """one row of one entry equals the reference; one empty row and a frontier of only empty rows: info 0 (asserted
    by every call), nvals == 0 and empty tuples"""
    for name in ("Z1", "Z0", "Zn"):
        case = sc.CASES[name]()
        for sr in sc.COMBINES:
            vals, fval, mask, sparse_mask = sc.operands(case, sr, dtype)
            for orient in sc.ORIENTS:
                A = check(hip, case, orient, sr, dtype, sc.MASKS)
                if case.total == 0:
                    for struconly in (0, 1):
                        nvals, idx, val = push(hip, A, case, orient, sr, dtype, fval, "none", mask, sparse_mask, struconly)
                        assert nvals == 0 and idx.size == 0 and val.size == 0
    # the single entry once more by hand, without the reference: row 3 holds column 69 alone
    one = sc.one_entry()
    vals = np.where(sc.operands(one, "PlusMultiplies", dtype)[0] == 0, 2, 1).astype(dtype)
    fval = np.full(1, 3, dtype=dtype)
    A = matrix(hip, one, "vxm", vals, dtype)
    nvals, idx, val = push(hip, A, one, "vxm", "PlusMultiplies", dtype, fval, "none", None, None, 0)
    assert nvals == 1 and idx.tolist() == [69] and val[0] == 3 * vals[one.ptr[3]]
