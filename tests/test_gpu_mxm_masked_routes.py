"""The masked product C<M> = op(A) (+.x) op(B) (grb_mxm with a mask, csrc/mxm.hip) on every route of its host dispatch,
against the host reference of tests/mxm_masked_cases.py (tied to the oracle on the CPU by
tests/test_mxm_masked_reference.py).  The patterns, and what each one reaches:

  comb      a pivot on both sides of every capacity edge (wave | 64 KiB | 128 KiB | segments for 8- and 4-byte slots,
            2048 | 2049 for the bitmap), in both passes, the mask distinct from A and B, rectangular
  fan       more than 1024 and more than 4096 entries of one pivot, empty partners
  ranges4   the bitmap kernel over cached ranges: an empty range between two others, a first range that is not 0
  ranges10  the bitmap kernel over more than 8 ranges: cut points searched per range
  Z...      A empty, B empty, every mask value zero, 1 x 1, an empty pivot row

Each runs mirrored too (A and B swapped, the mask transposed), in the four value layouts (which side holds one value
throughout decides between key-only and (key, value) tables and the one-valued shortcuts) and both types, the mask an
f32 matrix for one of the pair and an i32 matrix for the other.  The data are exact in float32 and int32 in any order,
so values are compared bit for bit; the structure is the mask's.  The two static environment switches run in child
processes (tests/tools/mxm_masked_child.py).  The wrong-shape calls at the end are only meaningful with the dimension
checks of grb_mxm in place: without them the entry-driven kernel would index B's pointers by the mask's columns.

Out of scope: the dense core (mxm_core.hip), tc_count.hip, column ids near 2^31, NaN / Inf data."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mxm_masked_cases as mc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = ["f32", "i32"]
ORIENTATIONS = [(0, 1), (0, 0), (1, 1), (1, 0)]               # (GrB_INP0, GrB_INP1) transposed; the first is tc()'s
OTHER = {np.float32: np.int32, np.int32: np.float32}


def check(g, case, dtype, layout, semirings, mask, orientations=ORIENTATIONS[:1], mask_csc=True):
    for sr in semirings:
        av, bv = mc.operands(case, sr, dtype, layout)
        ref = mc.want(case, sr, dtype, av, bv)
        for tran_a, tran_b in orientations:
            got = mc.product(g, case, dtype, sr, av, bv, mask, tran_a, tran_b)
            bad = mc.mismatches(case, dtype, layout, sr, got, ref, mask_csc)
            assert bad is None, "%s (INP0, INP1 transposed: %d, %d)" % (bad, tran_a, tran_b)


def pair(g, name, dtype):
    """(case, its mask) for a pattern and its mirror: the mask in the product's type for one, in the other type
    for the other (the kernels take the mask's type as a flag of its own)"""
    case = mc.get(name)
    return [(case, mc.build_mask(g, case, dtype)), (case.mirrored(), mc.build_mask(g, case.mirrored(), OTHER[dtype]))]


# ---- the 13 commutative semirings on every pattern, type and layout (the two large index spaces last) ----------------
@pytest.mark.parametrize("layout", mc.LAYOUTS)
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["comb", "fan", "ranges4", "ranges10"])
def test_commutative_semirings_on_every_route(hip, name, dtype, layout):
    for case, mask in pair(hip, name, dtype):
        check(hip, case, dtype, layout, mc.COMMUTATIVE, mask)


# ---- the four comparison semirings: one lane per entry, the hinted search on lists of 20 000 entries ------------------
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
def test_comparison_semirings_fold_ascending_on_comb(hip, dtype):
    for case, mask in pair(hip, "comb", dtype):
        for layout in ("valued", "iso_a"):
            check(hip, case, dtype, layout, mc.COMPARISONS, mask)


# ---- the four orientations, through stored transposes ------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["comb", "fan", "ranges4", "ranges10"])
def test_four_orientations(hip, name, dtype):
    """PlusMinus (the operand order is part of the answer) and MinimumPlus, valued and both sides one-valued"""
    for case, mask in pair(hip, name, dtype):
        for layout in ("valued", "iso_ab"):
            check(hip, case, dtype, layout, ["PlusMinus", "MinimumPlus"], mask, ORIENTATIONS)


# ---- a mask without a CSC of its own: pass 2 is the entry-driven kernel's ------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
@pytest.mark.parametrize("kind", ["product_result", "csr_only_format"])
@pytest.mark.parametrize("name", ["comb", "fan"])
def test_mask_without_a_csc(hip, name, kind, dtype):
    """The mask is itself the result of a masked product (which makes no CSC), or a matrix created under
    GRB_SPARSE_MATRIX_FORMAT=1: the entries whose row of B is the longer list go to entry_driven(1) -- on comb by the
    whole wave wherever the shorter list has more than 16 entries."""
    g = hip
    for case in (mc.get(name), mc.get(name + "~")):
        f = mc.routes(case, dtype, "valued", "PlusMinus", mask_csc=False)
        assert mc.PASS2 not in set(f["owner"].tolist())
        if name == "comb":
            assert mc.owned(f, mc.ENTRY_B_LONGER, "heavy") > 100 and mc.owned(f, mc.ENTRY_B_LONGER, "lane") > 100
        elif case.name.endswith("~"):
            assert mc.owned(f, mc.ENTRY_B_LONGER, "lane") > 3000
        if kind == "product_result":
            # C<M> = 1 (+.x) 1' over one shared column: 1 where the mask's value is not zero, 0 elsewhere -- as a mask
            # the same as M, in the product's type, with the arrays a result has
            ones = lambda n: (n, 1, np.arange(n + 1, dtype=np.int32), np.zeros(n, dtype=np.int32), np.ones(n))
            unit = mc.Case("unit", case.m, case.n, 1, ones(case.m)[2:4], ones(case.n)[2:4], (case.mp, case.mi))
            mask = g.Matrix(case.m, case.n, dtype)
            cv = mc.product(g, unit, dtype, "PlusMultiplies", np.ones(case.m, dtype=dtype), np.ones(case.n, dtype=dtype),
                            mc.build_mask(g, case, OTHER[dtype]), out=mask)
            assert np.array_equal(cv != 0, case.mask_values() != 0)
        else:
            saved = os.environ.get("GRB_SPARSE_MATRIX_FORMAT")
            os.environ["GRB_SPARSE_MATRIX_FORMAT"] = "1"
            try:
                mask = g.Matrix(case.m, case.n, dtype)
            finally:
                if saved is None:
                    del os.environ["GRB_SPARSE_MATRIX_FORMAT"]
                else:
                    os.environ["GRB_SPARSE_MATRIX_FORMAT"] = saved
            assert mask.build_csr(case.mp, case.mi, mc.mask_array(case, dtype)) == 0
        for layout in ("valued", "iso_ab"):
            check(g, case, dtype, layout, ["PlusMultiplies", "PlusMinus", "MinimumPlus"], mask, mask_csc=False)


# ---- real values ---------------------------------------------------------------------------------------------------------
def test_real_values_within_the_summation_bound_and_repeatable(hip):
    """f32 PlusMultiplies on values in [0.5, 1.5): |got - want| <= gamma(k + 1) sum |a b| against the float64 reference,
    k the entry's common columns (k products rounded once, k - 1 additions in some order: at most k roundings on any
    term, gamma(k); one more for the comparison's own rounding of the stored float).  Two calls give the same bits:
    a partner is folded by one wave in program order."""
    g = hip
    f32 = np.float32
    for case, mask in pair(g, "comb", f32):
        rng = np.random.default_rng(mc._seed(case.name, "real"))
        av = (0.5 + rng.random(case.ai.size)).astype(f32)
        bv = (0.5 + rng.random(case.bi.size)).astype(f32)
        got = mc.product(g, case, f32, "PlusMultiplies", av, bv, mask)
        again = mc.product(g, case, f32, "PlusMultiplies", av, bv, mask)
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))
        ref, mag = mc.want_real(case, av, bv)
        k = mc.common_columns(case)
        err = np.abs(got.astype(np.float64) - ref)
        bound = mc.gamma(k + 1) * mag
        worst = int(np.argmax(err - bound))
        assert np.all(err <= bound), (case.name, worst, int(k[worst]), float(err[worst]), float(bound[worst]))
        live = case.mask_values() != 0
        assert np.all(got[~live] == 0) and k[live].max() > 8000 and np.count_nonzero(err) > 1000


# ---- the static switches: a fresh process each ------------------------------------------------------------------------------
def test_static_switches_in_child_processes():
    """GRB_TC_BITMAP_MIN=0 (the compact key-only path on 128 KiB tables and segments) and GRB_MXM_PIVOT=0 (the
    entry-driven kernel alone) are read once per process: one child each, one at a time, nothing after a failure"""
    for mode, var in (("compact", "GRB_TC_BITMAP_MIN"), ("entry", "GRB_MXM_PIVOT")):
        env = dict(os.environ)
        env.pop("GRB_TC_BITMAP_MIN", None)
        env.pop("GRB_MXM_PIVOT", None)
        env[var] = "0"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "mxm_masked_child.py"), mode],
                             capture_output=True, text=True, timeout=240, cwd=ROOT, env=env)
        assert out.returncode == 0 and "mxm_masked_child %s: ok" % mode in out.stdout, \
            (mode, out.returncode, out.stdout[-3000:], out.stderr[-2000:])


# ---- degenerate patterns -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
def test_degenerate_patterns(hip, dtype):
    """info 0 (asserted by every call), the mask's structure, and the identity wherever nothing is folded"""
    from oracle.semiring import Semiring
    g = hip
    for name in mc.degenerate():
        for case, mask in pair(g, name, dtype):
            for layout in ("valued", "iso_ab"):
                check(g, case, dtype, layout, mc.COMMUTATIVE + mc.COMPARISONS, mask)
            if name in ("Za", "Zb", "Zm"):
                for sr in ("PlusMultiplies", "MinimumPlus", "GreaterPlus"):
                    av, bv = mc.operands(case, sr, dtype, "valued")
                    got = mc.product(g, case, dtype, sr, av, bv, mask)
                    assert got.size == 30 and np.all(got == Semiring(sr, dtype).identity()), (name, sr)
    one = mc.get("Z1")
    got = mc.product(g, one, dtype, "PlusMultiplies", np.array([3], dtype=dtype), np.array([-2], dtype=dtype),
                     mc.build(g, (1, 1, one.mp, one.mi, [1]), dtype))
    assert got.tolist() == [-6]
    # a mask without entries: nothing to compute, an empty result
    a, b = mc.stored(mc.get("Zm"), 0, 1, *mc.operands(mc.get("Zm"), "PlusMultiplies", dtype, "valued"))
    d = g.Descriptor()
    assert d.loadArgs() == 0 and d.toggle(g.GrB_INP1) == 0
    Cm = g.Matrix(5, 6, dtype)
    empty = mc.build(g, (5, 6, np.zeros(6, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0)), dtype)
    assert g.mxm(Cm, empty, None, "PlusMultiplies", mc.build(g, a, dtype), mc.build(g, b, dtype), d) == 0 and Cm.nvals() == 0


# ---- shapes that do not fit: GrB_DIMENSION_MISMATCH before C is touched -------------------------------------------------------
@pytest.mark.parametrize("dtype", mc.DTYPES, ids=IDS)
def test_dimension_mismatch_leaves_the_result_alone(hip, dtype):
    """op(B) with fewer or more columns than the mask, and operands whose shared dimensions differ, in the four
    orientations: GrB_DIMENSION_MISMATCH, and C -- which held another matrix -- is what it was"""
    g = hip
    rng = np.random.default_rng(77)
    m, n, K = 9, 12, 20

    def rows(nrows, ncols):
        return mc._csr([np.sort(rng.choice(ncols, int(rng.integers(1, 5)), replace=False)) for _ in range(nrows)])
    (mp, mi), (kp, ki) = rows(m, n), rows(m, n)
    mask = mc.build(g, (m, n, mp, mi, np.ones(mi.size)), dtype)
    kept = rng.integers(1, 9, ki.size).astype(dtype)
    for tran_a, tran_b in ORIENTATIONS:
        d = g.Descriptor()
        assert d.loadArgs() == 0
        if tran_a:
            assert d.toggle(g.GrB_INP0) == 0
        if tran_b:
            assert d.toggle(g.GrB_INP1) == 0
        # (columns of op(B), its shared dimension): fewer columns than the mask, more, another shared dimension
        for nb, kb in ((n - 5, K), (n + 3, K), (n, K - 1), (n, K + 7)):
            ap, ai = rows(K, m) if tran_a else rows(m, K)
            bp, bi = rows(nb, kb) if tran_b else rows(kb, nb)
            A = mc.build(g, ((K, m) if tran_a else (m, K)) + (ap, ai, np.ones(ai.size)), dtype)
            B = mc.build(g, ((nb, kb) if tran_b else (kb, nb)) + (bp, bi, np.ones(bi.size)), dtype)
            Cm = mc.build(g, (m, n, kp, ki, kept), dtype)
            info = g.mxm(Cm, mask, None, "PlusMultiplies", A, B, d)
            assert info == g.GrB_DIMENSION_MISMATCH, (tran_a, tran_b, nb, kb, info)
            cp, ci, cv = Cm.host_csr()
            assert Cm.nvals() == ki.size and np.array_equal(cp, kp) and np.array_equal(ci, ki) and np.array_equal(cv, kept)
        # ... and the same call with shapes that fit succeeds
        ap, ai = rows(K, m) if tran_a else rows(m, K)
        bp, bi = rows(n, K) if tran_b else rows(K, n)
        A = mc.build(g, ((K, m) if tran_a else (m, K)) + (ap, ai, np.ones(ai.size)), dtype)
        B = mc.build(g, ((n, K) if tran_b else (K, n)) + (bp, bi, np.ones(bi.size)), dtype)
        Cm = mc.build(g, (m, n, kp, ki, kept), dtype)
        assert g.mxm(Cm, mask, None, "PlusMultiplies", A, B, d) == 0 and np.array_equal(Cm.host_csr()[1], mi)
