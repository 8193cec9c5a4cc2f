"""Patterns, operands, the host reference and a model of the routes for the tests of the masked product
C<M> = op(A) (+.x) op(B) (grb_mxm with a mask, csrc/mxm.hip) -- tests/test_gpu_mxm_masked_routes.py on the GPU,
tests/test_mxm_masked_reference.py on the CPU.

A pattern is two lists of sorted rows over a shared dimension K -- A is m x K, B is n x K, the product is A B' -- and
a mask of m x n: C[i, j] folds A[i, k] (x) B[j, k] over the columns k the two rows share.  Every mask entry has an
OWNER (host code of grb_mxm):

  pass 1   row i of A is the pivot: the entries with len(B_j) <= len(A_i)
  pass 2   row j of B is the pivot: the others, listed by the mask's CSC -- or, for a mask without a CSC of its own,
           the entry-driven kernel (`entry_driven(1)`), which is also the only kernel of a semiring whose fold is
           ordered (the four comparison "monoids") and of GRB_MXM_PIVOT=0

and every pivot a KERNEL by its length: a wave's table up to WAVE_CAP entries, then LDS tables of 64 KiB, of 128 KiB,
the pivot in segments of a 128 KiB table -- with 8-byte (key, value) slots, or 4-byte keys when the pivot side holds
one value throughout -- or, for an int32 plus-monoid with both sides one-valued, a bitmap per range of BITMAP_COLS
columns beyond BITMAP_MIN entries (with cut points cached up to BITS_MAX_SEG ranges, searched per range beyond).
routes() restates that dispatch in numpy, and every builder asserts from it the facts it exists for: a changed seed
or constant cannot leave a route unnoticed.

  comb      215 x 245 over K = 40000      one row on each side for every length on a capacity edge (256 | 257,
                                          2048 | 2049, 4096 | 4097, 8192 | 8193, 16384 | 16385) and 20000, then some
                                          200 rows of 0..40 entries; the mask -- distinct from A and B -- holds every
                                          long row and column in full and 5 % of the rest: every kernel in both
                                          passes for both slot sizes, wave tiles of 64 partners, mixed routes
  fan       3 x 4200 over K = 60000       pivots of 300, 5000 and 20000 entries under a full mask: more than 1024 and
                                          more than 4096 entries of one pivot; partners of 0..12 entries
  ranges4   4 x 100 over 3 * 2^20 + 12345 bitmap pivots over several cached ranges: one over ranges 0..3, one with an
                                          empty range between two others, one that starts in range 1, one with entries
                                          in ranges 1 and 3 only; partners on both sides of every range boundary, and
                                          one wholly inside a range a pivot skips
  ranges10  3 x 100 over 9 * 2^20 + 777   a pivot in 10 ranges (searched per range), one in ranges 0 and 9 alone (eight
                                          skipped), one in ranges 4 and 5 (cached, first range not 0)
  Z...      small                         A empty, B empty, every mask value zero, 1 x 1, an empty pivot row

Every pattern also runs mirrored (A and B swapped, the mask transposed): pass 2 then sees what pass 1 saw and a
non-commutative multiply its operands in the other order.  LAYOUTS are the value layouts: both sides one-valued (3 and
2: a swapped operand order changes the answer), A alone, B alone, neither.

Data are small integers (dyadic quotients for PlusDivides; mostly 1 with at most four 2s to a row for the Multiplies
monoid): every partial result in any order is exact in float32 and in int32, which want() asserts in float64 / int64,
so GPU results are compared bit for bit.  A fifth of the mask's stored values are zero, some data are negative, and
some equal the semiring's identity -- wherever the multiply of the identity with a neighbour stays exact: for
MinimumPlus and MinimumMultiplies (identity FLT_MAX / INT_MAX) only in reserved columns where the other side holds the
multiply's neutral value, and only when both sides are valued.

The reference is the expand-sort-fold join over the shared dimension (expand_sort / fold, which the unmasked product's
test uses too), restricted to the mask's nonzero entries; everything else is the semiring's identity.  It folds
ascending in k, so it also defines the four comparison semirings.

Out of scope: the dense core (mxm_core.hip), tc_count.hip, column ids near 2^31, NaN / Inf data.
"""
import functools
import os

import numpy as np

from oracle.semiring import BINARY_OPS, Semiring
from spmv_long_cases import COMMUTATIVE, DTYPES, fold_rows

# ---- the constants of csrc/mxm.hip the dispatch depends on (tests/test_mxm_masked_reference.py reads them there) ------
LANE_DOT_MAX = 16          # kLaneDotMax: a longer shorter list goes to the whole wave (entry-driven kernel)
WAVE_CAP = 256             # kWaveCap: pivot entries a wave's table holds
WAVE_TILE = 64             # partners per tile of the wave kernel
BLOCK_TILE = 1024          # partners per trip of a workgroup (t0 += 1024)
TABLE_BYTES = (65536, 131072)
SLOT_BYTES = {"key+value": 8, "key": 4}                       # sizeof(HashSlot), sizeof(KeySlot)
BITMAP_MIN = 2048          # default of GRB_TC_BITMAP_MIN: longer pivots go to the bitmap kernel
BITS_MAX_SEG = 8           # kBitsMaxSeg: ranges per pivot whose cut points are cached
ITEM_ENTRIES = 4096        # kBitsItemEntries = 4 * 1024: entries of one PivotItem
BITMAP_COLS = 1 << 20      # kCols of the 128 KiB bitmap: columns per range

COMPARISONS = ["GreaterPlus", "CustomLessPlus", "NotEqualToPlus", "CustomLessLess"]
LAYOUTS = ["iso_ab", "iso_a", "iso_b", "valued"]
EDGE_LENGTHS = (17, 64, 65, 256, 257, 1024, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 20000)
ORDER_FREE = ("plus", "multiplies", "minimum", "maximum", "logical_or", "logical_and")     # mxm_order_free()

# owners and kernels of routes()
NOBODY, PASS1, PASS2, ENTRY_B_LONGER, ENTRY_ALONE = 0, 1, 2, 3, 4
KERNELS = ["none", "lane", "heavy", "wave", "table64", "table128", "segments", "bitmap"]
K_NONE, K_LANE, K_HEAVY, K_WAVE, K_T64, K_T128, K_SEG, K_BITMAP = range(8)


def _atoi(text):
    """atoi / atoll: an optional sign and the leading digits, 0 without any"""
    text = text.strip()
    end = 1 if text[:1] in "+-" else 0
    while end < len(text) and text[end].isdigit():
        end += 1
    try:
        return int(text[:end])
    except ValueError:
        return 0


def bitmap_min():
    """GRB_TC_BITMAP_MIN as grb_mxm reads it (once per process): 0 = never the bitmap"""
    e = os.environ.get("GRB_TC_BITMAP_MIN")
    return BITMAP_MIN if e is None else _atoi(e)


def pivot_on():
    """GRB_MXM_PIVOT as grb_mxm reads it (once per process): 0 keeps the entry-driven kernel alone"""
    e = os.environ.get("GRB_MXM_PIVOT")
    return e is None or _atoi(e) != 0


def _seed(*what):
    """a seed from names and flags that does not change between runs (hash() of a string does)"""
    return sum((i + 1) * sum(str(w).encode()) for i, w in enumerate(what)) % (1 << 31)


def _csr(rows):
    ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in rows], out=ptr[1:])
    ind = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows]) if ptr[-1] else np.zeros(0, dtype=np.int64)
    return ptr.astype(np.int32), ind.astype(np.int32)


def transpose(nrows, ncols, ptr, ind):
    """(ptr, ind, perm) of the transposed pattern: values of the transpose = values[perm]"""
    perm = np.argsort(ind, kind="stable")
    tind = np.repeat(np.arange(nrows, dtype=np.int32), np.diff(ptr))[perm]
    tptr = np.zeros(ncols + 1, dtype=np.int32)
    np.cumsum(np.bincount(ind, minlength=ncols), out=tptr[1:])
    return tptr, tind, perm


class Case:
    """A (m x K) and B (n x K) as sorted rows, the mask (m x n) in CSR.  mask_zero: every stored mask value is 0."""

    def __init__(self, name, m, n, K, a, b, mask, mask_zero=False):
        self.name, self.m, self.n, self.K, self.mask_zero = name, int(m), int(n), int(K), mask_zero
        (self.ap, self.ai), (self.bp, self.bi), (self.mp, self.mi) = a, b, mask
        for nr, nc, p, i in ((m, K, self.ap, self.ai), (n, K, self.bp, self.bi), (m, n, self.mp, self.mi)):
            assert p.dtype == np.int32 and i.dtype == np.int32 and p.size == nr + 1 and p[0] == 0 and p[-1] == i.size
            key = np.repeat(np.arange(nr, dtype=np.int64), np.diff(p)) * nc + i
            assert np.all(np.diff(key) > 0) and (i.size == 0 or (0 <= i.min() and i.max() < nc))
        self.la, self.lb = np.diff(self.ap).astype(np.int64), np.diff(self.bp).astype(np.int64)
        self.mrow = np.repeat(np.arange(self.m, dtype=np.int64), np.diff(self.mp))
        self._join = self._mirror = None

    def mask_values(self):
        """the mask's stored values as integers: a fifth are zero, the others 1, 2 or -1"""
        rng = np.random.default_rng(_seed(self.name, "mask"))
        mv = np.where(rng.random(self.mi.size) < 0.2, 0, rng.choice([1, 2, -1], self.mi.size))
        if self.mask_zero:
            mv[:] = 0
        elif mv.size >= 10:
            mv[0], mv[-1] = 0, 1
        return mv.astype(np.int64)

    def mirrored(self):
        """A and B swapped, the mask transposed"""
        if self._mirror is None:
            tp, ti, _ = transpose(self.m, self.n, self.mp, self.mi)
            self._mirror = Case(self.name + "~", self.n, self.m, self.K, (self.bp, self.bi), (self.ap, self.ai), (tp, ti),
                                self.mask_zero)
        return self._mirror

    def join(self):
        """the products of the mask's entries: (position in A's values, position in B's values, pointer of every mask
        entry into them), ascending in k inside an entry.  The full join A B' is expanded and sorted once, then cut to
        the mask's entries (whatever the mask's values)."""
        if self._join is None:
            tp, ti, perm = transpose(self.n, self.K, self.bp, self.bi)                 # B' in CSR: K x n
            ea, q, pi, pj, start = expand_sort(self.m, self.n, self.ap, self.ai, tp, ti)
            eb = perm[q]
            first = np.flatnonzero(start)
            gkey = pi[first].astype(np.int64) * self.n + pj[first]
            gptr = np.r_[first, ea.size].astype(np.int64)
            mkey = self.mrow * self.n + self.mi
            ptr = np.zeros(mkey.size + 1, dtype=np.int64)
            src = np.zeros(0, dtype=np.int64)
            if gkey.size and mkey.size:
                at = np.minimum(np.searchsorted(gkey, mkey), gkey.size - 1)
                cnt = np.where(gkey[at] == mkey, np.diff(gptr)[at], 0)
                np.cumsum(cnt, out=ptr[1:])
                src = np.repeat(gptr[at] - ptr[:-1], cnt) + np.arange(ptr[-1])
            self._join = (ea[src], eb[src], ptr)
        return self._join


# ---- the join over the shared dimension (the unmasked product's test folds with these too) -----------------------------
def expand_sort(m, n, ap, ai, bp, bi):
    """Every product of A (m x k, CSR) with B (k x n, CSR), sorted by (i, j, k): (position of the A factor, position
    of the B factor, i, j, first-of-its-(i, j) flag)"""
    rows = np.repeat(np.arange(m), np.diff(ap))
    lens = np.diff(bp)[ai]
    tot = int(lens.sum())
    if tot == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z, z, np.zeros(0, dtype=bool)
    ent = np.repeat(np.arange(ai.size), lens)
    q = bp[ai[ent]] + (np.arange(tot) - np.repeat(np.cumsum(lens) - lens, lens))
    pi, pj, pk = rows[ent], bi[q], ai[ent]
    order = np.lexsort((pk, pj, pi))
    ent, q, pi, pj = ent[order], q[order], pi[order], pj[order]
    key = pi.astype(np.int64) * n + pj
    start = np.r_[True, key[1:] != key[:-1]]
    return ent, q, pi, pj, start


def fold_ascending(sr, prod, ptr, dtype):
    """acc = add(product, acc) from the identity over every group's products in their order, one step of all groups
    at a time; ptr: the groups' pointer array"""
    lens = np.diff(ptr)
    acc = np.full(lens.size, sr.identity(), dtype=dtype)
    if prod.size == 0:
        return acc
    gid = np.repeat(np.arange(lens.size), lens)
    rank = np.arange(prod.size) - np.repeat(ptr[:-1], lens)
    order = np.argsort(rank, kind="stable")
    at = 0
    for c in np.bincount(rank):
        sel = order[at:at + c]
        acc[gid[sel]] = sr.add_op(prod[sel], acc[gid[sel]])
        at += c
    return acc


def fold(sr, m, n, ap, ai, av, bp, bi, bv, dtype=np.float32):
    """C = A (+.x) B in CSR, each entry acc = add(mul(a_ik, b_kj), acc) over k ascending (stored zeros kept)"""
    ea, eb, pi, pj, start = expand_sort(m, n, ap, ai, bp, bi)
    if ea.size == 0:
        return np.zeros(m + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, dtype)
    prod = sr.mul_op(av[ea], bv[eb])
    acc = fold_ascending(sr, prod, np.r_[np.flatnonzero(start), ea.size], dtype)
    cp = np.zeros(m + 1, np.int32)
    np.cumsum(np.bincount(pi[start], minlength=m), out=cp[1:])
    return cp, pj[start].astype(np.int32), acc


# ---- the route model ---------------------------------------------------------------------------------------------------
def _pass_kernels(piv_len, ent_count, piv_ind_ptr, piv_ind, piv_iso, par_iso, is_int, plus):
    """one run_pass: per pivot the kernel, and what the launch is instantiated with"""
    key_only = bool(piv_iso)
    slot = SLOT_BYTES["key" if key_only else "key+value"]
    cap64, cap128 = TABLE_BYTES[0] // slot // 2, TABLE_BYTES[1] // slot // 2
    big = (piv_len > WAVE_CAP) & (ent_count > 0)
    longest = int(piv_len[big].max()) if big.any() else 0
    max_tab = 0x7fffffff
    compact = key_only and is_int and plus and bool(par_iso)
    if compact and bitmap_min() > 0 and longest > bitmap_min():
        max_tab = bitmap_min()
    kern = np.full(piv_len.size, K_SEG, dtype=np.int8)
    kern[piv_len <= cap128] = K_T128
    kern[piv_len <= cap64] = K_T64
    kern[piv_len > max_tab] = K_BITMAP
    kern[piv_len <= WAVE_CAP] = K_WAVE
    kern[piv_len == 0] = K_NONE
    first = last = occupied = np.zeros(piv_len.size, dtype=np.int64)
    if piv_ind.size:
        first = piv_ind[np.minimum(piv_ind_ptr[:-1], piv_ind.size - 1)].astype(np.int64) // BITMAP_COLS
        last = piv_ind[np.maximum(piv_ind_ptr[1:] - 1, 0)].astype(np.int64) // BITMAP_COLS
        rng_of = piv_ind.astype(np.int64) // BITMAP_COLS
        row = np.repeat(np.arange(piv_len.size), piv_len)
        new = np.r_[True, (rng_of[1:] != rng_of[:-1]) | (row[1:] != row[:-1])]
        occupied = np.bincount(row[new], minlength=piv_len.size)       # ranges the pivot has an entry in
    nranges = np.where(piv_len > 0, last - first + 1, 0)
    return dict(key_only=key_only, compact=compact, slot=slot, cap64=cap64, cap128=cap128, max_tab=max_tab, kernel=kern,
                length=piv_len, entries=ent_count, items=-(-ent_count // ITEM_ENTRIES),
                segments=np.where(kern == K_SEG, -(-piv_len // cap128), 1),
                ranges=nranges, occupied=occupied, first_range=np.where(piv_len > 0, first, 0),
                cached=nranges <= BITS_MAX_SEG)


def routes(case, dtype, layout, semiring, mask_csc=True):
    """The dispatch of grb_mxm for one call: per mask entry the `owner` (NOBODY: a zero in the mask) and the `kernel`
    (an index into KERNELS) that computes it, `shorter` (the length of the shorter of its two lists), per pass what
    _pass_kernels says of its pivots, and count[(owner, kernel name)] = entries."""
    sr = Semiring(semiring, dtype)
    order_free = sr.monoid.opname in ORDER_FREE
    plus, is_int = sr.monoid.opname == "plus", np.dtype(dtype) == np.int32
    la, lb = case.la[case.mrow], case.lb[case.mi]
    live = case.mask_values() != 0
    shorter = np.minimum(la, lb)
    owner = np.zeros(case.mi.size, dtype=np.int8)
    kernel = np.zeros(case.mi.size, dtype=np.int8)
    passes = {}
    if not pivot_on() or not order_free:
        owner[live] = ENTRY_ALONE
        kernel[live] = np.where(order_free & (shorter > LANE_DOT_MAX), K_HEAVY, K_LANE)[live]
    else:
        iso_a = layout in ("iso_ab", "iso_a") and case.ai.size > 0
        iso_b = layout in ("iso_ab", "iso_b") and case.bi.size > 0
        first = live & (lb <= la)
        second = live & ~(lb <= la)
        passes[1] = _pass_kernels(case.la, np.diff(case.mp), case.ap, case.ai, iso_a, iso_b, is_int, plus)
        owner[first] = PASS1
        kernel[first] = passes[1]["kernel"][case.mrow[first]]
        if mask_csc:
            passes[2] = _pass_kernels(case.lb, np.bincount(case.mi, minlength=case.n), case.bp, case.bi, iso_b, iso_a,
                                      is_int, plus)
            owner[second] = PASS2
            kernel[second] = passes[2]["kernel"][case.mi[second]]
        else:
            owner[second] = ENTRY_B_LONGER
            kernel[second] = np.where(shorter > LANE_DOT_MAX, K_HEAVY, K_LANE)[second]
    count = {}
    for o, k in zip(owner[live], kernel[live]):
        count[(int(o), KERNELS[k])] = count.get((int(o), KERNELS[k]), 0) + 1
    return dict(owner=owner, kernel=kernel, shorter=shorter, passes=passes, count=count, order_free=order_free)


def owned(f, owner, kernel):
    return f["count"].get((owner, kernel), 0)


# ---- patterns ----------------------------------------------------------------------------------------------------------
def _mask_from(m, n, dense):
    rows, cols = np.nonzero(dense)
    return _csr([cols[rows == r] for r in range(m)])


def _comb(name, K, lengths, ma, nb, short_max, seed):
    rng = np.random.default_rng(seed)

    def side(nshort):
        rows = [np.sort(rng.choice(K, ln, replace=False)) for ln in lengths]
        rows += [np.sort(rng.choice(K, int(rng.integers(0, short_max + 1)), replace=False)) for _ in range(nshort)]
        rows[len(lengths) + 3] = np.zeros(0, dtype=np.int64)           # an empty row among the short ones
        return rows
    a, b = side(ma), side(nb)
    m, n, nl = len(a), len(b), len(lengths)
    dense = rng.random((m, n)) < 0.05
    dense[:nl, :] = True
    dense[:, :nl] = True
    return Case(name, m, n, K, _csr(a), _csr(b), _mask_from(m, n, dense))


@functools.lru_cache(maxsize=None)
def comb():
    c = _comb("comb", 40000, EDGE_LENGTHS, 200, 230, 40, seed=4101)
    assert (c.m, c.n) == (215, 245) and 8000 <= c.mi.size <= 10000 and np.any(c.la == 0) and np.any(c.lb == 0)
    if not pivot_on():                                          # (GRB_MXM_PIVOT=0: the entry-driven kernel alone, see routes())
        return c
    for case in (c, c.mirrored()):
        for dtype in DTYPES:
            for layout in LAYOUTS:
                f = routes(case, dtype, layout, "MinimumPlus")          # (never the bitmap: tables for every length)
                for p in (PASS1, PASS2):
                    # every table size of both slot sizes, in both passes, several hundred entries each
                    for k in ("wave", "table64", "table128", "segments"):
                        assert owned(f, p, k) >= 150, (case.name, layout, p, k, f["count"])
                    info = f["passes"][p]
                    length, kern = info["length"], info["kernel"]
                    side_iso = layout == "iso_ab" or layout == ("iso_a" if p == PASS1 else "iso_b")
                    assert info["key_only"] == side_iso and info["slot"] == (4 if side_iso else 8)
                    edges = {256: K_WAVE, 257: K_T64, info["cap64"]: K_T64, info["cap64"] + 1: K_T128,
                             info["cap128"]: K_T128, info["cap128"] + 1: K_SEG, 20000: K_SEG}
                    for ln, k in edges.items():                         # a pivot ON every edge, with entries of its own
                        r = int(np.flatnonzero(length == ln)[0])
                        piv = case.mrow if p == PASS1 else case.mi
                        assert kern[r] == k and np.any((f["owner"] == p) & (piv == r)), (layout, p, ln)
                    assert info["segments"][np.flatnonzero(length == 20000)[0]] >= 2
                    # a wave pivot whose owned entries reach into a second tile of 64 partners
                    mine = f["owner"] == p
                    piv = (case.mrow if p == PASS1 else case.mi)[mine]
                    assert np.any((np.bincount(piv, minlength=length.size) > WAVE_TILE) & (kern == K_WAVE))
            # the mixed layouts: key-only tables in one pass, (key, value) tables with a one-valued partner in the other
            f = routes(case, dtype, "iso_a", "PlusMinus")
            assert f["passes"][1]["key_only"] and not f["passes"][2]["key_only"] and not f["passes"][1]["compact"]
        # the bitmap line: int32, a plus monoid, both sides one-valued
        f = routes(case, np.int32, "iso_ab", "PlusMultiplies")
        if bitmap_min() == BITMAP_MIN:
            for p in (PASS1, PASS2):
                info = f["passes"][p]
                assert info["compact"] and info["max_tab"] == BITMAP_MIN
                assert info["kernel"][np.flatnonzero(info["length"] == 2048)[0]] == K_T64
                assert info["kernel"][np.flatnonzero(info["length"] == 2049)[0]] == K_BITMAP
                assert owned(f, p, "bitmap") >= 150 and owned(f, p, "table128") == 0 and owned(f, p, "segments") == 0
        for other in ((np.float32, "iso_ab", "PlusMultiplies"), (np.int32, "iso_ab", "MinimumPlus"),
                      (np.int32, "iso_a", "PlusMultiplies")):
            assert not any(k == "bitmap" for _, k in routes(case, *other)["count"])
        # without a CSC of the mask: the entry-driven kernel owns the B-longer entries, some on its whole-wave path
        f = routes(case, np.int32, "valued", "PlusMultiplies", mask_csc=False)
        assert owned(f, PASS2, "wave") == 0 and owned(f, ENTRY_B_LONGER, "heavy") >= 150 and owned(f, ENTRY_B_LONGER, "lane") >= 150
        # an ordered fold: the entry-driven kernel alone, a lane per entry, lists of 20000 entries among them
        f = routes(case, np.int32, "valued", "GreaterPlus")
        assert set(f["count"]) == {(ENTRY_ALONE, "lane")} and f["shorter"].max() == 20000
    return c


def _fan(name, K, pivots, npartners, seed):
    rng = np.random.default_rng(seed)
    a = [np.sort(rng.choice(K, ln, replace=False)) for ln in pivots]
    b = []
    for j in range(npartners):
        ln = int(rng.integers(0, 13))
        src = a[int(rng.integers(0, len(a)))]
        cols = np.where(rng.random(ln) < 0.7, rng.choice(src, ln), rng.integers(0, K, ln))   # mostly the pivot's columns
        b.append(np.unique(cols))
    m, n = len(a), npartners
    return Case(name, m, n, K, _csr(a), _csr(b), _csr([np.arange(n)] * m))


@functools.lru_cache(maxsize=None)
def fan():
    c = _fan("fan", 60000, (300, 5000, 20000), 4200, seed=4102)
    assert np.any(c.lb == 0) and c.lb.max() <= 12
    if not pivot_on():
        return c
    f = routes(c, np.float32, "valued", "PlusMinus")
    live = c.mask_values() != 0
    assert np.all(f["owner"][live] == PASS1)
    info = f["passes"][1]
    assert info["kernel"].tolist() == [K_T64, K_T128, K_SEG]
    assert np.all(info["entries"] > 4 * BLOCK_TILE) and np.all(info["items"] == 2)      # a second trip, a second item
    g = routes(c.mirrored(), np.float32, "valued", "PlusMinus")
    assert np.all(g["owner"][c.mirrored().mask_values() != 0] == PASS2) and np.all(g["passes"][2]["items"] == 2)
    g = routes(c.mirrored(), np.float32, "valued", "PlusMinus", mask_csc=False)
    assert set(g["count"]) == {(ENTRY_B_LONGER, "lane")}
    if bitmap_min() == BITMAP_MIN:
        f = routes(c, np.int32, "iso_ab", "PlusMultiplies")
        assert f["passes"][1]["kernel"].tolist() == [K_T64, K_BITMAP, K_BITMAP]
    return c


def _ranges(name, R, nranges, tail, pivot_spans, npartners, seed):
    """pivot_spans: for each pivot (entries, the ranges they are spread over).  Columns on both sides of every range
    boundary are put into the pivots whose ranges hold them, and into partners of their own."""
    rng = np.random.default_rng(seed)
    K = (nranges - 1) * R + tail
    hi = lambda r: min((r + 1) * R, K)
    edges = sorted({0, K - 1} | {r * R - 1 for r in range(1, nranges)} | {r * R for r in range(1, nranges)})
    a = []
    for count, spans in pivot_spans:
        take = [min(count // len(spans), (hi(r) - r * R) // 2) for r in spans]         # (the last range is a short one)
        take[0] += count - sum(take)
        cols = np.concatenate([r * R + rng.choice(hi(r) - r * R, t, replace=False) for r, t in zip(spans, take)])
        on_edge = [e for e in edges if e // R in spans]
        a.append(np.unique(np.r_[cols, on_edge]))
    b = [np.array([R - 1, R]), np.array([R - 1]), np.array([R]), np.zeros(0, dtype=np.int64), np.array([K - 1]), np.array(edges)]
    # a partner wholly inside range 1 (which the second pivot skips), half of it columns of the pivots that are there
    in1 = np.concatenate([p[(p >= R) & (p < hi(1))] for p in a])
    b.append(np.unique(np.r_[rng.choice(in1, min(in1.size, 60)), rng.integers(R, hi(1), 60)]))
    while len(b) < npartners:
        ln = int(rng.integers(1, max(2, min(400, R // 2))))
        src = a[int(rng.integers(0, len(a)))]
        cols = np.where(rng.random(ln) < 0.5, rng.choice(src, ln), rng.integers(0, K, ln))
        b.append(np.unique(np.r_[cols, rng.choice(edges, 2)]))
    m, n = len(a), len(b)
    return Case(name, m, n, K, _csr(a), _csr(b), _csr([np.arange(n)] * m))


def _bitmap_facts(case):
    """per pivot of pass 1 of the triangle-counting instantiation: (ranges, occupied ranges, first range, cached)"""
    f = routes(case, np.int32, "iso_ab", "PlusMultiplies")
    info = f["passes"][1]
    assert np.all(f["owner"][case.mask_values() != 0] == PASS1) and np.all(info["kernel"] == K_BITMAP) and info["compact"]
    g = routes(case.mirrored(), np.int32, "iso_ab", "PlusMultiplies")
    assert np.all(g["owner"][case.mirrored().mask_values() != 0] == PASS2) and np.all(g["passes"][2]["kernel"] == K_BITMAP)
    return [tuple(int(info[k][r]) for k in ("ranges", "occupied", "first_range", "cached")) for r in range(case.m)]


@functools.lru_cache(maxsize=None)
def ranges4():
    R = BITMAP_COLS
    c = _ranges("ranges4", R, 4, 12345, [(3000, (0, 1, 2, 3)), (2600, (0, 2)), (2700, (1, 2, 3)), (2400, (1, 3))], 100, seed=4103)
    assert c.K == 3 * R + 12345 and c.lb.max() <= 2048 < c.la.min()
    if pivot_on() and bitmap_min() == BITMAP_MIN:
        # all four cached; an empty range between two others; a first range that is not 0, then an empty one
        assert _bitmap_facts(c) == [(4, 4, 0, 1), (3, 2, 0, 1), (3, 3, 1, 1), (3, 2, 1, 1)]
    rows = [c.bi[c.bp[j]:c.bp[j + 1]] for j in range(c.n)]
    assert any(r.size > 50 and r[0] >= R and r[-1] < 2 * R for r in rows)   # a partner wholly inside the range pivot 1 skips
    for e in (R - 1, R, 2 * R - 1, 2 * R, 3 * R - 1, 3 * R):            # both sides of every boundary: in pivots AND partners
        assert np.count_nonzero(c.ai == e) >= 2 and np.count_nonzero(c.bi == e) >= 2
    return c


@functools.lru_cache(maxsize=None)
def ranges10():
    R = BITMAP_COLS
    c = _ranges("ranges10", R, 10, 777, [(3000, tuple(range(10))), (2200, (0, 9)), (2300, (4, 5))], 100, seed=4104)
    assert c.K == 9 * R + 777 and c.lb.max() <= 2048 < c.la.min()
    if pivot_on() and bitmap_min() == BITMAP_MIN:
        # ten ranges and ten with eight skipped: searched per range; two ranges from range 4: cached
        assert _bitmap_facts(c) == [(10, 10, 0, 0), (10, 2, 0, 0), (2, 2, 4, 1)]
    return c


def _tiny(name, a, b, mask, K, mask_zero=False):
    return Case(name, len(a), len(b), K, _csr(a), _csr(b), _csr(mask), mask_zero)


def _tiny_side(rng, nrows, K):
    return [np.sort(rng.choice(K, int(rng.integers(1, 9)), replace=False)) for _ in range(nrows)]


@functools.lru_cache(maxsize=None)
def degenerate():
    """name -> case: A empty, B empty, every mask value zero, 1 x 1, an empty pivot row with a non-empty partner"""
    rng = np.random.default_rng(4105)
    K, none = 30, np.zeros(0, dtype=np.int64)
    full = lambda m, n: [np.arange(n)] * m
    a, b = _tiny_side(rng, 5, K), _tiny_side(rng, 6, K)
    out = {
        "Za": _tiny("Za", [none] * 5, b, full(5, 6), K),
        "Zb": _tiny("Zb", a, [none] * 6, full(5, 6), K),
        "Zm": _tiny("Zm", a, b, full(5, 6), K, mask_zero=True),
        "Z1": _tiny("Z1", [np.array([0])], [np.array([0])], [np.array([0])], 1),
        "Ze": _tiny("Ze", [none, a[1]], [b[0], np.arange(K)], full(2, 2), K),
    }
    assert out["Ze"].la[0] == 0 and out["Ze"].lb[0] > 0
    return out


# reduced instances of the same builders, small enough for the oracle's loop per common column
@functools.lru_cache(maxsize=None)
def comb_small():
    return _comb("comb_s", 3000, (17, 64, 65, 256, 257, 300), 14, 17, 12, seed=4111)


@functools.lru_cache(maxsize=None)
def fan_small():
    return _fan("fan_s", 3000, (30, 120, 300), 90, seed=4112)


@functools.lru_cache(maxsize=None)
def ranges_small():
    return _ranges("ranges_s", 800, 4, 45, [(90, (0, 1, 2, 3)), (60, (0, 2)), (70, (1, 2, 3)), (50, (1, 3))], 30, seed=4113)


CASES = {"comb": comb, "fan": fan, "ranges4": ranges4, "ranges10": ranges10}
SMALL_CASES = {"comb_s": comb_small, "fan_s": fan_small, "ranges_s": ranges_small}


def get(name):
    """a case by name; a trailing ~ is the mirrored one"""
    base = name.rstrip("~")
    case = CASES[base]() if base in CASES else SMALL_CASES[base]() if base in SMALL_CASES else degenerate()[base]
    return case.mirrored() if name.endswith("~") else case


# ---- operands ----------------------------------------------------------------------------------------------------------
ISO_VALUES = (3, 2)                     # A's and B's one value
ISO_VALUES_TIMES = (1, -1)              # ... under the Multiplies monoid (6^k would not stay exact)
IDENT_COLS = 61                         # MinimumPlus / MinimumMultiplies: columns = 5 mod 61 hold A's identities, 6 mod 61 B's


def _arith(sr):
    return sr.mulname in ("plus", "minus", "multiplies", "divides")


def _draw_side(rng, sr, ptr, ind, side):
    nv = ind.size
    mono = sr.monoid.opname
    if mono == "multiplies":
        # 1 throughout, to every row at most four 2s, one -1 and (a row in three) one 0: a product over up to 20000
        # common columns stays below 2^8 in magnitude
        v = np.ones(nv, dtype=np.int64)
        for r in np.flatnonzero(np.diff(ptr) > 0):
            s, e = int(ptr[r]), int(ptr[r + 1])
            v[rng.integers(s, e, 4)] = 2
            v[rng.integers(s, e)] = -1
            if rng.random() < 0.33:
                v[rng.integers(s, e)] = 0
        return v
    if sr.mulname == "divides":
        if side == "B":                                         # the divisor: a power of two, never 0
            return (1 << rng.integers(0, 4, nv)) * rng.choice([-1, 1], nv)
        return rng.integers(-4, 5, nv)
    if mono in ("minimum", "maximum"):
        return rng.integers(-1000, 1001, nv)
    return rng.integers(-3, 5, nv)


def operands(case, sr_name, dtype, layout):
    """(A's values, B's values) in `dtype`, in the order of case.ai / case.bi"""
    sr = Semiring(sr_name, dtype)
    ident = sr.identity()
    rng = np.random.default_rng(_seed(case.name, sr_name, np.dtype(dtype).name, layout))
    iso = ISO_VALUES_TIMES if sr.monoid.opname == "multiplies" else ISO_VALUES
    small_ident = abs(float(ident)) <= 8
    out = []
    for side, ptr, ind, one in (("A", case.ap, case.ai, iso[0]), ("B", case.bp, case.bi, iso[1])):
        if layout == "iso_ab" or layout == "iso_" + side.lower():
            out.append(np.full(ind.size, one, dtype=dtype))
            continue
        v = _draw_side(rng, sr, ptr, ind, side).astype(dtype)
        divisor = sr.mulname == "divides" and side == "B"
        if (small_ident or not _arith(sr)) and not divisor and sr.monoid.opname != "multiplies":
            v[rng.random(ind.size) < 0.04] = ident             # the identity itself: 0, 1, FLT_MAX / INT_MAX
        if ind.size >= 2 and not divisor and sr.monoid.opname != "multiplies":
            v[0], v[-1] = -2, 3                                 # never one value throughout
        out.append(v)
    if layout == "valued" and _arith(sr) and not small_ident and sr.monoid.opname == "minimum" and sr.mulname in ("plus", "multiplies"):
        neutral = 0 if sr.mulname == "plus" else 1
        av, bv = out
        av[case.ai % IDENT_COLS == 5], bv[case.bi % IDENT_COLS == 5] = ident, neutral
        av[case.ai % IDENT_COLS == 6], bv[case.bi % IDENT_COLS == 6] = neutral, ident
    for v, key in zip(out, ("iso_a", "iso_b")):
        if v.size >= 2:
            assert (np.unique(v).size == 1) == (layout in ("iso_ab", key)), (case.name, sr_name, layout)
    return out[0], out[1]


def mask_array(case, dtype):
    return case.mask_values().astype(dtype)


# ---- reference ---------------------------------------------------------------------------------------------------------
def want(case, sr_name, dtype, av, bv, check_exact=True):
    """C's values on the mask's structure: the fold over the common columns where the mask's value is not zero, the
    semiring's identity elsewhere.  The multiply is oracle.semiring's in `dtype` itself (asserted to be what the wide
    type gives); the commutative monoids are folded in float64 / int64 with every partial result in any order exact
    (asserted), the comparison ones by add(product, acc) over k ascending."""
    sr = Semiring(sr_name, dtype)
    ea, eb, ptr = case.join()
    a, b = np.asarray(av)[ea], np.asarray(bv)[eb]
    assert a.dtype == dtype and b.dtype == dtype
    prod = sr.mul_op(a, b)
    wide_t = np.float64 if np.issubdtype(np.dtype(dtype), np.floating) else np.int64
    if check_exact and prod.size:
        with np.errstate(divide="ignore", invalid="ignore"):
            wide = np.asarray(BINARY_OPS[sr.mulname](a.astype(wide_t), b.astype(wide_t))).astype(wide_t)
        assert np.array_equal(prod.astype(wide_t), wide), (case.name, sr_name)        # no overflow, no rounding
    if sr.monoid.opname in ORDER_FREE:
        # (minimum / maximum / or accumulate nothing: every result is one of the products, or the identity)
        full = fold_rows(sr, ptr, prod, check_exact and sr.monoid.opname in ("plus", "multiplies"))
        out = full.astype(dtype)
        if check_exact:
            assert np.array_equal(out.astype(wide_t), full), (case.name, sr_name)
    else:
        out = fold_ascending(sr, prod, ptr, dtype)
    return np.where(case.mask_values() != 0, out, sr.identity()).astype(dtype)


def common_columns(case):
    """per mask entry, the number of columns its two rows share"""
    return np.diff(case.join()[2])


def want_real(case, av, bv):
    """(sum of a b, sum of |a b|) per mask entry in float64 for PlusMultiplies on real values; 0 where the mask is 0"""
    ea, eb, ptr = case.join()
    p = np.asarray(av, dtype=np.float64)[ea] * np.asarray(bv, dtype=np.float64)[eb]
    s, mag = np.zeros(ptr.size - 1), np.zeros(ptr.size - 1)
    nz = np.diff(ptr) > 0
    s[nz] = np.add.reduceat(p, ptr[:-1][nz])
    mag[nz] = np.add.reduceat(np.abs(p), ptr[:-1][nz])
    live = case.mask_values() != 0
    return np.where(live, s, 0.0), np.where(live, mag, 0.0)


def gamma(n):
    """n u / (1 - n u) with u = 2^-24: the bound of a float32 sum of n - 1 rounded products in any order"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def stored(case, tran_a, tran_b, av, bv):
    """The two matrices to BUILD for one orientation: (nrows, ncols, ptr, ind, values) of A and of B.  op(A) is m x K
    and op(B) is K x n: with GrB_INP1 transposed B is stored as its rows (n x K), otherwise as their transpose."""
    a = (case.m, case.K, case.ap, case.ai, av)
    b = (case.n, case.K, case.bp, case.bi, bv)
    if tran_a:
        tp, ti, perm = transpose(case.m, case.K, case.ap, case.ai)
        a = (case.K, case.m, tp, ti, av[perm])
    if not tran_b:
        tp, ti, perm = transpose(case.n, case.K, case.bp, case.bi)
        b = (case.K, case.n, tp, ti, bv[perm])
    return a, b


# ---- one call on the library `g` (the GPU tests, and the child process of the static switches) -----------------------
def build(g, spec, dtype):
    nrows, ncols, ptr, ind, val = spec
    M = g.Matrix(nrows, ncols, dtype)
    assert M.build_csr(ptr, ind, np.asarray(val).astype(dtype)) == 0
    return M


def build_mask(g, case, mask_dtype):
    return build(g, (case.m, case.n, case.mp, case.mi, case.mask_values()), mask_dtype)


def product(g, case, dtype, sr_name, av, bv, mask, tran_a=0, tran_b=1, out=None):
    """C's values of C<mask> = op(A) (+.x) op(B) for one orientation (the default: GrB_INP1 transposed, as tc() calls
    it); info 0 and the mask's structure are asserted"""
    a, b = stored(case, tran_a, tran_b, av, bv)
    A, B = build(g, a, dtype), build(g, b, dtype)
    d = g.Descriptor()
    assert d.loadArgs() == 0
    if tran_a:
        assert d.toggle(g.GrB_INP0) == 0
    if tran_b:
        assert d.toggle(g.GrB_INP1) == 0
    Cm = g.Matrix(case.m, case.n, dtype) if out is None else out
    info = g.mxm(Cm, mask, None, sr_name, A, B, d)
    assert info == 0, (case.name, sr_name, info)
    cp, ci, cv = Cm.host_csr()
    assert Cm.nvals() == case.mi.size and np.array_equal(cp, case.mp) and np.array_equal(ci, case.mi), (case.name, sr_name)
    assert cv.dtype == dtype
    return cv


def mismatches(case, dtype, layout, sr_name, got, ref, mask_csc=True):
    """None when got == ref bit for bit (the sign of a zero aside under a min / max monoid), otherwise a description:
    how many entries differ, which kernels own them, the first few"""
    if np.dtype(dtype) == np.float32 and Semiring(sr_name, dtype).monoid.opname in ("minimum", "maximum"):
        got, ref = got + dtype(0), ref + dtype(0)               # min / max of -0.0 and +0.0 is either, by the fold's order
    bad = np.flatnonzero(got.view(np.uint32) != ref.view(np.uint32))
    if bad.size == 0:
        return None
    f = routes(case, dtype, layout, sr_name, mask_csc)
    where = sorted({(int(f["owner"][e]), KERNELS[f["kernel"][e]]) for e in bad})
    first = [(int(case.mrow[e]), int(case.mi[e]), got[e].item(), ref[e].item()) for e in bad[:4]]
    return "%s %s %s %s: %d of %d entries differ, (owner, kernel) %s, first (i, j, got, want) %s" % (
        case.name, np.dtype(dtype).name, layout, sr_name, bad.size, got.size, where, first)
