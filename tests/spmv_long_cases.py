"""Matrices, operands and the host reference for the SpMV tests on input vectors longer than the LDS prefix
(tests/test_gpu_spmv_long_vectors.py on the GPU, tests/test_spmv_long_reference.py on the CPU).

k_spmv (csrc/spmv.hip) stages the 32768 first values of the input vector in LDS.  With a longer vector it either
renames the columns by reference count (the 32768 most referenced ones hold at least 1/8 of the entries) or, on a
flat matrix, gathers everything from memory; the column-sorted format is a fourth route.  Rectangular matrices
reach all of them with a host reference of some 60 k entries:

  W  wide   3000 x 40000   every column referenced, 200 hub columns, rows of 1300 / 512 / 513 entries, empty ends
  N  flat   1500 x 300000  every column exactly once, 200 to a row
  P  plain  1000 x 1000    W's shape in small: the whole vector fits the prefix

Everything is built from fixed seeds, and the conditions the routes depend on are asserted here in numpy, so a
change of seed cannot silently leave a route.  Data are small integers (or dyadic quotients): every partial sum
in any order is exact in float32 and in int32, and the reference -- rows folded in float64 / int64 by reduceat,
the multiply taken from oracle.semiring so that the operand order is the oracle's -- is compared bit for bit.
"""
import functools

import numpy as np

from oracle.semiring import Semiring

HOT = 32768           # kHot of csrc/spmv.hip: values of the (packed) input vector kept in LDS
TILE = 512            # kWaveTile: entries of one wave tile; a longer row is cut into slices of this size
TILE_ROWS = 64        # kWaveRows
EXACT = 1 << 24       # integers below this magnitude are exact in float32

# the 13 semirings over a commutative monoid; the comparison "monoids" (GreaterPlus, CustomLessPlus, NotEqualToPlus,
# CustomLessLess) depend on the reduction tree, which no reference defines
COMMUTATIVE = ["LogicalOrAnd", "PlusMultiplies", "MinimumPlus", "MaximumMultiplies", "PlusDivides", "PlusGreater",
               "PlusMinus", "PlusLess", "MinimumMultiplies", "MultipliesMultiplies", "MinimumSelectSecond",
               "PlusNotEqualTo", "MinimumNotEqualTo"]
DTYPES = [np.float32, np.int32]


def wave_tiles(ptr):
    """(row_start, row_end, is_slice) of the wave tiles build_spmv_plan cuts: <= 512 entries and <= 64 rows, a row
    of more than 512 entries in slices of its own"""
    ptr = np.asarray(ptr, dtype=np.int64)
    n = ptr.size - 1
    tiles = []
    r = 0
    while r < n:
        length = ptr[r + 1] - ptr[r]
        if length > TILE:
            tiles += [(r, r + 1, True)] * int(-(-length // TILE))
            r += 1
            continue
        start, nnz = r, 0
        while r < n and r - start < TILE_ROWS and nnz + ptr[r + 1] - ptr[r] <= TILE:
            nnz += ptr[r + 1] - ptr[r]
            r += 1
        tiles.append((start, r, False))
    return tiles


class Case:
    """One sparsity pattern in both orientations.  tran = 0: the rows of A (mxv), tran = 1: the rows of A' (vxm)."""

    def __init__(self, name, nrows, ncols, ptr, ind):
        self.name, self.nrows, self.ncols = name, int(nrows), int(ncols)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.ind = np.ascontiguousarray(ind, dtype=np.int32)
        self.nvals = int(self.ind.size)
        assert self.ptr.size == self.nrows + 1 and self.ptr[0] == 0 and self.ptr[-1] == self.nvals
        rows = np.repeat(np.arange(self.nrows, dtype=np.int64), np.diff(self.ptr))
        # no duplicates, columns ascending inside a row
        key = rows * self.ncols + self.ind
        assert np.all(np.diff(key) > 0)
        # the transposed orientation by a stable sort on the column: rows ascending inside a column
        self.perm = np.argsort(self.ind, kind="stable")
        self.tind = rows[self.perm].astype(np.int32)
        self.col_count = np.bincount(self.ind, minlength=self.ncols)
        self.tptr = np.zeros(self.ncols + 1, dtype=np.int32)
        np.cumsum(self.col_count, out=self.tptr[1:])

    def arrays(self, tran, vals):
        """(ptr, ind, values, rows of the result, length of the input vector) of one orientation"""
        if tran:
            return self.tptr, self.tind, vals[self.perm], self.ncols, self.nrows
        return self.ptr, self.ind, vals, self.nrows, self.ncols

    def hot_refs(self, tran):
        """entries held by the 32768 most referenced columns of this orientation (device_rank_columns' hot_refs)"""
        counts = np.diff(self.ptr) if tran else self.col_count
        return int(np.sort(counts)[::-1][:HOT].sum())


def _skewed(name, nrows, ncols, long_len, empty_run, nhubs, hubs_per_row, seed):
    """Every column dealt once over the ordinary rows, plus `hubs_per_row` of `nhubs` hub columns drawn with Zipf
    weights for each of them; row 0 and the last row empty, a run of empty rows, rows of long_len / 512 / 513."""
    rng = np.random.default_rng(seed)
    special = {7: long_len, 11: TILE, 12: TILE + 1}
    run0 = nrows // 3
    empty = {0, nrows - 1} | set(range(run0, run0 + empty_run))
    ordinary = np.array([r for r in range(nrows) if r not in empty and r not in special])
    owner = ordinary[np.arange(ncols) % ordinary.size]          # column c of a random order goes to this row
    order = rng.permutation(ncols)
    dealt = {int(r): [] for r in ordinary}
    for c, r in zip(order, owner):
        dealt[int(r)].append(int(c))
    hubs = rng.choice(ncols, nhubs, replace=False)
    weight = 1.0 / np.arange(1, nhubs + 1)
    weight /= weight.sum()
    rows = []
    for r in range(nrows):
        if r in empty:
            cols = np.zeros(0, dtype=np.int64)
        elif r in special:
            cols = rng.choice(ncols, special[r], replace=False)
        else:
            cols = np.union1d(dealt[r], hubs[rng.choice(nhubs, hubs_per_row, replace=False, p=weight)])
        rows.append(np.sort(cols))
    ptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum([c.size for c in rows], out=ptr[1:])
    case = Case(name, nrows, ncols, ptr, np.concatenate(rows))
    lens = np.diff(case.ptr)
    assert lens[0] == 0 and lens[-1] == 0 and lens[7] == long_len and lens[11] == TILE and lens[12] == TILE + 1
    assert np.all(case.col_count >= 1)                          # every column referenced
    tiles = wave_tiles(case.ptr)
    assert any(not s and case.ptr[b] == case.ptr[a] and b - a == TILE_ROWS for a, b, s in tiles)   # an all-empty tile
    assert sum(1 for a, _, s in tiles if s and a == 7) == -(-long_len // TILE) and long_len % TILE
    # the transposed orientation has long rows of its own: hub columns past one slice, the last slice partial
    assert np.count_nonzero(case.col_count > TILE) >= 2 and np.any(case.col_count[case.col_count > TILE] % TILE)
    return case


@functools.lru_cache(maxsize=None)
def wide():
    c = _skewed("W", 3000, 40000, 1300, 200, 200, 7, seed=20240)
    assert 55000 <= c.nvals <= 65000, c.nvals
    assert np.count_nonzero(c.col_count) > HOT                  # cold gathers really happen ...
    assert np.sort(c.col_count)[::-1][HOT] >= 1                 # ... and the column of rank exactly 32768 is one
    assert c.hot_refs(0) * 8 >= c.nvals                         # hub packing is taken (prepare_hub_packing)
    return c


@functools.lru_cache(maxsize=None)
def plain():
    c = _skewed("P", 1000, 1000, 1000, 130, 8, 5, seed=20241)
    assert c.ncols <= HOT and c.nrows <= HOT                    # both orientations: the whole vector in LDS
    return c


@functools.lru_cache(maxsize=None)
def flat():
    nrows, ncols, per = 1500, 300000, 200
    rng = np.random.default_rng(20242)
    ind = np.sort(rng.permutation(ncols).reshape(nrows, per), axis=1).ravel()
    c = Case("N", nrows, ncols, np.arange(nrows + 1, dtype=np.int64) * per, ind)
    assert c.nvals == ncols and np.all(c.col_count == 1)
    assert c.hot_refs(0) == HOT and c.hot_refs(0) * 8 < c.nvals  # flat: the natural column order is kept, nhot = 0
    return c


CASES = {"W": wide, "N": flat, "P": plain}


# ---- operands ------------------------------------------------------------------------------------------------------
def _seed(*what):
    """a seed from names and flags that does not change between runs (hash() of a string does)"""
    return sum((i + 1) * sum(str(w).encode()) for i, w in enumerate(what)) % (1 << 31)


def values(case, sr, iso):
    """the stored values as integers: 1..4 (one value for the iso twin); MultipliesMultiplies: mostly 1"""
    rng = np.random.default_rng(_seed(case.name, "values", sr == "MultipliesMultiplies"))
    if sr == "MultipliesMultiplies":
        return np.ones(case.nvals, dtype=np.int64) if iso else 1 + (rng.random(case.nvals) < 0.002).astype(np.int64)
    return np.full(case.nvals, 3, dtype=np.int64) if iso else rng.integers(1, 5, case.nvals)


def vector(case, tran, sr, attempt=0):
    """the input vector as integers: 0..1000; PlusDivides: powers of two in 1..8 (dyadic quotients, no division by
    zero); MultipliesMultiplies: 1 with a few 2 and very few 0"""
    n = case.nrows if tran else case.ncols
    rng = np.random.default_rng(_seed(case.name, "vector", tran, sr in ("PlusDivides", "MultipliesMultiplies"), attempt))
    if sr == "PlusDivides":
        return 1 << rng.integers(0, 4, n)
    if sr == "MultipliesMultiplies":
        x = rng.random(n)
        return np.where(x < 0.0003, 0, np.where(x < 0.0023, 2, 1)).astype(np.int64)
    return rng.integers(0, 1001, n)


def start_and_masks(case, tran, sr):
    """(w before the product: non-zero integers, the mask as 0 / 1) for the result's length"""
    n = case.ncols if tran else case.nrows
    rng = np.random.default_rng(_seed(case.name, "w0", tran))
    w0 = rng.integers(1, 3 if sr == "MultipliesMultiplies" else 6, n)
    mask = (rng.random(n) < 0.5).astype(np.int64)
    return w0, mask


# ---- reference -----------------------------------------------------------------------------------------------------
_FOLD = {"plus": np.add, "multiplies": np.multiply, "minimum": np.minimum, "maximum": np.maximum}


def fold_rows(sr, ptr, prod, check_exact=True):
    """identity (+) the products of every row, in float64 / int64; the result in the wide type"""
    wide_t = np.float64 if np.issubdtype(sr.dtype, np.floating) else np.int64
    n = ptr.size - 1
    ident = wide_t(sr.identity())
    out = np.full(n, ident, dtype=wide_t)
    nz = np.diff(ptr) > 0
    starts = ptr[:-1][nz].astype(np.int64)
    p = prod.astype(wide_t)
    name = sr.monoid.opname
    if name == "logical_or":
        red = (np.add.reduceat((p != 0).astype(np.int64), starts) > 0).astype(wide_t)
        out[nz] = np.maximum(red, (ident != 0).astype(wide_t))
        return out
    uf = _FOLD[name]
    out[nz] = uf(ident, uf.reduceat(p, starts))
    if check_exact:
        # every partial result in ANY order is an integer (or a multiple of 1/8) below 2^24: exact in float32, no
        # overflow in int32
        if name == "plus":
            bound = np.add.reduceat(np.abs(p), starts)
        elif name == "multiplies":
            bound = np.multiply.reduceat(np.maximum(np.abs(p), 1), starts)
        else:
            bound = np.zeros(1)
        assert np.all(bound < EXACT), (sr.name, float(bound.max()))
        assert np.all(p * 8 == np.round(p * 8))
    return out


def want(case, tran, sr_name, dtype, vals, u, mask=None, scmp=0, accum=0, w0=None, check_exact=True):
    """w = A (+.x) u of one orientation with the mask / accumulate epilogue of spmv_store: where the mask FAILS the
    value is the semiring's identity (backend/cuda/spmv.hpp:203-212), the accumulation is the semiring's add (:213-220)"""
    sr = Semiring(sr_name, dtype)
    ptr, ind, v, nout, nin = case.arrays(tran, np.asarray(vals))
    u = np.asarray(u)
    assert u.size == nin
    prod = sr.mul_op(v.astype(dtype), u.astype(dtype)[ind])     # mul(matrix value, vector value), in the type itself
    full = fold_rows(sr, ptr, prod, check_exact)
    if check_exact:
        finite = np.abs(full) < EXACT
        assert np.all(finite | (full == full.dtype.type(sr.identity()))), sr_name
    out = full.astype(dtype)
    if mask is not None:
        passes = (np.asarray(mask) == 0) if scmp else (np.asarray(mask) != 0)
        out = np.where(passes, out, sr.identity()).astype(dtype)
    if accum:
        out = sr.add_op(np.asarray(w0).astype(dtype), out)
        if check_exact and sr.monoid.opname in ("plus", "multiplies"):
            assert np.all(np.abs(out.astype(np.float64)) < EXACT), sr_name
    assert out.size == nout
    return out


def operands(case, tran, sr, iso=False):
    """(values, vector, w0, mask) as integer arrays for which every row's result is exact; MultipliesMultiplies
    redraws its vector until every row's product stays below 2^24"""
    vals = values(case, sr, iso)
    w0, mask = start_and_masks(case, tran, sr)
    for attempt in range(20):
        u = vector(case, tran, sr, attempt)
        try:
            want(case, tran, sr, np.int32, vals, u, None, 0, 1, w0)
            return vals, u, w0, mask
        except AssertionError:
            if sr != "MultipliesMultiplies":
                raise
    raise AssertionError("no exact MultipliesMultiplies operands for " + case.name)


# the epilogue variants: (name, mask used, scmp, accum)
VARIANTS = {"none": (0, 0, 0), "mask": (1, 0, 0), "scmp": (1, 1, 0), "accum": (0, 0, 1), "scmp+accum": (1, 1, 1),
            "mask+accum": (1, 0, 1)}
