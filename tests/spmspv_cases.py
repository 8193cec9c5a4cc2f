"""Patterns, operands, the host reference and a model of the routes for the tests of the push product (SpMSpV:
csrc/spmspv.hip on top of csrc/push_common.hpp) -- tests/test_gpu_spmspv_shapes.py on the GPU,
tests/test_spmspv_reference.py on the CPU.

The push runs in four stages, and each changes behaviour at a size:

  degree + tile scan          DEG_TILE = 1024 frontier entries to a scan tile; with one tile the scan of the tile sums
                              is skipped, with more than 256 tiles push_scan_tiles_kernel loops with a carry
  partition                   EDGE_CHUNK = 2048 expanded edges to a chunk; chunk_owner[c] by binary search
  expansion                   a chunk whose frontier range [k0, k1] holds more than SEG_MAX = 2048 entries leaves the
                              LDS-staged owner map for a search per edge; with more than MAX_GRID = 2048 chunks a
                              workgroup takes a second chunk and reuses its LDS
  ordered bitmap compaction   WORD_TILE = 256 words (8192 outputs) to a tile; more than 256 tiles: the carry loop again

A pattern is the CSR of the matrix M that the push walks: its rows are indexed by the frontier, its columns are the
outputs.  vxm on A = M walks A's CSR, mxv on A = M' walks A's CSC; both are the same product.  What each pattern
is for -- and so what would no longer be covered without it:

  S   1000 x 1000, 37 frontier rows      one tile of everything; the anchor against the oracle
  E0  6000 x 20011, ~5000 frontier rows  the chunk edges, laid out by hand in frontier order (see chunk_edges):
  E1                                     empty rows in front, a running total of exactly 2048 at a row boundary, a
                                         scan-tile boundary inside a staged chunk, a hub of 5000 from the middle of a
                                         chunk over two whole ones, a hub of exactly 2048 on a chunk boundary, 2600
                                         empty rows between two rows of one chunk (range > SEG_MAX: the search per
                                         edge; a scan tile of sum 0), empty rows behind; 3 bitmap tiles, the last word
                                         partial.  Total == 0 (E0) and == 1 (E1) modulo 2048: a full last chunk and a
                                         last chunk of one edge
  T   300100 x 50021, 300000 rows        294 scan tiles: the carry of the tile-sum scan, stretches of empty rows over
                                         whole tiles on both sides of it
  B   3000 x 2200001, 2000 rows          269 bitmap tiles: the carry in the compaction's scan; the first word, the last
                                         (one valid bit) and the words on both sides of the carry are hit
  D   2100 x 2100 full, every row        4 410 000 edges, 2154 chunks: past the grid cap, every row a hub over a chunk
                                         boundary, 2100 combines into every output
  Z1 / Z0 / Zn                           one row of one entry; one empty row; only empty rows (nvals == 0, info 0)

routes() restates push_degree_kernel / push_partition_kernel in numpy, and every builder asserts from it the facts it
exists for: a changed seed or constant cannot leave a route unnoticed.

Data are small integers, dyadic quotients for PlusDivides, and {0, 1, 2} with a bounded number of 2s to an output
for MultipliesMultiplies: every partial result in any order is exact in float32 and in int32 (asserted), so the
reference -- the multiply from oracle.semiring with the identity short-circuit, each output folded in float64 /
int64, then the epilogue of the reference's spmspv.hpp:199-243 as oracle/ops.py:_spmspv_merge restates it -- is
compared bit for bit.  Every semiring gets operands equal to its identity on both sides (0, FLT_MAX / INT_MAX, 1)
and negative values.

Out of scope: the grid loop of push_partition_kernel (more than 262 144 chunks), 32-bit overflow of the expanded-edge
total, NaN / Inf data, and the four comparison "monoids", whose result depends on a fold order atomics do not define.
"""
import functools

import numpy as np

from oracle.semiring import Semiring
from spmv_long_cases import COMMUTATIVE, DTYPES, EXACT

DEG_TILE = 1024       # kDegTile = kBlock * kDegItems of csrc/push_common.hpp: frontier entries per scan tile
EDGE_CHUNK = 2048     # kEdgeChunk = kBlock * kEdgeItems: expanded edges per chunk
SEG_MAX = 2048        # kSegMax = kEdgeChunk: frontier entries lb_expand_kernel stages in LDS for one chunk
WORD_TILE = 256       # kBlock of csrc/common.hpp: bitmap words per workgroup of bitmap_count_kernel / bitmap_write_kernel
SCAN_BLOCK = 256      # kBlock again: tile sums push_scan_tiles_kernel scans per turn of its carry loop
MAX_GRID = 2048       # the cap of egrid in lb_run: workgroups of lb_expand_kernel

ORIENTS = ["vxm", "mxv"]
MASKS = ["none", "dense", "dense+scmp", "sparse"]          # (mask kind, scmp) = MASK_ARGS[name]
MASK_ARGS = {"none": ("none", 0), "dense": ("dense", 0), "dense+scmp": ("dense", 1), "sparse": ("sparse", 0)}
# one semiring for each combine of atomic_combine: atomicAdd, atomicMin, atomicMax, plain store, CAS loop
COMBINES = ["PlusMultiplies", "MinimumPlus", "MaximumMultiplies", "LogicalOrAnd", "MultipliesMultiplies"]


class Case:
    """The CSR of M (rows: frontier, columns: outputs) and the frontier's row ids, ascending."""

    def __init__(self, name, nrows, ncols, ptr, ind, fidx):
        self.name, self.nrows, self.ncols = name, int(nrows), int(ncols)
        self.ptr = np.ascontiguousarray(ptr, dtype=np.int32)
        self.ind = np.ascontiguousarray(ind, dtype=np.int32)
        self.fidx = np.ascontiguousarray(fidx, dtype=np.int32)
        self.nvals, self.nf = int(self.ind.size), int(self.fidx.size)
        assert self.ptr.size == self.nrows + 1 and self.ptr[0] == 0 and self.ptr[-1] == self.nvals
        assert np.all(np.diff(self.ptr) >= 0) and self.nf >= 1
        assert np.all(np.diff(self.fidx) > 0) and 0 <= self.fidx[0] and self.fidx[-1] < self.nrows
        if self.nvals:
            assert 0 <= self.ind.min() and self.ind.max() < self.ncols
        lens = np.diff(self.ptr).astype(np.int64)
        self.full = self.nvals == self.nrows * self.ncols
        if self.full:
            assert np.array_equal(self.ind, np.tile(np.arange(self.ncols, dtype=np.int32), self.nrows))
        else:
            key = np.repeat(np.arange(self.nrows, dtype=np.int64), lens) * self.ncols + self.ind
            assert np.all(np.diff(key) > 0)                     # no duplicates, columns ascending inside a row
        # the expanded edges of the frontier, in the order the kernel numbers them
        self.deg = lens[self.fidx]
        self.scan = np.cumsum(self.deg) - self.deg              # exclusive
        self.total = int(self.deg.sum())
        self.owner = np.repeat(np.arange(self.nf), self.deg)    # frontier position of every edge
        self.epos = self.ptr[self.fidx].astype(np.int64)[self.owner] + np.arange(self.total) - self.scan[self.owner]
        self.dest = self.ind[self.epos].astype(np.int64)
        self.col_count = np.bincount(self.dest, minlength=self.ncols)
        self._t = None

    def transposed(self):
        """(ptr, ind, perm) of M': what the matrix of the mxv orientation is built from, values = vals[perm]"""
        if self._t is None:
            if self.full:
                perm = np.arange(self.nvals, dtype=np.int64).reshape(self.nrows, self.ncols).T.ravel()
                tind = np.tile(np.arange(self.nrows, dtype=np.int32), self.ncols)
                tptr = np.arange(self.ncols + 1, dtype=np.int64) * self.nrows
            else:
                perm = np.argsort(self.ind, kind="stable")
                tind = np.repeat(np.arange(self.nrows, dtype=np.int32), np.diff(self.ptr))[perm]
                tptr = np.zeros(self.ncols + 1, dtype=np.int64)
                np.cumsum(np.bincount(self.ind, minlength=self.ncols), out=tptr[1:])
            self._t = (tptr.astype(np.int32), tind, perm)
        return self._t

    def matrix_arrays(self, orient, vals):
        """(nrows, ncols, ptr, ind, values) of the matrix A of one orientation: M for vxm, M' for mxv"""
        if orient == "vxm":
            return self.nrows, self.ncols, self.ptr, self.ind, vals
        tptr, tind, perm = self.transposed()
        return self.ncols, self.nrows, tptr, tind, vals[perm]


# ---- the route model -------------------------------------------------------------------------------------------------
def routes(case):
    """push_degree_kernel (degrees, scan, tile sums), push_partition_kernel (chunk_owner[c] = the LAST frontier entry
    whose scan value is <= min(c * EDGE_CHUNK, total - 1); find_owner's two levels find the same entry as one search
    over the global scan) and the count = k1 - k0 + 1 of lb_expand_kernel, with the facts the cases are built for"""
    nf, total = case.nf, case.total
    ntiles = -(-nf // DEG_TILE)
    tile_sums = np.add.reduceat(case.deg, np.arange(0, nf, DEG_TILE))
    nchunks = -(-total // EDGE_CHUNK)
    nwords = -(-case.ncols // 32)
    r = dict(nf=nf, total=total, scan_tiles=ntiles, chunks=nchunks, total_mod=total % EDGE_CHUNK,
             zero_tile=bool(np.any(tile_sums == 0)), word_tiles=-(-nwords // WORD_TILE),
             past_grid=nchunks > MAX_GRID, scan_carry=ntiles > SCAN_BLOCK,
             word_carry=-(-nwords // WORD_TILE) > SCAN_BLOCK, last_word_bits=case.ncols - 32 * (nwords - 1))
    if total == 0:
        r.update(unstaged=0, single_row=0, tile_edge_staged=0, count=np.zeros(0, dtype=np.int64),
                 chunk_owner=np.zeros(0, dtype=np.int64))
        return r
    e = np.minimum(np.arange(nchunks + 1, dtype=np.int64) * EDGE_CHUNK, total - 1)
    chunk_owner = np.searchsorted(case.scan, e, side="right") - 1
    assert np.all(case.deg[chunk_owner] > 0)                    # an owner owns: never an empty row among equal scans
    count = chunk_owner[1:] - chunk_owner[:-1] + 1
    first = case.owner[np.arange(nchunks) * EDGE_CHUNK]
    last = case.owner[np.minimum(np.arange(1, nchunks + 1) * EDGE_CHUNK, total) - 1]
    assert np.array_equal(first, chunk_owner[:-1]) and np.all(last <= chunk_owner[1:])   # [k0, k1] is a superset
    k0, k1 = chunk_owner[:-1], chunk_owner[1:]
    edge = (k1 // DEG_TILE > k0 // DEG_TILE) & (count <= SEG_MAX)      # a staged range over a scan-tile boundary
    r.update(unstaged=int(np.count_nonzero(count > SEG_MAX)), single_row=int(np.count_nonzero(first == last)),
             tile_edge_staged=int(np.count_nonzero(edge)), count=count, chunk_owner=chunk_owner)
    return r


# ---- the patterns ----------------------------------------------------------------------------------------------------
def _assemble(name, nrows, ncols, frontier_rows, fidx, rng, other_deg=4):
    """rows of the frontier as given (in frontier order), every other row a few random columns"""
    rows = [None] * nrows
    for r, cols in zip(fidx, frontier_rows):
        rows[r] = np.sort(np.asarray(cols, dtype=np.int64))
    for r in range(nrows):
        if rows[r] is None:
            rows[r] = np.sort(rng.choice(ncols, int(rng.integers(0, other_deg + 1)), replace=False))
    ptr = np.zeros(nrows + 1, dtype=np.int64)
    np.cumsum([c.size for c in rows], out=ptr[1:])
    return Case(name, nrows, ncols, ptr, np.concatenate(rows), fidx)


@functools.lru_cache(maxsize=None)
def small():
    rng = np.random.default_rng(31001)
    n = 1000
    lens = rng.integers(5, 12, n)
    lens[::97] = 0
    ind = np.concatenate([np.sort(rng.choice(n, k, replace=False)) for k in lens])
    fidx = np.sort(rng.choice(n, 37, replace=False))
    fidx[5] = 97 if 97 not in fidx else fidx[5]                 # an empty row in the frontier
    c = Case("S", n, n, np.concatenate([[0], np.cumsum(lens)]), ind, np.unique(fidx))
    f = routes(c)
    assert f["scan_tiles"] == 1 and f["chunks"] == 1 and f["word_tiles"] == 1 and f["unstaged"] == 0
    assert 7000 <= c.nvals <= 9000 and 0 < c.total < EDGE_CHUNK
    return c


def chunk_edges(variant):
    """E0 / E1.  Degrees in frontier order (position: what; edges before it):

         0 ..    9   empty                                               0
        10 ..  265   256 rows of 8: the total is 2048 at a row boundary  0 .. 2048
       266 .. 1265   500 rows of 2 and 500 of 1, mixed; position 1024,   2048 .. 3548
                     a scan-tile boundary, lies inside chunk 1 (staged)
      1266           hub of 5000 from the middle of chunk 1: chunks 2    3548 .. 8548
                     and 3 are its alone
      1267 .. 2112   846 rows of 2: up to the chunk boundary at 10240    8548 .. 10240
      2113           hub of exactly 2048: chunk 5 and nothing else       10240 .. 12288
      2114           a row of 3                                          12288 .. 12291
      2115 .. 4714   2600 empty rows: positions 3072 .. 4095 are a scan
                     tile of sum 0, and chunk 6's range is 2602 long or
                     more: the search per edge
      4715 .. 4969   255 rows of 8, then one row of 5 (E0) or of 5 and   12291 .. 14336 (E0), 14337 (E1)
                     one more row of 1 (E1): the total is 7 * 2048 (+ 1)
      then           20 empty rows
    """
    rng = np.random.default_rng(31002)
    nrows, ncols = 6000, 20011
    short = rng.permutation(np.repeat([2, 1], 500))
    deg = np.concatenate([np.zeros(10), np.full(256, 8), short, [5000], np.full(846, 2), [2048], [3], np.zeros(2600),
                          np.full(255, 8), [5], [1] * variant, np.zeros(20)]).astype(np.int64)
    fidx = np.sort(rng.choice(nrows, deg.size, replace=False))
    frontier_rows = []
    for k, d in enumerate(deg):
        if d > 100:
            cols = rng.choice(ncols, d, replace=False)
        else:                                                   # short rows: half of them crowd the first 1500 outputs
            cols = rng.choice(1500 if k % 2 else ncols, d, replace=False)
        frontier_rows.append(cols)
    frontier_rows[10] = np.array([0, 1, 31, 32, 33, 8191, 8192, ncols - 1])     # first / last word, a bitmap tile's edge
    c = _assemble("E%d" % variant, nrows, ncols, frontier_rows, fidx, rng)
    f = routes(c)
    assert np.array_equal(c.deg, deg)
    assert c.scan[266] == EDGE_CHUNK and c.deg[265] > 0         # 2048 at a row boundary
    assert c.scan[1266] == 3548 and c.deg[1266] == 5000 and f["single_row"] >= 3     # chunks 2, 3 and 5
    assert np.array_equal(f["chunk_owner"][2:5], [1266, 1266, 1266])
    assert c.scan[2113] == 5 * EDGE_CHUNK and c.deg[2113] == EDGE_CHUNK and f["count"][5] == 2
    assert f["count"][6] > SEG_MAX and f["unstaged"] == 1 and f["zero_tile"]
    assert f["count"][1] <= SEG_MAX and f["chunk_owner"][1] < DEG_TILE <= f["chunk_owner"][2]
    assert f["tile_edge_staged"] >= 1 and f["scan_tiles"] >= 5 and f["word_tiles"] == 3 and ncols % 32
    assert c.deg[0] == 0 and c.deg[-1] == 0
    assert f["total_mod"] == variant and f["chunks"] == 7 + variant
    return c


@functools.lru_cache(maxsize=None)
def chunk_edges_0():
    return chunk_edges(0)


@functools.lru_cache(maxsize=None)
def chunk_edges_1():
    return chunk_edges(1)


@functools.lru_cache(maxsize=None)
def many_scan_tiles():
    rng = np.random.default_rng(31003)
    nrows, ncols, nf = 300100, 50021, 300000
    lens = rng.integers(0, 4, nrows)
    fidx = np.sort(rng.choice(nrows, nf, replace=False))
    # stretches of empty frontier rows: whole scan tiles of sum 0 before and after the carry at tile 256
    for a, b in ((5000, 9000), (100000, 103000), (270000, 273500)):
        lens[fidx[a:b]] = 0
    ptr = np.concatenate([[0], np.cumsum(lens)])
    ind = rng.integers(0, ncols, int(ptr[-1]))
    # columns ascending and distinct inside a row: sort by (row, column), then spread the few duplicates
    rows = np.repeat(np.arange(nrows, dtype=np.int64), lens)
    order = np.lexsort((ind, rows))
    ind = ind[order]
    dup = np.nonzero((np.diff(ind) <= 0) & (np.diff(rows) == 0))[0] + 1
    while dup.size:                                             # at most 3 to a row: a step or two
        ind[dup] = ind[dup - 1] + 1
        dup = np.nonzero((np.diff(ind) <= 0) & (np.diff(rows) == 0))[0] + 1
    assert ind.max() < ncols
    c = Case("T", nrows, ncols, ptr, ind, fidx)
    f = routes(c)
    assert nf >= 300000 and f["scan_tiles"] > SCAN_BLOCK and f["scan_carry"] and f["zero_tile"]
    sums = np.add.reduceat(c.deg, np.arange(0, nf, DEG_TILE))
    assert np.any(sums[:SCAN_BLOCK] == 0) and np.any(sums[SCAN_BLOCK:] == 0)
    assert sums[SCAN_BLOCK - 1] > 0 and sums[SCAN_BLOCK] > 0 and sums[-1] > 0       # work on both sides of the carry
    assert f["unstaged"] >= 1 and c.deg.max() == 3 and f["chunks"] > 150 and not f["past_grid"]
    return c


@functools.lru_cache(maxsize=None)
def many_bitmap_tiles():
    rng = np.random.default_rng(31004)
    nrows, ncols, nf = 3000, 2200001, 2000
    fidx = np.sort(rng.choice(nrows, nf, replace=False))
    frontier_rows = [rng.choice(ncols, int(rng.integers(25, 36)), replace=False) for _ in range(nf)]
    step = SCAN_BLOCK * WORD_TILE * 32                          # outputs before the scan's carry: 2 097 152
    frontier_rows[0] = np.array([0, 31, 32, step - 33, step - 32, step - 1, step, step + 31, step + 32, ncols - 1])
    frontier_rows[nf - 1] = np.array([0, step - 1, step, ncols - 1, ncols - 2])
    c = _assemble("B", nrows, ncols, frontier_rows, fidx, rng)
    f = routes(c)
    assert f["word_tiles"] > SCAN_BLOCK and f["word_carry"] and f["last_word_bits"] == 1
    assert all(c.col_count[x] >= 2 for x in (0, step - 1, step, ncols - 1))
    tiles_hit = np.unique(np.nonzero(c.col_count)[0] // (WORD_TILE * 32))
    assert tiles_hit[0] == 0 and tiles_hit[-1] == f["word_tiles"] - 1 and tiles_hit.size > SCAN_BLOCK
    assert 50000 <= c.total <= 70000 and f["scan_tiles"] == 2
    return c


@functools.lru_cache(maxsize=None)
def dense():
    n = 2100
    c = Case("D", n, n, np.arange(n + 1, dtype=np.int64) * n, np.tile(np.arange(n, dtype=np.int32), n), np.arange(n))
    f = routes(c)
    assert c.total == 4410000 and f["chunks"] > MAX_GRID and f["past_grid"] and f["unstaged"] == 0
    assert n > EDGE_CHUNK                                       # every row crosses a chunk boundary
    assert np.all(c.scan // EDGE_CHUNK < (c.scan + n - 1) // EDGE_CHUNK)
    return c


def _tiny(name, fidx):
    """40 x 70: row 3 has one entry, rows 5, 6, 7, 20 are empty, the rest have a few"""
    rng = np.random.default_rng(31005)
    rows = [np.sort(rng.choice(70, int(rng.integers(1, 5)), replace=False)) for _ in range(40)]
    rows[3] = np.array([69])
    for r in (5, 6, 7, 20):
        rows[r] = np.zeros(0, dtype=np.int64)
    ptr = np.concatenate([[0], np.cumsum([r.size for r in rows])])
    return Case(name, 40, 70, ptr, np.concatenate(rows), fidx)


@functools.lru_cache(maxsize=None)
def one_entry():
    c = _tiny("Z1", [3])
    assert c.nf == 1 and c.total == 1
    return c


@functools.lru_cache(maxsize=None)
def one_empty_row():
    c = _tiny("Z0", [20])
    assert c.nf == 1 and c.total == 0
    return c


@functools.lru_cache(maxsize=None)
def only_empty_rows():
    c = _tiny("Zn", [5, 6, 7, 20])
    assert c.nf == 4 and c.total == 0
    return c


CASES = {"S": small, "E0": chunk_edges_0, "E1": chunk_edges_1, "T": many_scan_tiles, "B": many_bitmap_tiles,
         "D": dense, "Z1": one_entry, "Z0": one_empty_row, "Zn": only_empty_rows}
ORACLE_CASES = ["S", "E0", "E1", "Z1", "Z0", "Zn"]              # small enough for the oracle's sequential folds


# ---- operands --------------------------------------------------------------------------------------------------------
def _seed(*what):
    """a seed from names and flags that does not change between runs (hash() of a string does)"""
    return sum((i + 1) * sum(str(w).encode()) for i, w in enumerate(what)) % (1 << 31)


def _draw(case, sr_name, dtype, attempt):
    sr = Semiring(sr_name, dtype)
    ident = sr.identity()
    rng = np.random.default_rng(_seed(case.name, sr_name, np.dtype(dtype).name, attempt))
    nv, nf = case.nvals, case.nf
    if sr_name == "MultipliesMultiplies":
        # mostly the identity 1, and 1 on either side short-circuits to 1 (2 x 1 is 1 here): an output moves only
        # where a 2 or a 0 meets a 2 or a 0.  About two such 2 x 2 to the fullest output; a few 0, which is NOT the
        # identity and survives
        most = max(int(case.col_count.max()), 1)
        p2 = min(0.3, (2.0 / most) ** 0.5)
        vals = np.where(rng.random(nv) < p2, 2, 1)
        vals[rng.random(nv) < min(0.02, 0.3 / (most * p2))] = 0
        fval = np.where(rng.random(nf) < p2, 2, 1)
        if most < 1000:                                         # a 0 in D's frontier would zero every output
            fval[rng.random(nf) < 0.02] = 0
        fval[0] = 2
    elif sr_name == "PlusDivides":
        vals = rng.integers(-4, 5, nv)                          # 0 is the identity: short-circuit, no 0 / x
        fval = 1 << rng.integers(0, 4, nf)                      # 1, 2, 4, 8: dyadic quotients
        fval[rng.random(nf) < 0.1] = 0                          # the identity: short-circuit, no division by zero
    elif sr.monoid.opname in ("minimum", "maximum"):
        # nothing accumulates: a wide range, so that the extreme of D's 2100 entries to an output differs from output
        # to output and a lost combine shows (sums and products stay below 2^21)
        vals = rng.integers(-1000, 1001, nv)
        fval = rng.integers(-1000, 1001, nf)
    else:
        vals = rng.integers(-3, 5, nv)
        fval = rng.integers(-3, 6, nf)
    vals, fval = vals.astype(dtype), fval.astype(dtype)
    # the identity itself on both sides, whatever it is (0, 1, FLT_MAX, INT_MAX)
    vals[rng.random(nv) < 0.04] = ident
    fval[rng.random(nf) < 0.04] = ident
    if nv:
        vals[0] = vals[-1] = ident
    return vals, fval


def operands(case, sr_name, dtype):
    """(matrix values in M's CSR order, frontier values, dense mask, (sparse mask indices, values)), the first two in
    `dtype`, the masks as integers; redrawn until every partial result is exact (MultipliesMultiplies: bounded 2s)"""
    return prepared(case, sr_name, dtype)[0]


def prepared(case, sr_name, dtype):
    """(operands(), what fold() returns for them): the fold that proved them exact, for many epilogues"""
    rng = np.random.default_rng(_seed(case.name, "masks"))
    n = case.ncols
    mask = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 4, n) * rng.choice([-1, 1], n))
    sm_idx = np.nonzero(rng.random(n) < 0.3)[0].astype(np.int32)
    if sm_idx.size == 0:
        sm_idx = np.array([0], dtype=np.int32)
    sm_val = np.where(rng.random(sm_idx.size) < 0.3, 0, 1)
    for attempt in range(20):
        vals, fval = _draw(case, sr_name, dtype, attempt)
        try:
            folded = fold(case, sr_name, dtype, vals, fval)
            return (vals, fval, mask, (sm_idx, sm_val)), folded
        except AssertionError:
            if sr_name != "MultipliesMultiplies":
                raise
    raise AssertionError("no exact MultipliesMultiplies operands for " + case.name)


# ---- reference -------------------------------------------------------------------------------------------------------
_FOLD = {"plus": np.add, "multiplies": np.multiply, "minimum": np.minimum, "maximum": np.maximum}


def fold(case, sr_name, dtype, vals, fval):
    """(touched, reduced): which outputs the frontier reaches, and identity (+) every product of an output, folded in
    float64 / int64 and cast to `dtype`.  The products are mul_op(A value, u value) of oracle.semiring in the type
    itself, with the short-circuit of the reference's kernels/ewisemult.hpp:22-25: an operand equal to the identity
    gives the identity.  Asserts that every partial result in any order is exact in float32 and in int32."""
    sr = Semiring(sr_name, dtype)
    vals, fval = np.asarray(vals), np.asarray(fval)
    assert vals.dtype == dtype and fval.dtype == dtype and vals.size == case.nvals and fval.size == case.nf
    wide_t = np.float64 if np.issubdtype(np.dtype(dtype), np.floating) else np.int64
    ident = sr.identity()
    name = sr.monoid.opname
    n = case.ncols
    if case.full:                                               # D: a dense product, column by column
        a = vals.reshape(case.nrows, n)[case.fidx]
        x = np.broadcast_to(fval[:, None], a.shape)
        prod = np.where((a == ident) | (x == ident), ident, sr.mul_op(a, x)).astype(wide_t)
        touched = np.ones(n, dtype=bool)
        if name == "logical_or":
            red = ((prod != 0).any(axis=0) | bool(ident != 0)).astype(wide_t)
        else:
            red = _FOLD[name](wide_t(ident), _FOLD[name].reduce(prod, axis=0))
        mag = np.abs(prod).astype(np.float64)
        bound = mag.sum(axis=0) if name == "plus" else np.maximum(mag, 1).prod(axis=0) if name == "multiplies" else 0
    else:
        a, x = vals[case.epos], fval[case.owner]
        prod = np.where((a == ident) | (x == ident), ident, sr.mul_op(a, x)).astype(wide_t)
        touched = case.col_count > 0
        if name == "logical_or":
            red = ((np.bincount(case.dest, weights=(prod != 0), minlength=n) > 0) | bool(ident != 0)).astype(wide_t)
        else:
            red = np.full(n, ident, dtype=wide_t)
            _FOLD[name].at(red, case.dest, prod)
        mag = np.abs(prod)
        if name == "plus":
            bound = np.bincount(case.dest, weights=mag, minlength=n)
        elif name == "multiplies":
            bound = np.ones(n)
            np.multiply.at(bound, case.dest, np.maximum(mag, 1).astype(np.float64))
        else:
            bound = 0
    # plus / multiplies: every partial result in any order stays below 2^24 in magnitude and is a multiple of 1/8:
    # exact in float32, no overflow in int32.  minimum / maximum / or never round: every product is a value of `dtype`
    assert np.all(np.asarray(bound) < EXACT), (case.name, sr_name, float(np.max(bound)))
    if name in ("plus", "multiplies"):
        assert np.all(prod * 8 == np.round(prod * 8)) and np.all(np.abs(prod) < EXACT)
    out = red.astype(dtype)
    assert np.array_equal(out.astype(wide_t), red)
    return touched, out


def want(case, orient, sr_name, dtype, vals, fidx, fval, mask_kind="none", mask=None, scmp=0, struconly=0, folded=None):
    """(indices, values) of w = u M: ascending unique indices; values None for a structure-only product.  Both
    orientations are this same product (`orient` says which call is meant and is only checked).  The epilogue of the
    reference's spmspv.hpp:199-243 (oracle/ops.py:_spmspv_merge): a dense mask filters (scmp: where it is zero), a
    sparse mask filters nothing, any mask in key-value mode prunes the reduced values equal to 0.  `folded`: what
    fold() returned for these operands, to fold once for many epilogues."""
    assert orient in ORIENTS and mask_kind in ("none", "dense", "sparse")
    assert np.array_equal(fidx, case.fidx)
    touched, red = fold(case, sr_name, dtype, vals, fval) if folded is None else folded
    keys = np.nonzero(touched)[0]
    if mask_kind == "dense":
        m = np.asarray(mask)[keys]
        keys = keys[(m == 0) if scmp else (m != 0)]
    if struconly:
        return keys.astype(np.int32), None
    out = red[keys]
    if mask_kind != "none":
        keys, out = keys[out != 0], out[out != 0]
    return keys.astype(np.int32), out
