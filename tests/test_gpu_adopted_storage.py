"""GPU suite (-m gpu): vector operations, products, BFS and CDLP on storage the caller owns, at every 4-byte alignment.

grb_vector_adopt_dense / grb_vector_adopt_sparse / grb_matrix_adopt_device_csr, grb_k_spmv and grb_spmm take device
pointers as they are.  Several kernels choose between 16-byte and 4-byte accesses by looking at the pointer (reduce_kernel,
assign_dense_mask_dense_kernel, k_copy, the label pass of the one-launch BFS, cd_stream of cdlp.hip); a fresh allocation
is 256-byte aligned, so only the wide side of each ever ran under test.  carve() below places the payload 4 * k bytes
(k = 0 .. 3) past a 16-byte boundary inside a larger tensor filled with a sentinel; every test asserts the pointer's
residue (which side of the predicate it takes) and, for everything the library writes through such a pointer, that the
sentinel on both sides is untouched.  Expected values come from the oracle (oracle/ops.py, oracle/semiring.py,
oracle/simple_reference.py, the numpy CDLP of test_gpu_cdlp.py), never from the library's own aligned run; the k = 0 run
is compared in addition where it costs nothing.  All data is integer-valued, so every order of summation agrees."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_gpu_cdlp as cd
from backends import HipBackend, OracleBackend

pytestmark = pytest.mark.gpu

F, I = np.float32, np.int32
KS = (0, 1, 2, 3)
SENTINEL = int(np.array([0xFFA5A5A5], np.uint32).view(np.int32)[0])   # as f32: a NaN; occurs in no test's data
MONOIDS = ["Plus", "Multiplies", "Minimum", "Maximum", "LogicalOr", "LogicalAnd"]
G_LANES = 2048 * 256                                   # lanes of the capped grid of reduce_kernel (stream_grid: 2048 workgroups)


@pytest.fixture(scope="module")
def hb():
    return HipBackend()


@pytest.fixture(scope="module")
def ob():
    return OracleBackend()


# ---- the helper --------------------------------------------------------------------------------------------------------
def carve(values, k, guard=8):
    """-> (pointer to the payload, the tensor that owns it, check()): values (f32 or i32, any shape, row-major) copied to
    element guard + k of a sentinel-filled tensor whose base is 16-byte aligned, so the payload is 4 * k bytes past a
    16-byte boundary; check(what) asserts that everything around the payload still holds the sentinel, bit for bit"""
    assert guard % 4 == 0 and k in KS
    raw = np.ascontiguousarray(values).reshape(-1)
    assert raw.dtype in (np.dtype(F), np.dtype(I)), raw.dtype
    bits = raw.view(I).copy()
    assert not np.any(bits == SENTINEL)
    n, lo = bits.size, guard + k
    t = torch.full((lo + n + guard,), SENTINEL, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 16 == 0
    if n:
        t[lo:lo + n] = torch.from_numpy(bits).to("cuda")
    torch.cuda.synchronize()
    ptr = t.data_ptr() + 4 * lo
    assert ptr % 16 == (4 * k) % 16

    def check(what=""):
        torch.cuda.synchronize()                        # every stream of the device, the library's included
        head, tail = t[:lo].cpu().numpy(), t[lo + n:].cpu().numpy()
        assert head.size == lo and tail.size == guard
        assert np.all(head == SENTINEL), ("bytes before the payload changed", what, k, np.flatnonzero(head != SENTINEL) - lo)
        assert np.all(tail == SENTINEL), ("bytes behind the payload changed", what, k, np.flatnonzero(tail != SENTINEL))

    return ptr, t, check


def payload(t, k, n, dtype, guard=8):
    """the n payload elements of a carved tensor, as the caller sees them"""
    torch.cuda.synchronize()
    return t[guard + k:guard + k + n].cpu().numpy().view(dtype)


def adopt_dense(g, values, k):
    """-> (Vector over the carved values, tensor, check)"""
    values = np.ascontiguousarray(values)
    ptr, t, check = carve(values, k)
    v = g.Vector(values.size, values.dtype.type)
    assert v.build_device(ptr, values.size) == 0
    v._keep = [t]
    return v, t, check


def adopt_sparse(g, nsize, idx, vals, ki, kv):
    idx, vals = np.ascontiguousarray(idx, I), np.ascontiguousarray(vals)
    pi, ti, ci = carve(idx, ki)
    pv, tv, cv = carve(vals, kv)
    v = g.Vector(nsize, vals.dtype.type)
    assert v.build_device(pv, idx.size, pi) == 0
    v._keep = [ti, tv]
    return v, (ci, cv)


def adopt_csr(g, shape, dt, ptr, ind, val, ks, csc=None, kcs=None):
    """-> (Matrix over carved ptr / ind / val (and the CSC arrays), the checks)"""
    A = g.Matrix(shape[0], shape[1], dt)
    parts = [carve(np.asarray(a, d), k) for a, d, k in zip((ptr, ind, val), (I, I, dt), ks)]
    if csc is not None:
        parts += [carve(np.asarray(a, d), k) for a, d, k in zip(csc, (I, I, dt), kcs)]
    assert (parts[1][0] % 16, parts[2][0] % 16) == (4 * ks[1], 4 * ks[2])
    args = [p[0] for p in parts[:3]] + [int(np.asarray(ind).size)] + [p[0] for p in parts[3:]]
    assert A.build_device_csr(*args, keep=[p[1] for p in parts]) == 0
    return A, [p[2] for p in parts]


def fold(mon, arr):
    """the oracle's monoid over arr by halving (its operator on whole arrays: exact data, every order agrees)"""
    a = np.asarray(arr, mon.dtype)
    if a.size == 0:
        return mon.identity()
    while a.size > 1:
        h = a.size // 2
        b = mon.op(a[:h], a[h:2 * h])
        a = np.concatenate([b, a[2 * h:]]) if a.size & 1 else b
    return mon.dtype(mon.op(mon.identity(), a[0])[()])


def reduce_data(monoid, dt, n, rng):
    if monoid == "Plus":
        return rng.integers(1, 3, n).astype(dt)                 # a dropped or doubled element changes the sum
    if monoid == "Multiplies":
        a = np.ones(n, dt)
        a[rng.choice(n, min(20, n), replace=False)] = 2
        return a
    if monoid in ("Minimum", "Maximum"):
        return rng.integers(-5, 6, n).astype(dt)
    return rng.integers(0, 2, n).astype(dt)


def planted_positions(n):
    return sorted({p for p in (0, 1, 2, 3, 4 * (n // 4) - 1, 4 * (n // 4), n - 1) if 0 <= p < n})


def row_ptr(n, rows):
    return np.linspace(0, n, rows + 1).astype(I)


# ---- reductions --------------------------------------------------------------------------------------------------------
SMALL_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 1023, 1024, 1025, 1027, 2049]
LARGE_LENGTHS = [4 * G_LANES + 42, 8 * G_LANES + 3, 8 * G_LANES + 4000 + 1, 12 * G_LANES + 5]


def hip_reduce_all(hb, monoid, vals, k, desc, what):
    """the three routes to k_reduce on vals carved at k: dense vector, sparse vector (indices carved elsewhere), matrix"""
    g = hb.g
    n = vals.size
    out = {}
    v, _, _ = adopt_dense(g, vals, k)
    info, out["dense"] = g.reduce(None, monoid, v, desc)
    assert info == 0, (what, "dense")
    s, _ = adopt_sparse(g, n + 3, np.arange(n), vals, (k + 1) % 4, k)
    assert s.getStorage() == g.GrB_SPARSE and s.nvals() == n
    info, out["sparse"] = g.reduce(None, monoid, s, desc)
    assert info == 0, (what, "sparse")
    rows = min(n, 5)
    A, _ = adopt_csr(g, (rows, n), vals.dtype.type, row_ptr(n, rows), np.arange(n), vals, ((k + 2) % 4, (k + 3) % 4, k))
    info, out["matrix"] = g.reduce_matrix(None, monoid, A, desc)
    assert info == 0, (what, "matrix")
    return out


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("monoid", MONOIDS)
def test_reduce_small_lengths(hb, ob, monoid, dt):
    """every length around the quad and the workgroup, every offset; the tree fold used for the expectations equals the
    oracle's sequential reduce_vector at every length"""
    rng = np.random.default_rng(21)
    mon = ob.Monoid(monoid, dt)
    desc, odesc = hb.descriptor(), ob.descriptor()
    for n in SMALL_LENGTHS:
        base = reduce_data(monoid, dt, n, rng)
        variants = [("base", base)]
        if monoid in ("Minimum", "Maximum"):
            for p in planted_positions(n):
                x = base.copy()
                x[p] = -9 if monoid == "Minimum" else 9    # the unique extreme
                variants.append(("extreme at %d" % p, x))
        if monoid == "LogicalOr":
            for p in planted_positions(n):
                x = np.zeros(n, dt)
                x[p] = 1                                    # the only true element
                variants.append(("only %d true" % p, x))
            variants.append(("all false", np.zeros(n, dt)))
        if monoid == "LogicalAnd":
            variants.append(("all true", np.ones(n, dt)))
        for name, x in variants:
            want = fold(mon, x)
            if name == "base" or n <= 8:
                ov = ob.vector(n, dt)
                ob.build_dense(ov, x)
                assert ob.reduce(monoid, ov, odesc)[1] == want, (monoid, dt, n, name)
            first = None
            for k in KS:
                got = hip_reduce_all(hb, monoid, x, k, desc, (monoid, dt.__name__, n, name, k))
                for route, val in got.items():
                    assert dt(val) == want, (monoid, dt.__name__, n, name, "k", k, route, val, want)
                first = got if first is None else first
                assert got == first, (monoid, dt.__name__, n, name, k, got, first)


@pytest.fixture(scope="module")
def big_buffers():
    """one device buffer per element type for the four lengths that reach the capped grid: [guard | Lmax + 1 values | guard],
    refilled per data kind; the (length n, offset k) case reads values[k : k + n]"""
    guard, room = 8, max(LARGE_LENGTHS) + 1
    out = {}
    for dt in (F, I):
        t = torch.full((guard + room + guard,), SENTINEL, dtype=torch.int32, device="cuda")
        assert t.data_ptr() % 16 == 0
        out[dt] = t
    cols = torch.arange(room, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return guard, room, out, cols


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("monoid", MONOIDS)
def test_reduce_capped_grid(hb, ob, big_buffers, monoid, dt):
    """n > 2 Mi: the grid is capped at 2048 workgroups, so the two-loads-in-flight loop, its single-fold remainder and the
    n % 4 tail run -- on the wide side at k = 0 and the element-per-lane side at k = 1"""
    g = hb.g
    guard, room, bufs, cols = big_buffers
    t = bufs[dt]
    rng = np.random.default_rng(22)
    H = reduce_data(monoid, dt, room, rng)
    assert not np.any(H.view(I) == SENTINEL)
    t[guard:guard + room] = torch.from_numpy(H.view(I).copy()).to("cuda")
    torch.cuda.synchronize()
    mon = ob.Monoid(monoid, dt)
    desc = hb.descriptor()
    ext = dt(-9 if monoid == "Minimum" else 9)
    for n in LARGE_LENGTHS:
        assert n > 2048 * 256 * 4 and n // 4 > G_LANES          # the grid is capped and some lane has a second quad
        for k in (0, 1):
            ptr = t.data_ptr() + 4 * (guard + k)
            assert ptr % 16 == 4 * k
            x = H[k:k + n]
            want = fold(mon, x)
            if monoid == "Plus":
                assert want == x.astype(np.int64).sum() < 2 ** 24
            v = g.Vector(n, dt)
            assert v.build_device(ptr, n) == 0
            info, val = g.reduce(None, monoid, v, desc)
            assert info == 0 and dt(val) == want, (monoid, dt.__name__, n, k, "dense", val, want)
            s = g.Vector(n, dt)
            assert s.build_device(ptr, n, cols.data_ptr() + 4 * k) == 0
            info, val = g.reduce(None, monoid, s, desc)
            assert info == 0 and dt(val) == want, (monoid, dt.__name__, n, k, "sparse", val, want)
            A = g.Matrix(1024, room, dt)
            tp = torch.from_numpy(row_ptr(n, 1024)).to("cuda")
            torch.cuda.synchronize()
            assert A.build_device_csr(tp.data_ptr(), cols.data_ptr(), ptr, n, keep=(tp, cols, t)) == 0
            info, val = g.reduce_matrix(None, monoid, A, desc)
            assert info == 0 and dt(val) == want, (monoid, dt.__name__, n, k, "matrix", val, want)
            if monoid in ("Minimum", "Maximum"):
                for p in planted_positions(n):
                    y = x.copy()
                    y[p] = ext
                    t[guard + k + p] = int(np.array([ext], dt).view(I)[0])
                    torch.cuda.synchronize()
                    info, val = g.reduce(None, monoid, v, desc)
                    t[guard + k + p] = int(x[p:p + 1].view(I)[0])
                    assert info == 0 and dt(val) == fold(mon, y) == ext, (monoid, dt.__name__, n, k, "extreme at", p, val)
                torch.cuda.synchronize()
    assert np.array_equal(payload(t, 0, room, dt, guard), H)
    assert np.all(t[:guard].cpu().numpy() == SENTINEL) and np.all(t[guard + room:].cpu().numpy() == SENTINEL)


@pytest.mark.parametrize("dt", [F, I])
def test_reduce_struconly_and_empty(hb, ob, dt):
    g = hb.g
    rng = np.random.default_rng(23)
    sdesc, osdesc = hb.descriptor(struconly=1), ob.descriptor(struconly=True)
    desc, odesc = hb.descriptor(), ob.descriptor()
    for n in (1, 5, 1027):
        x = reduce_data("Plus", dt, n, rng)
        ov = ob.vector(n + 3, dt)
        ob.build_sparse(ov, np.arange(n), x)
        for k in KS:
            s, _ = adopt_sparse(g, n + 3, np.arange(n), x, k, (k + 1) % 4)
            info, val = g.reduce(None, "Plus", s, sdesc)
            assert info == 0 and val == n == ob.reduce("Plus", ov, osdesc)[1], (n, k, val)
            A, _ = adopt_csr(g, (1, n), dt, [0, n], np.arange(n), x, (k, k, (k + 1) % 4))
            info, val = g.reduce_matrix(None, "Plus", A, sdesc)
            assert info == 0 and val == n == ob.ops.reduce_matrix(ob.Monoid("Plus", dt), x, n, osdesc), (n, k, val)
    for monoid in MONOIDS:
        mon = ob.Monoid(monoid, dt)
        ov = ob.vector(7, dt)
        ob.build_sparse(ov, np.zeros(0, I), np.zeros(0, dt))
        want = ob.reduce(monoid, ov, odesc)[1]
        assert want == mon.identity() == ob.ops.reduce_matrix(mon, np.zeros(0, dt), 0, odesc)
        for k in KS:
            s, _ = adopt_sparse(g, 7, np.zeros(0, I), np.zeros(0, dt), k, (k + 1) % 4)
            info, val = g.reduce(None, monoid, s, desc)
            assert info == 0 and dt(val) == want, (monoid, dt.__name__, k, val, want)
            A, _ = adopt_csr(g, (3, 4), dt, [0, 0, 0, 0], np.zeros(0, I), np.zeros(0, dt), (k, (k + 1) % 4, (k + 2) % 4))
            info, val = g.reduce_matrix(None, monoid, A, desc)
            assert info == 0 and dt(val) == want, (monoid, dt.__name__, k, "matrix", val, want)


@pytest.mark.parametrize("dt", [F, I])
def test_convert_counts_on_carved_vectors(hb, ob, dt):
    """k_count_nonidentity, the counting form of reduce_kernel, through Vector::convert: the first call records the ratio of
    a full vector, the caller rewrites its tensor so that exactly c elements differ from the identity (the ends of the quads
    and the tail among them), and the second call turns the vector sparse if and only if c / n <= switchpoint -- with the
    switchpoint at c / n it must (one element counted twice would keep it dense), at (c - 1) / n it must not (one element
    dropped would convert it)"""
    g = hb.g
    rng = np.random.default_rng(36)
    desc, odesc = hb.descriptor(), ob.descriptor()
    cases = [(n, KS) for n in (5, 7, 8, 1023, 1024, 1025, 1027, 2049)] + [(n, (0, 1)) for n in (LARGE_LENGTHS[1], LARGE_LENGTHS[3])]
    for n, ks in cases:
        full = rng.integers(1, 9, n).astype(dt)
        c = max(1, n // 8)
        pos = np.array(planted_positions(n)[::-1][:c], np.int64)         # n - 1, 4 (n / 4), 4 (n / 4) - 1, 3, ... first
        others = np.setdiff1d(np.arange(n), pos)
        pos = np.concatenate([pos, rng.choice(others, c - pos.size, replace=False)])
        few = np.zeros(n, dt)
        few[pos] = rng.choice(np.array([-2, -1, 1, 2, 3], dt), c)
        assert np.count_nonzero(few) == c < n
        for exact in (True, False):
            sp = np.float32(c if exact else c - 1) / np.float32(n)
            ov = ob.vector(n, dt)
            ob.build_dense(ov, full)
            assert ov.convert(dt(0), sp, odesc) == 0 and ob.storage(ov) == ob.ops.GrB_DENSE
            ov.d_val[:] = few
            assert ov.convert(dt(0), sp, odesc) == 0
            assert ob.storage(ov) == (ob.ops.GrB_SPARSE if exact else ob.ops.GrB_DENSE)
            for k in ks:
                what = (dt.__name__, n, "c", c, "switchpoint at c" if exact else "switchpoint below c", "k", k)
                v, t, check = adopt_dense(g, full, k)
                assert v.convert(0, float(sp), desc) == 0 and hb.storage(v) == g.GrB_DENSE, what
                t[8 + k:8 + k + n] = torch.from_numpy(few.view(I).copy()).to("cuda")    # the caller's tensor: the caller may write it
                torch.cuda.synchronize()
                assert v.convert(0, float(sp), desc) == 0, what
                assert hb.storage(v) == ob.storage(ov) and hb.nvals(v) == ob.nvals(ov), (what, hb.storage(v), hb.nvals(v))
                if exact:
                    idx, vals = hb.sparse_tuples(v)
                    oidx, ovals = ob.sparse_tuples(ov)
                    assert np.array_equal(idx, oidx) and np.array_equal(vals, ovals), what
                check(what)


# ---- row reduction -----------------------------------------------------------------------------------------------------
ROW_LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 0, 0, 1000, 1]


@pytest.mark.parametrize("dt", [F, I])
@pytest.mark.parametrize("monoid", MONOIDS)
def test_reduce_rows_every_group_length(hb, ob, monoid, dt):
    """rows around the 16 lanes a row gets, empty rows (the identity) and a long one; a library-owned matrix, and an adopted
    one with val and the result vector carved at every offset"""
    g = hb.g
    rng = np.random.default_rng(24)
    ptr = np.concatenate([[0], np.cumsum(ROW_LENGTHS)]).astype(I)
    ind = np.concatenate([np.arange(m) for m in ROW_LENGTHS]).astype(I)
    nrows, ncols, nnz = len(ROW_LENGTHS), 1000, int(ptr[-1])
    val = reduce_data(monoid, dt, nnz, rng)
    if monoid == "Multiplies":
        val = np.where(ind % 53 == 0, 2, 1).astype(dt)                # 19 twos in the long row: 2^19 is exact
    if monoid in ("LogicalOr", "LogicalAnd"):
        val[ptr[2]:ptr[3]] = 0
        val[ptr[3]:ptr[4]] = 1
    OA = ob.ops.Matrix(nrows, ncols, dt)
    OA.build_csr(ptr, ind, val)
    ow = ob.vector(nrows, dt)
    assert ob.reduce_rows(ow, monoid, OA, ob.descriptor()) == 0
    want = ob.dense_values(ow)
    assert want[0] == want[8] == ob.Monoid(monoid, dt).identity()
    desc = hb.descriptor()
    A = g.Matrix(nrows, ncols, dt)
    assert A.build_csr(ptr, ind, val) == 0
    w = g.Vector(nrows, dt)
    assert hb.reduce_rows(w, monoid, A, desc) == 0
    assert np.array_equal(hb.dense_values(w), want), (monoid, dt.__name__, "owned")
    for kv in KS:
        for kw in KS:
            B, _ = adopt_csr(g, (nrows, ncols), dt, ptr, ind, val, ((kv + 1) % 4, (kv + 2) % 4, kv))
            w, t, check = adopt_dense(g, np.full(nrows, 77, dt), kw)
            assert hb.reduce_rows(w, monoid, B, desc) == 0
            got = hb.dense_values(w)
            assert np.array_equal(got, want), (monoid, dt.__name__, kv, kw, got, want)
            assert np.array_equal(payload(t, kw, nrows, dt), want)
            check(("reduce_rows", monoid, kv, kw))


# ---- masked constant assign --------------------------------------------------------------------------------------------
ASSIGN_LENGTHS = list(range(1, 10)) + [255, 256, 257] + list(range(1023, 1030)) + [4099]
ASSIGN_LARGE = 2097152 + 4 * 37 + 3
SPECIAL_MASK = np.array([0.0, -0.0, 1.0, -1.0, np.nan, np.inf, np.finfo(F).tiny, 1e-45], F)   # the last: the smallest denormal


def mask_patterns(n, dt, rng):
    """-> {name: mask}; true elements take several values (the sign bit alone among them for i32), false ones 0 / -0.0"""
    true = np.array([1, -1, 0.5, 3e38], F) if dt is F else np.array([1, -1, np.iinfo(I).min, 7], I)
    false = np.array([0.0, -0.0], F) if dt is F else np.array([0, 0], I)
    i = np.arange(n)
    shapes = {"all pass": np.ones(n, bool), "none pass": np.zeros(n, bool), "random half": rng.random(n) < 0.5,
              "one fails per quad": (i % 4) != ((i // 4) % 4), "one passes per quad": (i % 4) == ((i // 4) % 4)}
    return {name: np.where(on, true[i % 4], false[i % 2]).astype(dt) for name, on in shapes.items()}


def oracle_assign(ob, w0, mask, val, scmp):
    ow, om = ob.vector(w0.size, w0.dtype.type), ob.vector(mask.size, mask.dtype.type)
    ob.build_dense(ow, w0)
    ob.build_dense(om, mask)
    od = ob.descriptor()
    if scmp:
        ob.toggle(od, ob.ops.GrB_MASK)
    assert ob.assign(ow, om, val, od) == 0
    return ob.dense_values(ow)


def hip_assign_adopted(hb, w0, mask_carved, n, val, desc, kw, what):
    g = hb.g
    w, t, check = adopt_dense(g, w0, kw)
    m = g.Vector(n, mask_carved[2])
    assert m.build_device(mask_carved[0], n) == 0
    assert hb.assign(w, m, val, desc) == 0 and g.lazy_pending() == 0, what   # adopted: runs at once
    got = hb.dense_values(w)
    assert np.array_equal(payload(t, kw, n, w0.dtype.type), got), what
    check(what)
    return got


@pytest.mark.parametrize("scmp", [False, True])
@pytest.mark.parametrize("dt", [F, I])
def test_assign_every_offset_pair(hb, ob, dt, scmp):
    """w and the mask carved independently: the wide path only at (0, 0), the element path everywhere else, the n % 4 tail
    of the wide path at every residue; w's surroundings after every call"""
    g = hb.g
    rng = np.random.default_rng(25)
    desc = hb.descriptor()
    if scmp:
        hb.toggle(desc, g.GrB_MASK)
    val = -3
    cases = [(n, [(kw, km) for kw in KS for km in KS]) for n in ASSIGN_LENGTHS] + [(ASSIGN_LARGE, [(0, 0), (1, 0), (0, 3)])]
    for n, pairs in cases:
        w0 = (np.arange(n) % 97 + 2).astype(dt)
        masks = mask_patterns(n, dt, rng)
        masks["special values"] = np.resize(SPECIAL_MASK, n)            # an f32 mask, whatever w's type
        for name, mask in masks.items():
            want = oracle_assign(ob, w0, mask, val, scmp)
            assert np.array_equal(want, np.where((mask == 0) if scmp else (mask != 0), dt(val), w0))
            carved = {}
            for kw, km in pairs:
                if km not in carved:
                    p, t, _ = carve(mask, km)
                    carved[km] = (p, t, mask.dtype.type)
                what = ("assign", dt.__name__, "scmp", scmp, n, name, "k_w", kw, "k_m", km)
                got = hip_assign_adopted(hb, w0, carved[km], n, val, desc, kw, what)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]], mask[bad[:8]])


@pytest.mark.parametrize("scmp", [False, True])
@pytest.mark.parametrize("dt", [F, I])
def test_assign_three_implementations_agree_with_the_oracle(hb, ob, dt, scmp):
    """one mask through the 16-byte path (adopted, k = 0), the element path (adopted, k = 1) and the queued chain
    (library-owned w and mask, two steps pending, flushed by reading): all three equal the oracle, whose rule is numpy's
    `!= 0` -- so -0.0 fails and NaN, inf and denormals pass"""
    g = hb.g
    rng = np.random.default_rng(26)
    desc = hb.descriptor()
    if scmp:
        hb.toggle(desc, g.GrB_MASK)
    val = -3
    before = g.set_lazy(1)
    try:
        for n in (7, 1027, 4099):
            w0 = (np.arange(n) % 97 + 2).astype(dt)
            masks = mask_patterns(n, dt, rng)
            if dt is F:
                masks["special values"] = np.resize(SPECIAL_MASK, n)
            for name, mask in masks.items():
                want = oracle_assign(ob, w0, mask, val, scmp)
                got = {}
                for route, k in (("wide", 0), ("element", 1)):
                    p, t, _ = carve(mask, k)
                    got[route] = hip_assign_adopted(hb, w0, (p, t, dt), n, val, desc, k, (route, n, name))
                ws = [g.Vector(n, dt), g.Vector(n, dt)]
                m = g.Vector(n, dt)
                assert m.build(mask, n) == 0
                for w in ws:
                    assert w.build(w0, n) == 0
                for w in ws:
                    assert hb.assign(w, m, val, desc) == 0
                assert g.lazy_pending() == 2, (n, name)                  # both wait in the queue: they run as one program
                got["queued"] = hb.dense_values(ws[0])
                assert g.lazy_pending() == 0
                assert np.array_equal(hb.dense_values(ws[1]), got["queued"])
                for route, x in got.items():
                    bad = np.flatnonzero(x != want)
                    assert bad.size == 0, (route, dt.__name__, "scmp", scmp, n, name, bad[:8], x[bad[:8]], want[bad[:8]], mask[bad[:8]])
    finally:
        g.set_lazy(before)


# ---- copies ------------------------------------------------------------------------------------------------------------
COPY_LENGTHS = [1, 3, 4, 5, 1027, 4096]


@pytest.mark.parametrize("dt", [F, I])
def test_copies_between_carved_vectors(hb, ob, dt):
    """k_copy through dup, eWiseAdd (sparse, dense), eWiseAdd with a scalar and resize: 16-byte copies plus a tail only
    when source and destination are both aligned, byte counts that are and are not multiples of 16"""
    g = hb.g
    rng = np.random.default_rng(27)
    desc, odesc = hb.descriptor(), ob.descriptor()
    sr = "PlusMultiplies"
    for n in COPY_LENGTHS:
        src = rng.integers(1, 50, n).astype(dt)
        old = rng.integers(-50, 0, n).astype(dt)
        sidx = np.sort(rng.choice(n, (n + 1) // 2, replace=False)).astype(I)
        sval = rng.integers(1, 9, sidx.size).astype(dt)
        ou, ov, ow = ob.vector(n, dt), ob.vector(n, dt), ob.vector(n, dt)
        ob.build_sparse(ou, sidx, sval)
        ob.build_dense(ov, src)
        ob.build_dense(ow, old)
        assert ob.eWiseAdd(ow, None, None, sr, ou, ov, odesc) == 0
        want_add = ob.dense_values(ow)
        ow = ob.vector(n, dt)
        ob.build_dense(ow, old)
        assert ob.eWiseAdd(ow, None, None, sr, ov, 5, odesc) == 0
        want_scalar = ob.dense_values(ow)
        od = ob.vector(n, dt)
        assert od.dup(ov) == 0 and np.array_equal(ob.dense_values(od), src)
        for ks in KS:
            # an adopted source into a library-owned vector and back
            s, ts, cs = adopt_dense(g, src, ks)
            owned = g.Vector(n, dt)
            assert owned.dup(s) == 0 and np.array_equal(hb.dense_values(owned), src), ("dup to owned", n, ks)
            d, td, cdst = adopt_dense(g, old, ks)
            assert d.dup(owned) == 0 and np.array_equal(hb.dense_values(d), src), ("dup from owned", n, ks)
            assert np.array_equal(payload(td, ks, n, dt), src)
            cdst(("dup from owned", n, ks))
            for kd in KS:
                what = (dt.__name__, n, "k_src", ks, "k_dst", kd)
                d, td, cdst = adopt_dense(g, old, kd)
                assert d.dup(s) == 0, what
                assert np.array_equal(hb.dense_values(d), src) and np.array_equal(payload(td, kd, n, dt), src), ("dup",) + what
                cdst(("dup",) + what)
                # w = u (+) v, u sparse: v is copied into w, then the sparse entries are folded in
                w, tw, cw = adopt_dense(g, old, kd)
                u = g.Vector(n, dt)
                assert u.build(sidx, sval, sidx.size, None) == 0
                assert g.eWiseAdd(w, None, None, sr, u, s, desc) == 0, what
                got = hb.dense_values(w)
                assert np.array_equal(got, want_add) and np.array_equal(payload(tw, kd, n, dt), want_add), ("eWiseAdd",) + what + (got, want_add)
                cw(("eWiseAdd",) + what)
                # w = u (+) 5, u != w: u is copied into w first
                w, tw, cw = adopt_dense(g, old, kd)
                assert g.eWiseAdd(w, None, None, sr, s, 5, desc) == 0, what
                got = hb.dense_values(w)
                assert np.array_equal(got, want_scalar) and np.array_equal(payload(tw, kd, n, dt), want_scalar), ("scalar",) + what + (got, want_scalar)
                cw(("eWiseAdd scalar",) + what)
            # the sources were only read
            assert np.array_equal(payload(ts, ks, n, dt), src)
            cs(("source", n, ks))
            # resize: the result is the library's own storage, the caller's tensor keeps its bytes
            for size in sorted({n + 5, max(n - 2, 1)} - {n}):
                r, tr, cr = adopt_dense(g, src, ks)
                carved_ptr = tr.data_ptr() + 4 * (8 + ks)
                assert r.device_ptrs()[2] == carved_ptr
                orv = ob.vector(n, dt)
                ob.build_dense(orv, src)
                assert orv.resize(size) == 0 and r.resize(size) == 0
                assert r.size() == size and np.array_equal(hb.dense_values(r), ob.dense_values(orv)), ("resize", n, size, ks)
                assert r.device_ptrs()[2] != carved_ptr
                assert r.fill(123) == 0 and np.all(hb.dense_values(r) == 123)          # ... and writing it leaves the tensor alone
                assert np.array_equal(payload(tr, ks, n, dt), src)
                cr(("resize", n, size, ks))


# ---- products ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def product_graph():
    """777 vertices, random edges (not symmetric), row 5 with 300 entries, values 1 .. 3"""
    from graphblast_amd.graphgen import finalize_edges
    rng = np.random.default_rng(28)
    n, m = 777, 5000
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    src[:300] = 5
    dst[:300] = rng.permutation(n)[:300]
    gr = finalize_edges(src, dst, n, symmetrize=False)
    ptr, ind = (np.asarray(x, I) for x in gr["csr"])
    assert ptr[6] - ptr[5] >= 299
    val = rng.integers(1, 4, ind.size).astype(F)
    return n, ptr, ind, val


OFFSETS3 = [(a, b, c) for a in (0, 1, 3) for b in (0, 1, 3) for c in (0, 1, 3)]


def snapshot(b, w):
    """storage, stored count and values of a result (reading the values makes a sparse one dense: read last, once)"""
    return b.storage(w), b.nvals(w), b.dense_values(w)


def compare_snapshots(got, want, what):
    assert got[:2] == want[:2], (what, got[:2], want[:2])
    bad = np.flatnonzero(got[2] != want[2])
    assert bad.size == 0, (what, bad[:8], got[2][bad[:8]], want[2][bad[:8]])


@pytest.mark.parametrize("is_vxm", [False, True])
@pytest.mark.parametrize("sr", ["PlusMultiplies", "MinimumPlus", "LogicalOrAnd"])
def test_mxv_vxm_on_carved_operands(hb, ob, product_graph, sr, is_vxm):
    g = hb.g
    n, ptr, ind, val = product_graph
    rng = np.random.default_rng(29)
    A = hb.matrix_from_csr(n, ptr, ind, val)
    OA = ob.matrix_from_csr(n, ptr, ind, val)
    u_dense = rng.integers(0, 4, n).astype(F)
    u_idx = np.sort(rng.choice(n, n // 3, replace=False)).astype(I)
    u_val = rng.integers(1, 4, u_idx.size).astype(F)
    mask = (rng.random(n) < 0.5).astype(F)
    w0 = rng.integers(10, 20, n).astype(F)

    def call(b, *a):
        return b.vxm(a[0], a[1], None, sr, a[3], a[2], a[4]) if is_vxm else b.mxv(a[0], a[1], None, sr, a[2], a[3], a[4])

    for mode in (1, 2):                                                 # push only, pull only
        for u_sparse in (False, True):
            for masked, scmp in ((False, False), (True, False), (True, True)):
                od = ob.descriptor(mxvmode=mode)
                if scmp:
                    ob.toggle(od, ob.ops.GrB_MASK)
                ou, ow, om = ob.vector(n, F), ob.vector(n, F), ob.vector(n, F)
                ob.build_sparse(ou, u_idx, u_val) if u_sparse else ob.build_dense(ou, u_dense)
                ob.build_dense(ow, w0)
                ob.build_dense(om, mask)
                want_info = call(ob, ow, om if masked else None, OA, ou, od)
                want = snapshot(ob, ow)
                for ku, kw, km in OFFSETS3:
                    if not masked and km:
                        continue                                        # no mask: its offset does not matter
                    what = (sr, "vxm" if is_vxm else "mxv", "mode", mode, "sparse u", u_sparse, "mask", masked, scmp, "k", ku, kw, km)
                    d = hb.descriptor(mxvmode=mode)
                    if scmp:
                        hb.toggle(d, g.GrB_MASK)
                    if u_sparse:
                        u, _ = adopt_sparse(g, n, u_idx, u_val, ku, (ku + 1) % 4)
                    else:
                        u, _, _ = adopt_dense(g, u_dense, ku)
                    w, tw, cw = adopt_dense(g, w0, kw)
                    m, _, _ = adopt_dense(g, mask, km)
                    assert call(hb, w, m if masked else None, A, u, d) == want_info, what
                    compare_snapshots(snapshot(hb, w), want, what)
                    assert hb.lastmxv(d) == ob.lastmxv(od), what
                    cw(what)


@pytest.mark.parametrize("sr", ["PlusMultiplies", "MinimumPlus", "LogicalOrAnd"])
def test_k_spmv_on_carved_pointers(hb, ob, product_graph, sr):
    """the raw entry point: d_u, d_mask and d_w at every combination of offsets, against the oracle's pull product (the
    generic kernel: no fused Boolean mask)"""
    g = hb.g
    n, ptr, ind, val = product_graph
    rng = np.random.default_rng(30)
    A = hb.matrix_from_csr(n, ptr, ind, val)
    OA = ob.matrix_from_csr(n, ptr, ind, val)
    u = rng.integers(0, 4, n).astype(F)
    mask = (rng.random(n) < 0.5).astype(F)
    w0 = rng.integers(10, 20, n).astype(F)
    for tran in (0, 1):
        for masked, scmp in ((False, 0), (True, 0), (True, 1)):
            od = ob.descriptor(mxvmode=2, fusedmask=False)
            if scmp:
                ob.toggle(od, ob.ops.GrB_MASK)
            ou, ow, om = ob.vector(n, F), ob.vector(n, F), ob.vector(n, F)
            ob.build_dense(ou, u)
            ob.build_dense(ow, w0)
            ob.build_dense(om, mask)
            if tran:
                assert ob.vxm(ow, om if masked else None, None, sr, ou, OA, od) == 0
            else:
                assert ob.mxv(ow, om if masked else None, None, sr, OA, ou, od) == 0
            want = ob.dense_values(ow)
            for ku, kw, km in OFFSETS3:
                if not masked and km:
                    continue
                what = (sr, "tran", tran, "mask", masked, scmp, "k", ku, kw, km)
                pu, tu, _ = carve(u, ku)
                pm, tm, _ = carve(mask, km)
                pw, tw, cw = carve(w0, kw)
                assert g.k_spmv(A, tran, sr, pu, pm if masked else None, scmp, 0, pw) == 0, what
                got = payload(tw, kw, n, F)
                bad = np.flatnonzero(got != want)
                assert bad.size == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])
                cw(what)


@pytest.mark.parametrize("k", [5, 70])
@pytest.mark.parametrize("sr", ["PlusMultiplies", "MinimumPlus", "LogicalOrAnd"])
def test_spmm_on_carved_matrices(hb, ob, product_graph, sr, k):
    """B and C row-major at every pair of offsets; 70 columns take two launches (64 + 6)"""
    g = hb.g
    n, ptr, ind, val = product_graph
    rng = np.random.default_rng(31)
    A = hb.matrix_from_csr(n, ptr, ind, val)
    B = rng.integers(0, 3, (n, k)).astype(F)
    S = ob.Semiring(sr, F)
    want = np.empty((n, k), F)
    for i in range(n):                                                  # rows folded in CSR order, the identity for an empty row
        acc = np.full(k, S.identity(), F)
        for p in range(ptr[i], ptr[i + 1]):
            acc = S.add_op(acc, S.mul_op(np.full(k, val[p], F), B[ind[p]])).astype(F)
        want[i] = acc
    for kb in (0, 1, 3):
        for kc in (0, 1, 3):
            pb, tb, _ = carve(B, kb)
            pc, tc, cc = carve(np.full((n, k), 77, F), kc)
            assert g.spmm(sr, A, pb, pc, k, None) == 0
            got = payload(tc, kc, n * k, F).reshape(n, k)
            assert np.array_equal(got, want), (sr, k, kb, kc, np.argwhere(got != want)[:5])
            cc(("spmm", sr, k, kb, kc))


# ---- BFS into an adopted label vector ----------------------------------------------------------------------------------
def bfs_graphs():
    from graphblast_amd.graphgen import finalize_edges, grid_edges
    out = {}
    out["path45"] = finalize_edges(np.arange(44), np.arange(1, 45), 45, symmetrize=True)       # more levels than the 32 kept
    rng = np.random.default_rng(2)                                                             # rand200 of test_gpu_algorithms.py
    out["rand200"] = finalize_edges(rng.integers(0, 200, 500), rng.integers(0, 200, 500), 200, symmetrize=True)
    s, d, n = grid_edges(37, keep=1.0)                                                         # n = 1369: a last partial word
    out["grid37"] = finalize_edges(s, d, n, symmetrize=True)
    rng = np.random.default_rng(32)                                                            # n = 2 x 1024: whole lines at k = 0
    out["rand2048"] = finalize_edges(rng.integers(0, 2048, 9000), rng.integers(0, 2048, 9000), 2048, symmetrize=True)
    return out


@pytest.mark.parametrize("name", ["path45", "rand200", "grid37", "rand2048"])
def test_bfs_into_adopted_labels(hb, name):
    """the one-launch traversal (its label pass writes whole lines only into a 16-byte aligned vector, and element by element
    for vertices labelled beyond the kept levels) and the op-by-op loop (masked assign into v, v as the complemented mask)"""
    from oracle import simple_reference as sr
    g = hb.g
    gr = bfs_graphs()[name]
    n = gr["n"]
    ptr, ind = (np.asarray(x, I) for x in gr["csr"])
    cptr, cind = (np.asarray(x, I) for x in gr["csc"])
    assert (name != "rand2048" or n % 1024 == 0) and (name != "grid37" or n % 32 != 0)
    A = g.Matrix(n, n)
    assert A.build_csr(ptr, ind, np.ones(ind.size, F), csc=(cptr, cind, np.ones(cind.size, F))) == 0
    src = 0 if name == "path45" else int(np.nonzero(np.diff(ptr))[0][0])
    want = sr.bfs(ptr, ind, src)[0]
    if name == "path45":
        assert want.max() == 45                                          # levels beyond the 32 kept bitmaps: labelled directly
    routes = [("one launch", True, 0), ("op by op, push / pull", False, 0), ("op by op, pull", False, 2)]
    for route, fused, mode in routes:
        for k in KS:
            v, t, check = adopt_dense(g, np.full(n, -7, F), k)
            d = hb.descriptor(mxvmode=mode)
            info, res = g.bfs(v, A, src, d, fused=fused)
            assert info == 0, (name, route, k, info)
            got = hb.dense_values(v)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (name, route, "k", k, bad[:8], got[bad[:8]], want[bad[:8]])
            assert np.array_equal(payload(t, k, n, F), want), (name, route, k, "the caller's tensor holds the labels")
            check((name, route, k))


# ---- CDLP on an adopted matrix -----------------------------------------------------------------------------------------
def csc_of(S):
    T = sp.csc_matrix(S)
    T.sort_indices()
    return T.indptr.astype(I), T.indices.astype(I)


def adopted_cdlp_matrix(g, S, dt, rng, ks, kcs=None):
    """A over carved copies of S's arrays; kcs: the offsets of the CSC arrays, None for a CSR-only adoption"""
    n = S.shape[0]
    vals = rng.integers(-3, 4, S.nnz).astype(dt)
    csc = None
    if kcs is not None:
        cp, ci = csc_of(S)
        csc = (cp, ci, rng.integers(-3, 4, S.nnz).astype(dt))
    return adopt_csr(g, (n, n), dt, S.indptr.astype(I), S.indices.astype(I), vals, ks, csc, kcs)[0]


def hub_graph(n, draws, hubs, rng, symmetric):
    """random edges plus a few rows of 100 to 200 entries: lists longer than a wave's 64, which cd_stream walks"""
    r, c = [rng.integers(0, n, draws)], [rng.integers(0, n, draws)]
    for h, deg in hubs:
        r.append(np.full(deg, h))
        c.append(rng.choice(n, deg, replace=False))
    r, c = np.concatenate(r), np.concatenate(c)
    return cd._sym(n, r, c) if symmetric else cd._pattern(n, r, c)


@pytest.mark.parametrize("dt", [F, I])
def test_cdlp_undirected_on_carved_arrays(hb, dt):
    """ind at every offset: without a CSC (every task reads its own row: the pull form) and with one (a changed vertex
    marks along the CSC: cd_stream over csc.ind too)"""
    g = hb.g
    rng = np.random.default_rng(33)
    S = hub_graph(300, 1500, [(7, 200), (150, 120), (299, 100)], rng, True)
    assert np.diff(S.indptr).max() > cd.WAVE_LEN
    wants = {it: cd._ref(S, False, None, it) for it in (2, 20)}            # labels still moving, and settled
    assert wants[2][1]["changed"] > 0 and wants[20][1]["changed"] == 0
    Own = cd._matrix(g, S, dt, rng)
    owned = {it: cd._check(hb, S, Own, max_iter=it, name="owned", want=wants[it])[0] for it in wants}
    for ki in KS:
        for kc in (None, (ki + 1) % 4, ki):
            kcs = None if kc is None else ((ki + 2) % 4, kc, (ki + 3) % 4)
            A = adopted_cdlp_matrix(g, S, dt, rng, ((ki + 1) % 4, ki, (ki + 2) % 4), kcs)
            for it in wants:
                got, _, _ = cd._check(hb, S, A, max_iter=it, name=("undirected", dt.__name__, "k_ind", ki, "k_cind", kc, it), want=wants[it])
                assert np.array_equal(got, owned[it])


@pytest.mark.parametrize("dt", [F, I])
def test_cdlp_directed_on_carved_arrays(hb, dt):
    """rows and columns: csr.ind and csc.ind each at every offset"""
    g = hb.g
    rng = np.random.default_rng(34)
    S = hub_graph(300, 2500, [(3, 150), (160, 90)], rng, False)
    cp, _ = csc_of(S)
    assert (S != S.T).nnz > 0 and np.diff(S.indptr).max() > cd.WAVE_LEN and (np.diff(S.indptr) + np.diff(cp)).max() > 2 * cd.WAVE_LEN
    wants = {it: cd._ref(S, True, None, it) for it in (2, 20)}
    assert wants[2][1]["changed"] > 0 and wants[20][1]["changed"] == 0
    Own = cd._matrix(g, S, dt, rng)
    owned = {it: cd._check(hb, S, Own, directed=True, max_iter=it, name="owned", want=wants[it])[0] for it in wants}
    for ki in KS:
        for kc in KS:
            A = adopted_cdlp_matrix(g, S, dt, rng, (kc, ki, ki ^ 1), (ki, kc, kc ^ 2))
            for it in wants:
                got, _, _ = cd._check(hb, S, A, directed=True, max_iter=it, name=("directed", dt.__name__, "k_ind", ki, "k_cind", kc, it), want=wants[it])
                assert np.array_equal(got, owned[it])


def test_cdlp_long_row_on_carved_arrays(hb):
    """the crafted star of test_gpu_cdlp.py at the first length that takes the count array in global memory: 1024 threads
    walk the hub's list through cd_stream"""
    g = hb.g
    rng = np.random.default_rng(35)
    length = cd.BLOCK_LEN + 1
    n = length + 1
    hub = n // 2
    leaves = np.setdiff1d(np.arange(n), [hub])
    S = cd._sym(n, np.full(length, hub), leaves)
    assert S.indptr[hub + 1] - S.indptr[hub] == length
    mats = [adopted_cdlp_matrix(g, S, F, rng, (0, k, 0), kcs) for k in KS for kcs in (None, (0, (k + 2) % 4, 0))]
    for name, (init, want) in cd._crafted_inits(n, hub, leaves).items():
        ref = cd._ref(S, False, init, 1)
        for i, A in enumerate(mats):
            got, _, _ = cd._check(hb, S, A, init=init, max_iter=1, name=(length, name, "matrix", i), want=ref)
            assert want is None or got[hub] == want, (name, i, got[hub], want)


@pytest.mark.parametrize("dt, n, draws", [(F, 2000, 8000), (I, 2000, 8000), (F, 20000, 200000)])
def test_cdlp_random_undirected_on_an_adopted_aligned_matrix(hb, dt, n, draws):
    """the inputs of test_gpu_cdlp.py::test_random_undirected through grb_matrix_adopt_device_csr, every array aligned"""
    rng = np.random.default_rng(7)
    diag = np.sort(rng.choice(n, n // 10, replace=False))
    S = cd._sym(n, rng.integers(0, n, draws), rng.integers(0, n, draws), diag)
    want = cd._ref(S, False, None, 30)
    for kcs in (None, (0, 0, 0)):
        A = adopted_cdlp_matrix(hb.g, S, dt, rng, (0, 0, 0), kcs)
        _, res, history = cd._check(hb, S, A, max_iter=30, name=("adopted", n, dt.__name__, kcs), want=want)
        assert 3 <= res["iterations"] < 30 and res["changed"] == 0, res
