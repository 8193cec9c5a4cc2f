"""Host-side mirror of the reference frontend over the C ABI.

Same names, argument order and error behaviour as `graphblas::Vector`,
`graphblas::Matrix`, `graphblas::Descriptor` (graphblas/{vector,matrix,descriptor}.hpp)
and the free functions of graphblas/operations.hpp, so a test written against the
reference reads the same here.  Operations return the `graphblas::Info` code (they do
not raise) exactly like the reference's functions; container constructors raise on
allocation failure.  All compute happens in libgrb_hip.so -- this file moves pointers.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import BfsLevel, BfsResult, AlgoResult

# graphblas/types.hpp
GrB_NULL = None
GrB_ALL = None
(GrB_SUCCESS, GrB_UNINITIALIZED_OBJECT, GrB_NULL_POINTER, GrB_INVALID_VALUE, GrB_INVALID_INDEX,
 GrB_DOMAIN_MISMATCH, GrB_DIMENSION_MISMATCH, GrB_OUTPUT_NOT_EMPTY, GrB_NO_VALUE,
 GrB_NOT_IMPLEMENTED, GrB_OUT_OF_MEMORY, GrB_INSUFFICIENT_SPACE, GrB_INVALID_OBJECT,
 GrB_INDEX_OUT_OF_BOUNDS, GrB_PANIC) = range(15)
GrB_UNKNOWN, GrB_SPARSE, GrB_DENSE = 0, 1, 2
(GrB_MASK, GrB_OUTP, GrB_INP0, GrB_INP1, GrB_MODE, GrB_TA, GrB_TB, GrB_NT, GrB_MXVMODE, GrB_TOL,
 GrB_BACKEND) = range(11)
GrB_SCMP, GrB_REPLACE, GrB_TRAN, GrB_DEFAULT = 0, 1, 2, 3
GrB_PUSHPULL, GrB_PUSHONLY, GrB_PULLONLY = 10, 11, 12

F32, I32 = 0, 1
_NP = {F32: np.float32, I32: np.int32}

# graphblas/stddef.hpp:159-172 / :195-213 (order == include/grb_hip.h enums)
MONOIDS = ["Plus", "Multiplies", "Minimum", "Maximum", "LogicalOr", "LogicalAnd", "Greater",
           "CustomLess", "NotEqualTo"]
SEMIRINGS = ["LogicalOrAnd", "PlusMultiplies", "MinimumPlus", "MaximumMultiplies", "PlusDivides",
             "PlusGreater", "GreaterPlus", "PlusMinus", "PlusLess", "CustomLessPlus",
             "MinimumMultiplies", "MultipliesMultiplies", "NotEqualToPlus", "MinimumSelectSecond",
             "PlusNotEqualTo", "CustomLessLess", "MinimumNotEqualTo"]


def _monoid_id(op):
    if isinstance(op, int):
        return op
    name = op[:-len("Monoid")] if op.endswith("Monoid") else op
    return MONOIDS.index(name)


def _semiring_id(op):
    if isinstance(op, int):
        return op
    name = op[:-len("Semiring")] if op.endswith("Semiring") else op
    return SEMIRINGS.index(name)


BINARY_OPS = ["logical_or", "logical_and", "logical_xor", "equal", "not_equal_to", "greater", "less", "greater_equal",
              "less_equal", "first", "second", "minimum", "maximum", "plus", "minus", "multiplies", "divides"]


def register_semiring(add_op, add_identity, mul_op):
    """REGISTER_SEMIRING over REGISTER_MONOID (graphblas/stddef.hpp:140-191): a monoid (binary operator by name +
    identity) with any binary operator as the multiply.  Returns an id usable wherever a semiring name is."""
    out = C.c_int(0)
    _lib.call("grb_semiring_register", BINARY_OPS.index(add_op), float(add_identity), BINARY_OPS.index(mul_op),
              C.byref(out))
    return out.value


def _h(obj):
    return None if obj is None else obj._h


def _accum(accum):
    return 0 if accum is None else 1


def _dtype_code(dtype):
    if dtype in (F32, I32):
        return dtype
    dt = np.dtype(dtype)
    if dt == np.float32:
        return F32
    if dt == np.int32 or dt == np.bool_:
        return I32          # Vector<bool> of the reference maps to 4-byte ints
    raise TypeError("graphblast_amd supports float32 and int32 vectors/matrices")


class Descriptor:
    """graphblas::Descriptor (descriptor.hpp:17-39)."""

    def __init__(self):
        self._h = C.c_void_p()
        _lib.call("grb_descriptor_new", C.byref(self._h))

    def __del__(self):
        try:
            if self._h:
                _lib.load().grb_descriptor_free(self._h)
                self._h = None
        except Exception:
            pass

    def set(self, field, value):
        return _lib.load().grb_descriptor_set(self._h, field, value)

    def get(self, field):
        out = C.c_int(0)
        _lib.call("grb_descriptor_get", self._h, field, C.byref(out))
        return out.value

    def toggle(self, field):
        return _lib.load().grb_descriptor_toggle(self._h, field)

    def loadArgs(self, **vm):
        """Descriptor::loadArgs: parseArgs defaults (util.hpp:39-132), then the given flags."""
        info = _lib.load().grb_descriptor_load_defaults(self._h)
        for k, val in vm.items():
            if info != 0:
                break
            info = _lib.load().grb_descriptor_set_arg(self._h, k.encode(), float(val))
        return info

    def arg(self, name):
        out = C.c_double(0)
        _lib.call("grb_descriptor_get_arg", self._h, name.encode(), C.byref(out))
        return out.value

    @property
    def lastmxv_(self):
        out = C.c_int(0)
        _lib.call("grb_descriptor_lastmxv", self._h, C.byref(out))
        return out.value


class Vector:
    """graphblas::Vector<T> (vector.hpp:12-66); T in {float32, int32}."""

    def __init__(self, nsize, dtype=np.float32):
        self.dtype_code = _dtype_code(dtype)
        self.np_dtype = _NP[self.dtype_code]
        self._h = C.c_void_p()
        _lib.call("grb_vector_new", C.byref(self._h), self.dtype_code, int(nsize))
        self._keep = []

    def __del__(self):
        try:
            if self._h:
                _lib.load().grb_vector_free(self._h)
                self._h = None
        except Exception:
            pass

    # -- C API methods --------------------------------------------------------
    def dup(self, rhs):
        return _lib.load().grb_vector_dup(self._h, rhs._h)

    def clear(self):
        return _lib.load().grb_vector_clear(self._h)

    def size(self):
        out = C.c_int(0)
        _lib.call("grb_vector_size", self._h, C.byref(out))
        return out.value

    def nvals(self):
        out = C.c_int(0)
        _lib.call("grb_vector_nvals", self._h, C.byref(out))
        return out.value

    def build(self, *args):
        """build(indices, values, nvals, dup)  -> sparse;  build(values, nvals) -> dense."""
        lib = _lib.load()
        if len(args) >= 3 and args[1] is not None and not np.isscalar(args[1]):
            idx = np.ascontiguousarray(args[0], dtype=np.int32)
            val = np.ascontiguousarray(args[1], dtype=self.np_dtype)
            n = int(args[2])
            return lib.grb_vector_build_sparse(self._h, idx.ctypes.data, val.ctypes.data, n)
        val = np.ascontiguousarray(args[0], dtype=self.np_dtype)
        n = int(args[1]) if len(args) > 1 else val.size
        return lib.grb_vector_build_dense(self._h, val.ctypes.data, n)

    def build_device(self, d_values_ptr, nvals, d_indices_ptr=None):
        """build(T* values, nvals) / build(Index*, T*, nvals): adopt device pointers."""
        lib = _lib.load()
        if d_indices_ptr is None:
            return lib.grb_vector_adopt_dense(self._h, d_values_ptr, int(nvals))
        return lib.grb_vector_adopt_sparse(self._h, d_indices_ptr, d_values_ptr, int(nvals))

    def resize(self, nsize):
        return _lib.load().grb_vector_resize(self._h, int(nsize))

    def setElement(self, val, index):
        return _lib.load().grb_vector_set_element(self._h, float(val), int(index))

    def extractElement(self, index):
        out = C.c_double(0)
        info = _lib.load().grb_vector_extract_element(self._h, C.byref(out), int(index))
        return info, self.np_dtype(out.value)

    def extractTuples(self, n=None, sparse=False):
        """extractTuples(values, n) (dense; densifies a sparse vector with fill 0) or, with
        sparse=True, extractTuples(indices, values, n).  Returns (info, ...arrays)."""
        lib = _lib.load()
        if sparse:
            n = self.nvals() if n is None else int(n)
            idx = np.zeros(max(n, 1), dtype=np.int32)
            val = np.zeros(max(n, 1), dtype=self.np_dtype)
            cn = C.c_int(n)
            info = lib.grb_vector_extract_tuples_sparse(self._h, idx.ctypes.data, val.ctypes.data, C.byref(cn))
            return info, idx[:n], val[:n]
        n = self.size() if n is None else int(n)
        val = np.zeros(max(n, 1), dtype=self.np_dtype)
        cn = C.c_int(n)
        info = lib.grb_vector_extract_tuples_dense(self._h, val.ctypes.data, C.byref(cn))
        return info, val[:n]

    def fill(self, val):
        return _lib.load().grb_vector_fill(self._h, float(val))

    def fillAscending(self, nvals=0):
        return _lib.load().grb_vector_fill_ascending(self._h, int(nvals))

    def getStorage(self):
        out = C.c_int(0)
        _lib.call("grb_vector_get_storage", self._h, C.byref(out))
        return out.value

    def setStorage(self, storage):
        return _lib.load().grb_vector_set_storage(self._h, int(storage))

    def swap(self, rhs):
        return _lib.load().grb_vector_swap(self._h, rhs._h)

    # backend::Vector methods the reference's tests reach through `#define private public`
    def convert(self, identity, switchpoint, desc):
        return _lib.load().grb_vector_convert(self._h, float(identity), float(switchpoint), desc._h)

    def sparse2dense(self, identity, desc=None):
        return _lib.load().grb_vector_sparse2dense(self._h, float(identity), _h(desc))

    def dense2sparse(self, identity, desc):
        return _lib.load().grb_vector_dense2sparse(self._h, float(identity), desc._h)

    def device_ptrs(self):
        a, b, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.call("grb_vector_device_ptrs", self._h, C.byref(a), C.byref(b), C.byref(c))
        return a.value, b.value, c.value


class Matrix:
    """graphblas::Matrix<T> (matrix.hpp:13-84)."""

    def __init__(self, nrows, ncols, dtype=np.float32):
        self.dtype_code = _dtype_code(dtype)
        self.np_dtype = _NP[self.dtype_code]
        self._h = C.c_void_p()
        self._nrows, self._ncols = int(nrows), int(ncols)
        _lib.call("grb_matrix_new", C.byref(self._h), self.dtype_code, self._nrows, self._ncols)
        self._keep = []

    def __del__(self):
        try:
            if self._h:
                _lib.load().grb_matrix_free(self._h)
                self._h = None
        except Exception:
            pass

    @classmethod
    def from_mtx(cls, path, dtype=np.float32, directed=0):
        """readMtx + build with the MatrixMarket text parsed on the device (grb_matrix_load_mtx);
        `directed` as readMtx: 0 = symmetric iff the banner says so, 1 = directed, 2 = undirected."""
        self = cls.__new__(cls)
        self.dtype_code = _dtype_code(dtype)
        self.np_dtype = _NP[self.dtype_code]
        self._h = C.c_void_p()
        self._keep = []
        dims = (C.c_int * 3)()
        info = _lib.load().grb_matrix_load_mtx(C.byref(self._h), str(path).encode(), self.dtype_code, int(directed), dims)
        if info != 0:
            self._h = None
            raise RuntimeError("grb_matrix_load_mtx(%s): Info %d" % (path, info))
        self._nrows, self._ncols = int(dims[0]), int(dims[1])
        return self

    def build(self, row_indices, col_indices, values, nvals=None, dup=None):
        r = np.ascontiguousarray(row_indices, dtype=np.int32)
        c = np.ascontiguousarray(col_indices, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=self.np_dtype)
        n = r.size if nvals is None else int(nvals)
        return _lib.load().grb_matrix_build(self._h, r.ctypes.data, c.ctypes.data, v.ctypes.data, n)

    def build_csr(self, row_ptr, col_ind, values, csc=None):
        p = np.ascontiguousarray(row_ptr, dtype=np.int32)
        i = np.ascontiguousarray(col_ind, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=self.np_dtype)
        if csc is None:
            return _lib.load().grb_matrix_build_csr(self._h, p.ctypes.data, i.ctypes.data, v.ctypes.data,
                                                    i.size, None, None, None)
        cp = np.ascontiguousarray(csc[0], dtype=np.int32)
        ci = np.ascontiguousarray(csc[1], dtype=np.int32)
        cv = np.ascontiguousarray(csc[2], dtype=self.np_dtype)
        return _lib.load().grb_matrix_build_csr(self._h, p.ctypes.data, i.ctypes.data, v.ctypes.data, i.size,
                                                cp.ctypes.data, ci.ctypes.data, cv.ctypes.data)

    def build_device_csr(self, d_ptr, d_ind, d_val, nvals, d_cptr=None, d_cind=None, d_cval=None, keep=()):
        """build(row_ptr, col_ind, values, nvals) adopting device pointers; `keep` holds
        whatever owns that memory (e.g. torch tensors) alive."""
        self._keep = list(keep)
        return _lib.load().grb_matrix_adopt_device_csr(self._h, d_ptr, d_ind, d_val, int(nvals), d_cptr, d_cind,
                                                       d_cval)

    def ingest_device(self, d_rows, d_cols, d_vals, nvals, symmetrize=False, drop_selfloops=True,
                      drop_duplicates=True, keep=()):
        """readMtx's loader semantics + build on a DEVICE coordinate list (graphblas/util.hpp:197-329,
        363-430): optionally add the reverse of every off-diagonal entry, drop self loops, drop
        duplicates (first wins); d_vals None = pattern."""
        self._keep = list(keep)
        flags = (1 if symmetrize else 0) | (2 if drop_selfloops else 0) | (4 if drop_duplicates else 0)
        return _lib.load().grb_matrix_ingest_device(self._h, d_rows, d_cols, d_vals, int(nvals), flags)

    def nrows(self):
        return self._nrows

    def ncols(self):
        return self._ncols

    def nvals(self):
        out = C.c_int(0)
        _lib.call("grb_matrix_nvals", self._h, C.byref(out))
        return out.value

    def _host(self, which):
        p, i, v = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _lib.call(which, self._h, C.byref(p), C.byref(i), C.byref(v))
        n = self._nrows if which.endswith("csr") else self._ncols
        nv = self.nvals()
        ptr = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(n + 1,)).copy()
        if nv == 0:                      # e.g. data/small/test_sgm.mtx: only self loops -> empty
            return ptr, np.zeros(0, dtype=np.int32), np.zeros(0, dtype=self.np_dtype)
        ind = np.ctypeslib.as_array(C.cast(i, C.POINTER(C.c_int32)), shape=(nv,)).copy()
        raw = np.ctypeslib.as_array(C.cast(v, C.POINTER(C.c_uint32)), shape=(nv,)).copy()
        return ptr, ind, raw.view(self.np_dtype)

    def host_csr(self):
        """h_csrRowPtr_, h_csrColInd_, h_csrVal_ (what the CPU oracles read)."""
        return self._host("grb_matrix_host_csr")

    def host_csc(self):
        return self._host("grb_matrix_host_csc")

    def write_cache(self, path):
        """The reference's binary CSR cache (sparse_matrix.hpp:328-348): int32 nrows, nvals, rowptr, colind."""
        return _lib.load().grb_matrix_write_cache(self._h, os.fsencode(str(path)))

    def build_cache(self, path):
        """Matrix::build(dat_name) (sparse_matrix.hpp:355-407): values = 1, CSC made on the device."""
        info = _lib.load().grb_matrix_build_cache(self._h, os.fsencode(str(path)))
        if info == 0:
            n = C.c_int(0)
            _lib.call("grb_matrix_nrows", self._h, C.byref(n))
            self._nrows = self._ncols = n.value
        return info

    def set_values(self, csr_values):
        v = np.ascontiguousarray(csr_values, dtype=self.np_dtype)
        return _lib.load().grb_matrix_set_values(self._h, v.ctypes.data)


def cache_name(mtx_path, is_undirected):
    """util.hpp:340-357 (convert): `<dir>/.<file>.<ud|d>.<nosl|sl>.bin`."""
    buf = C.create_string_buffer(1024)
    _lib.call("grb_cache_name", os.fsencode(str(mtx_path)), int(bool(is_undirected)), buf, 1024)
    return buf.value.decode()


# ---- graphblas/operations.hpp ------------------------------------------------------
def vxm(w, mask, accum, op, u, A, desc):
    return _lib.load().grb_vxm(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(u), _h(A), _h(desc))


def mxv(w, mask, accum, op, A, u, desc):
    return _lib.load().grb_mxv(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(A), _h(u), _h(desc))


def eWiseMult(w, mask, accum, op, u, v, desc):
    """eWiseMult(w, mask, accum, op, u, v, desc) on vectors, or with u a Matrix the matrix form (see eWiseAdd): C = op(A) (x)
    op(B) on the intersection of the two structures, C(i,j) = mul(a, b)."""
    if isinstance(u, Matrix) or isinstance(w, Matrix):
        return _lib.load().grb_matrix_eWiseMult(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(u), _h(v), _h(desc))
    return _lib.load().grb_eWiseMult(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(u), _h(v), _h(desc))


def eWiseAdd(w, mask, accum, op, u, v, desc):
    """eWiseAdd(w, mask, accum, op, u, v | scalar, desc).  With u a Matrix: C = op(A) (+) op(B) (GrB_INP0 / GrB_INP1 =
    GrB_TRAN transpose an operand, read from its CSC) on the union of the two structures, C(i,j) = add(a, b) where both
    store an entry and the stored value where one does; stored zeros are kept.  A mask keeps the entries where it stores a
    nonzero (inverted by GrB_SCMP).  f32 or i32, all three alike (GrB_NOT_IMPLEMENTED otherwise); C may be A, B or the
    mask; shapes -> GrB_DIMENSION_MISMATCH, a transposed operand without its CSC -> GrB_INVALID_OBJECT, more than INT32_MAX
    entries -> GrB_OUT_OF_MEMORY (C unchanged on every error).  C gets a CSC too when every input has its other
    orientation.  Returns the info code."""
    if isinstance(u, Matrix) or isinstance(w, Matrix):
        return _lib.load().grb_matrix_eWiseAdd(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(u), _h(v), _h(desc))
    if isinstance(v, Vector):
        return _lib.load().grb_eWiseAdd(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(u), _h(v), _h(desc))
    return _lib.load().grb_eWiseAdd_scalar(_h(w), _h(mask), _accum(accum), _semiring_id(op), _h(u), float(v),
                                           _h(desc))


def reduce(accum, op, u, desc, w=None, mask=None):
    """reduce(&val, accum, MonoidT, Vector u, desc) -> (info, val)  or, with w given and u a
    Matrix, reduce(Vector w, mask, accum, MonoidT, Matrix A, desc) -> info."""
    if isinstance(u, Matrix):
        return _lib.load().grb_reduce_matrix_rows(_h(w), _h(mask), _accum(accum), _monoid_id(op), _h(u), _h(desc))
    out = C.c_double(0)
    info = _lib.load().grb_reduce_vector(C.byref(out), _accum(accum), _monoid_id(op), _h(u), _h(desc))
    return info, out.value


def assign(w, mask, accum, val, indices, nindices, desc):
    """assign(w, mask, accum, val, GrB_ALL, n, desc)."""
    if indices is not None:
        return GrB_NOT_IMPLEMENTED
    return _lib.load().grb_assign(_h(w), _h(mask), _accum(accum), float(val), _h(desc))


UNARY_OPS = ["identity", "ainv", "minv", "abs", "lnot", "bind_first", "bind_second"]      # grb_unary_op
BINARY_OPS = ["logical_or", "logical_and", "logical_xor", "equal", "not_equal_to", "greater", "less", "greater_equal",
              "less_equal", "first", "second", "minimum", "maximum", "plus", "minus", "multiplies", "divides"]


def apply(w, mask, accum, unary, u, desc, binop=None, scalar=0.0):
    """apply on the device (grb_vector_apply / grb_matrix_apply): w = f(u) on every stored element.  unary: a name of
    UNARY_OPS; the two bind kinds take binop (a name of BINARY_OPS) and scalar."""
    k = UNARY_OPS.index(unary)
    b = BINARY_OPS.index(binop) if binop is not None else 0
    fn = "grb_matrix_apply" if isinstance(w, Matrix) else "grb_vector_apply"
    return getattr(_lib.load(), fn)(_h(w), _h(mask), _accum(accum), k, b, float(scalar), _h(u), _h(desc))


def mxm(Cm, mask, accum, op, A, B, desc):
    """graphblas::mxm: C = op(A) (+.x) op(B) (GrB_INP0 / GrB_INP1 = GrB_TRAN transpose an operand).  With a mask, C takes
    the mask's structure.  With mask=None, the unmasked product: float32 A, B and C only (GrB_NOT_IMPLEMENTED otherwise),
    any semiring, products folded over k ascending; C == A or B -> GrB_NOT_IMPLEMENTED, shapes -> GrB_DIMENSION_MISMATCH,
    a transposed operand without its CSC -> GrB_INVALID_OBJECT, more than INT32_MAX results -> GrB_OUT_OF_MEMORY (C
    unchanged).  Returns the info code."""
    return _lib.load().grb_mxm(_h(Cm), _h(mask), _accum(accum), _semiring_id(op), _h(A), _h(B), _h(desc))


def kronecker(Cm, mask, accum, op, A, B, desc):
    """GraphBLAS's kronecker: C = op(A) (x) op(B) (GrB_INP0 / GrB_INP1 = GrB_TRAN transpose an operand, read from its
    CSC).  With op(A) mA x nA and op(B) mB x nB, C is (mA * mB) x (nA * nB) and C(iA * mB + iB, jA * nB + jB) = mul(a, b)
    wherever both entries are stored, mul the multiply of op (a semiring name or a registered id; its monoid is not used), a
    first; stored zeros count, so C.nvals() == A.nvals() * B.nvals().  f32 or i32, all three alike (GrB_NOT_IMPLEMENTED
    otherwise); a mask -> GrB_NOT_IMPLEMENTED; C may be A, B or both; shapes -> GrB_DIMENSION_MISMATCH, a transposed operand
    without its CSC -> GrB_INVALID_OBJECT, more than INT32_MAX entries -> GrB_OUT_OF_MEMORY, an unknown semiring id ->
    GrB_INVALID_VALUE (C unchanged on every error).  C gets a CSC too when both operands have their other orientation.
    Returns the info code."""
    return _lib.load().grb_kronecker(_h(Cm), _h(mask), _accum(accum), _semiring_id(op), _h(A), _h(B), _h(desc))


def transpose(Cm, mask, accum, A, desc):
    """graphblas::transpose: C = A^T, or C = A under GrB_INP0 = GrB_TRAN, with both orientations (a CSR-only A, such as a
    product result, is sorted on the device).  f32 or i32, C of A's type; a mask -> GrB_NOT_IMPLEMENTED; C may be A; C
    unchanged on every error.  Returns the info code."""
    return _lib.load().grb_transpose(_h(Cm), _h(mask), _accum(accum), _h(A), _h(desc))


def _index_list(indices, dim):
    """None (GrB_ALL) -> (None, dim); anything else -> a contiguous int32 array and its length"""
    if indices is None:
        return None, int(dim)
    a = np.ascontiguousarray(np.asarray(indices, np.int32).reshape(-1))
    return a, a.size


def extract(out, mask, accum, src, rows, cols, desc):
    """graphblas::extract, the three forms by the types of out and src; rows / cols are None (GrB_ALL: every index in
    order) or anything np.asarray(..., np.int32) takes, in any order, duplicates allowed (a duplicate repeats a row, a
    column or an element).  GrB_INP0 = GrB_TRAN reads A^T (from A's CSC; for the column form: row `cols` of A).
    Matrix, Matrix: C = op(A)(rows, cols), C(i, j) = op(A)(rows[i], cols[j]) where stored (stored zeros kept, values
    copied bit for bit, columns ascending); f32 or i32, C of A's type; C may be A; C gets a CSC too when op(A) has its other
    orientation.  Vector, Matrix: w = op(A)(rows, cols) with cols an int: a sparse w of size len(rows).  Vector, Vector
    (cols must be None): w = u(rows), dense for a dense u and sparse for a sparse one; w may be u.  A mask ->
    GrB_NOT_IMPLEMENTED; shapes that differ from the lists' lengths -> GrB_DIMENSION_MISMATCH; an index outside op(A) / u ->
    GrB_INDEX_OUT_OF_BOUNDS; a transposed operand without its CSC -> GrB_INVALID_OBJECT; more than INT32_MAX entries ->
    GrB_OUT_OF_MEMORY (the output unchanged on every error).  Returns the info code."""
    lib = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data
    tran = desc is not None and desc.get(GrB_INP0) == GrB_TRAN
    if isinstance(out, Matrix):
        m, n = (0, 0) if src is None else (src.ncols(), src.nrows()) if tran else (src.nrows(), src.ncols())
        r, nr = _index_list(rows, m)
        c, nc = _index_list(cols, n)
        return lib.grb_matrix_extract(_h(out), _h(mask), _accum(accum), _h(src), ptr(r), nr, ptr(c), nc, _h(desc))
    if isinstance(src, Matrix):
        r, nr = _index_list(rows, src.ncols() if tran else src.nrows())
        if not isinstance(cols, (int, np.integer)):
            raise TypeError("extract(Vector, Matrix): cols is the column's index")
        return lib.grb_matrix_extract_col(_h(out), _h(mask), _accum(accum), _h(src), ptr(r), nr, int(cols), _h(desc))
    if cols is not None:
        raise TypeError("extract(Vector, Vector): cols must be None")
    r, nr = _index_list(rows, src.size() if src is not None else 0)
    return lib.grb_vector_extract(_h(out), _h(mask), _accum(accum), _h(src), ptr(r), nr, _h(desc))


SELECT_OPS = ["tril", "triu", "diag", "offdiag", "rowle", "rowgt", "colle", "colgt",
              "valueeq", "valuene", "valuelt", "valuele", "valuegt", "valuege"]             # grb_select_op


def select(out, mask, accum, op, src, thunk, desc):
    """GraphBLAS's select: out keeps exactly the stored entries of op(src) for which the predicate holds, values bit for
    bit, order unchanged.  op is a name of SELECT_OPS; with i, j the entry's row and column in op(src) (a Vector: j = 0),
    a its value and k the thunk: tril j <= i + k, triu j >= i + k, diag j == i + k, offdiag j != i + k, rowle i <= k,
    rowgt i > k, colle j <= k, colgt j > k, valueeq / valuene / valuelt / valuele / valuegt / valuege compare a with k.
    select(C, None, None, "valuene", A, 0, desc) drops the stored zeros; "tril" with thunk 0 is the lower triangle.
    Matrix: f32 or i32, C of A's type and of op(A)'s shape; C may be A; GrB_INP0 = GrB_TRAN reads A^T from A's CSC; C gets a
    CSC too when op(A) has its other orientation.  Vector: w of u's size and type becomes sparse; w may be u.  A positional
    thunk must be an integer, a value thunk on i32 an integer that fits (else GrB_INVALID_VALUE); a mask ->
    GrB_NOT_IMPLEMENTED; the output unchanged on every error (grb_hip.h lists the codes).  Returns the info code."""
    k = SELECT_OPS.index(op)
    fn = "grb_matrix_select" if isinstance(out, Matrix) else "grb_vector_select"
    return getattr(_lib.load(), fn)(_h(out), _h(mask), _accum(accum), k, float(thunk), _h(src), _h(desc))


def assign_matrix(Cm, mask, accum, src, rows, cols, desc):
    """graphblas::assign into a matrix (GrB_assign without GrB_REPLACE), the form by the type of src: a Matrix --
    C(rows, cols) = op(A); a Vector -- C(rows, j) = u when cols is an int, C(i, cols) = u when rows is one; a number --
    C(rows, cols) = val.  rows / cols are None (GrB_ALL) or anything np.asarray(..., np.int32) takes, in any order,
    without repeats (a repeated index -> GrB_INVALID_INDEX).  accum is None or a name of BINARY_OPS, applied as
    accum(c, t).  Without an accum the entries of C inside rows x cols that the source does not store are deleted; with a
    Matrix mask (matrix and number forms) C changes only where the mask stores a nonzero (GrB_MASK = GrB_SCMP inverts it).
    Stored zeros count; f32 or i32, src of C's type; C may be src or the mask; C unchanged on every error (grb_hip.h lists
    the codes).  Returns the info code."""
    lib = _lib.load()
    ptr = lambda a: None if a is None else a.ctypes.data
    op = -1 if accum is None else BINARY_OPS.index(accum)
    if isinstance(src, Matrix):
        r, nr = _index_list(rows, Cm.nrows())
        c, nc = _index_list(cols, Cm.ncols())
        return lib.grb_matrix_assign(_h(Cm), _h(mask), op, _h(src), ptr(r), nr, ptr(c), nc, _h(desc))
    if isinstance(src, Vector):
        row_is_int = isinstance(rows, (int, np.integer))
        col_is_int = isinstance(cols, (int, np.integer))
        if row_is_int == col_is_int:
            raise TypeError("assign_matrix(Matrix, Vector): exactly one of rows / cols is the row's or column's index")
        if col_is_int:
            r, nr = _index_list(rows, Cm.nrows())
            return lib.grb_matrix_assign_col(_h(Cm), _h(mask), op, _h(src), ptr(r), nr, int(cols), _h(desc))
        c, nc = _index_list(cols, Cm.ncols())
        return lib.grb_matrix_assign_row(_h(Cm), _h(mask), op, _h(src), int(rows), ptr(c), nc, _h(desc))
    r, nr = _index_list(rows, Cm.nrows())
    c, nc = _index_list(cols, Cm.ncols())
    return lib.grb_matrix_assign_scalar(_h(Cm), _h(mask), op, float(src), ptr(r), nr, ptr(c), nc, _h(desc))


def tril(Cm, A, desc):
    return _lib.load().grb_matrix_tril(_h(Cm), _h(A), _h(desc))


def reduce_matrix(accum, op, A, desc):
    out = C.c_double(0)
    info = _lib.load().grb_reduce_matrix_scalar(C.byref(out), _accum(accum), _monoid_id(op), _h(A), _h(desc))
    return info, out.value


def assignScatter(w, mask, accum, u, indices, desc):
    return _lib.load().grb_assignScatter(_h(w), _h(mask), _accum(accum), _h(u), _h(indices), _h(desc))


def extractGather(w, mask, accum, u, indices, desc):
    return _lib.load().grb_extractGather(_h(w), _h(mask), _accum(accum), _h(u), _h(indices), _h(desc))


# ---- graphblas/algorithm/*.hpp -----------------------------------------------------
def bfs(v, A, s, desc, fused=False, profile=False, max_levels=4096):
    """algorithm::bfs. Returns (info, result dict). fused=True runs the device-resident loop."""
    res = BfsResult()
    if not fused:
        info = _lib.load().grb_bfs(_h(v), _h(A), int(s), _h(desc), C.byref(res))
        return info, dict(levels=res.levels, tight_ms=res.tight_ms)
    if not profile:                     # no per-level table wanted: nothing to allocate or copy back
        info = _lib.load().grb_bfs_fused(_h(v), _h(A), int(s), _h(desc), C.byref(res), None, 0, 0)
        levels = []
    else:
        lv = (BfsLevel * max_levels)()
        info = _lib.load().grb_bfs_fused(_h(v), _h(A), int(s), _h(desc), C.byref(res), lv, max_levels,
                                         int(profile))
        n = min(res.levels, max_levels)
        levels = [dict(direction="pull" if lv[i].direction else "push", frontier=lv[i].frontier,
                       frontier_edges=lv[i].frontier_edges, discovered=lv[i].discovered, ms=lv[i].ms)
                  for i in range(n)]
    return info, dict(levels=res.levels, tight_ms=res.tight_ms, edges_traversed=res.edges_traversed,
                      reached=res.reached, per_level=levels)


def bfs_enqueue(v, A, s, desc):
    """grb_bfs_fused_enqueue: queue the traversal on the library's stream and return (info, ticket) without waiting.
    v, A and desc must stay alive until bfs_wait(ticket)."""
    t = C.c_int64(0)
    info = _lib.load().grb_bfs_fused_enqueue(_h(v), _h(A), int(s), _h(desc), C.byref(t))
    return info, t.value


def bfs_wait(ticket):
    """grb_bfs_wait: (info, result dict) of a queued traversal; what bfs(..., fused=True) would have returned."""
    res = BfsResult()
    info = _lib.load().grb_bfs_wait(C.c_int64(ticket), C.byref(res))
    return info, dict(levels=res.levels, tight_ms=res.tight_ms, edges_traversed=res.edges_traversed,
                      reached=res.reached, per_level=[])


def bfs_set_lanes(n=-1):
    """grb_bfs_set_lanes: traversals in flight at once for bfs_enqueue (n < 1 only queries); returns the previous value."""
    return int(_lib.load().grb_bfs_set_lanes(int(n)))


def bfs_set_sweep_from(k=-1):
    """grb_bfs_set_sweep_from: gathered traversals from which bfs_enqueue's groups run as one bit-parallel sweep (0: never;
    k < 0 only queries); returns the previous value."""
    return int(_lib.load().grb_bfs_set_sweep_from(int(k)))


def bfs_sweep_counts():
    """grb_bfs_sweep_counts: {"sweeps", "traversals"} -- the groups bfs_enqueue's queue has run as one sweep so far."""
    a, b = C.c_longlong(0), C.c_longlong(0)
    info = _lib.load().grb_bfs_sweep_counts(C.byref(a), C.byref(b))
    assert info == 0, info
    return {"sweeps": int(a.value), "traversals": int(b.value)}


def bfs_set_coschedule(k=-1):
    """grb_bfs_set_coschedule: traversals per launch for bfs_enqueue (k < 1 only queries); returns the previous value."""
    return int(_lib.load().grb_bfs_set_coschedule(int(k)))


def bfs_coschedule_profile(on):
    """grb_bfs_coschedule_profile: on=True starts HIP events around the launches of several traversals; on=False stops and
    returns dict(ms_total, launches, traversals)."""
    ms, nl, nt = C.c_double(0), C.c_int(0), C.c_int(0)
    info = _lib.load().grb_bfs_coschedule_profile(1 if on else 0, C.byref(ms), C.byref(nl), C.byref(nt))
    assert info == 0, info
    return dict(ms_total=ms.value, launches=nl.value, traversals=nt.value)


def bfs_host_times(reset=False):
    """Host microseconds spent queueing / waiting inside the one-launch traversal since the last reset, and the calls."""
    e, w, n = C.c_double(0), C.c_double(0), C.c_longlong(0)
    _lib.call("grb_bfs_host_times", C.byref(e), C.byref(w), C.byref(n), int(bool(reset)))
    return dict(enqueue_us=e.value, wait_us=w.value, calls=n.value)


def spmm(op, A, d_B, d_C, k, desc=None, tran=False):
    """C = A (+).(x) B with dense row-major device arrays B [ncols x k], C [nrows x k] (grb_spmm)."""
    return _lib.load().grb_spmm(_semiring_id(op), _h(A), int(bool(tran)), d_B, d_C, int(k), _h(desc))


def bfs_batch(vs, A, sources, desc):
    """Up to 64 traversals at once (grb_bfs_batch): vs[i] receives the depth labels of sources[i]."""
    k = len(vs)
    assert k == len(sources)
    handles = (C.c_void_p * k)(*[_h(v) for v in vs])
    src = np.ascontiguousarray(sources, dtype=np.int32)
    res = BfsResult()
    info = _lib.load().grb_bfs_batch(handles, k, _h(A), src.ctypes.data, _h(desc), C.byref(res))
    return info, dict(levels=res.levels, tight_ms=res.tight_ms, edges_traversed=res.edges_traversed,
                      reached=res.reached)


def bfs_batch_set_tail(edges=-1):
    """Out-edge limit of the levels grb_bfs_batch runs inside its one light-level launch (grb_bfs_batch_set_tail):
    0 never, < 0 only queries; returns the previous limit."""
    return int(_lib.load().grb_bfs_batch_set_tail(int(edges)))


def bfs_batch_hot(A):
    """The hot block the batched traversal keeps for A (grb_bfs_batch_hot; built if A has none yet): dict(H, t, cap, hubs) --
    the hubs are the vertices of out-degree >= t, ascending; H = 0: A sweeps without one."""
    lib = _lib.load()
    H, t, cap = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
    info = lib.grb_bfs_batch_hot(_h(A), C.byref(H), C.byref(t), C.byref(cap), None, 0)
    assert info == 0, info
    hubs = np.zeros(max(int(H.value), 1), dtype=np.int32)
    info = lib.grb_bfs_batch_hot(_h(A), None, None, None, hubs.ctypes.data, int(H.value))
    assert info == 0, info
    return dict(H=int(H.value), t=int(t.value), cap=int(cap.value), hubs=hubs[:int(H.value)])


def sssp(v, A, s, desc):
    res = AlgoResult()
    info = _lib.load().grb_sssp(_h(v), _h(A), int(s), _h(desc), C.byref(res))
    return info, dict(iterations=res.iterations, tight_ms=res.tight_ms, succ=res.last_value)


def pr(p, A, alpha, eps, desc):
    res = AlgoResult()
    info = _lib.load().grb_pr(_h(p), _h(A), float(alpha), float(eps), _h(desc), C.byref(res))
    return info, dict(iterations=res.iterations, tight_ms=res.tight_ms, error=res.last_value)


def cc(v, A, seed, desc):
    res = AlgoResult()
    info = _lib.load().grb_cc(_h(v), _h(A), int(seed), _h(desc), C.byref(res))
    return info, dict(iterations=res.iterations, tight_ms=res.tight_ms, succ=res.last_value)


def tc(A, B, desc):
    res = AlgoResult()
    n = C.c_int64(0)
    info = _lib.load().grb_tc(C.byref(n), _h(A), _h(B), _h(desc), C.byref(res))
    return info, n.value, dict(tight_ms=res.tight_ms)


def _truss_dict(res):
    return dict(rounds=res.rounds, supports=res.supports, edges=res.edges, result_edges=res.result_edges, kmax=res.kmax,
                loop_ms=res.loop_ms)


def ktruss(Cm, A, k, desc):
    """grb_ktruss: Cm = the k-truss of A's graph, the largest subgraph in which every edge lies in at least k - 2 triangles
    of the subgraph.  A is n x n with a symmetric structure; its values are never read (stored zeros are edges), its
    diagonal takes no part.  Cm is n x n, f32 or i32 whatever A's type, holds both directions of every surviving edge
    (columns ascending, rows that lose everything stay empty, CSC = a copy of the CSR) and Cm(i, j) is the edge's support:
    the common neighbours of i and j inside the truss.  k = 2 is the whole graph with its supports.  Cm may be A; the same
    inputs give the same bits.  k < 2 -> GrB_INVALID_VALUE; A not square or Cm not n x n -> GrB_DIMENSION_MISMATCH; a type
    outside f32 / i32 -> GrB_NOT_IMPLEMENTED; an A without its own CSC (a product result) -> GrB_INVALID_OBJECT; an A that
    is not symmetric -> GrB_INVALID_VALUE (Cm unchanged on every error).  Returns (info, dict(rounds, supports, edges,
    result_edges, kmax = k, loop_ms))."""
    res = _lib.TrussResult()
    info = _lib.load().grb_ktruss(_h(Cm), _h(A), int(k), _h(desc), C.byref(res))
    return info, _truss_dict(res)


def trussness(Cm, A, desc):
    """grb_trussness: Cm gets the structure of A's graph (A as for ktruss: symmetric structure, values never read, no
    diagonal) and Cm(i, j) = the largest k such that the edge {i, j} is in the k-truss: 2 for an edge in no triangle.  Types,
    orientations, aliasing and error codes as for ktruss.  Returns (info, dict(rounds, supports, edges, result_edges,
    kmax = the largest k with a non-empty truss, loop_ms))."""
    res = _lib.TrussResult()
    info = _lib.load().grb_trussness(_h(Cm), _h(A), _h(desc), C.byref(res))
    return info, _truss_dict(res)


def bc(v, A, sources, desc):
    """grb_bc: v = the betweenness centrality of A's graph by batched Brandes, 64 sources per sweep.  A is n x n, f32 or
    i32; its values are never read (stored zeros are edges), a stored A(i, j), i != j, is the edge i -> j, its diagonal
    takes no part and its structure need not be symmetric.  sources: vertex ids (a source listed twice counts twice), or
    None for every vertex (exact centrality).  v is an f32 vector of size n and becomes dense: v[x] = the sum over the
    sources s of delta_s(x), not normalised and not halved (all sources on a symmetric graph count every unordered pair
    twice, as LAGraph does), exactly 0 for a vertex between no pair.  Path counts and dependencies are f64, v is rounded
    to f32 once; the same inputs give the same bits.  An empty list -> GrB_INVALID_VALUE; a source outside 0 .. n - 1 ->
    GrB_INVALID_INDEX; A not square or v not of size n -> GrB_DIMENSION_MISMATCH; v not f32 or A outside f32 / i32 ->
    GrB_NOT_IMPLEMENTED; an A without its own CSC (a product result) -> GrB_INVALID_OBJECT (v unchanged on every error).
    Returns (info, dict(sources, batches, levels = the largest depth + 1, reached = vertices reached summed over the
    sources, loop_ms))."""
    res = _lib.BcResult()
    if sources is None:
        info = _lib.load().grb_bc(_h(v), _h(A), None, 0, _h(desc), C.byref(res))
    else:
        src = np.ascontiguousarray(sources, dtype=np.int32).ravel()
        buf = src if src.size else np.zeros(1, np.int32)   # an empty list is an error of the call, not "every vertex"
        info = _lib.load().grb_bc(_h(v), _h(A), buf.ctypes.data, int(src.size), _h(desc), C.byref(res))
    return info, dict(sources=res.sources, batches=res.batches, levels=res.levels, reached=res.reached, loop_ms=res.loop_ms)


def cdlp(v, A, desc, init=None, directed=False, max_iter=10):
    """grb_cdlp: v = the communities of A's graph by synchronous label propagation (CDLP, as Graphalytics and LAGraph define
    it).  A is n x n, f32 or i32; its values are never read (stored zeros are edges) and its diagonal takes no part.  N(x)
    is a multiset: directed=False, the off-diagonal columns stored in row x of the CSR (an asymmetric A means "rows only",
    the symmetry is not checked); directed=True, those plus the off-diagonal rows stored in column x (from the CSC), so a
    vertex joined to x both ways counts twice.  L_0(x) = x, or init: an i32 vector of size n, either storage, all n values
    stored, each in 0 .. n - 1.  L_t+1(x) = the smallest of the most frequent labels in { L_t(u) : u in N(x) }, L_t(x) when
    N(x) is empty; iterations are synchronous and run until one changes nothing or max_iter have run.  v is an i32 vector
    of size n and becomes dense; v may be init; the same inputs give the same bits.  max_iter < 1 or nvals(init) != n ->
    GrB_INVALID_VALUE; an init value outside 0 .. n - 1 -> GrB_INVALID_INDEX; A not square or v / init not of size n ->
    GrB_DIMENSION_MISMATCH; v or init not i32 or A outside f32 / i32 -> GrB_NOT_IMPLEMENTED; directed=True on an A without
    its own CSC (a product result, the CSR-only format) -> GrB_INVALID_OBJECT (v unchanged on every error).  Returns (info,
    dict(iterations = those run, the one that changed nothing included, changed = labels the last one changed, evaluated =
    (vertex, iteration) pairs whose mode was computed: every vertex with neighbours in iteration 1, afterwards those with
    a neighbour that changed in the iteration before, communities = distinct labels in v, loop_ms))."""
    res = _lib.CdlpResult()
    info = _lib.load().grb_cdlp(_h(v), _h(A), _h(init), int(directed), int(max_iter), _h(desc), C.byref(res))
    return info, dict(iterations=res.iterations, changed=res.changed, evaluated=res.evaluated, communities=res.communities,
                      loop_ms=res.loop_ms)


def cdlp_set_skip(on=-1):
    """grb_cdlp_set_skip: 1 = an iteration of cdlp evaluates only the vertices with a neighbour whose label changed in the
    iteration before (default), 0 = every vertex with neighbours, every time (same labels; evaluated = iterations x that
    count); < 0 queries.  Returns the previous setting."""
    return int(_lib.load().grb_cdlp_set_skip(int(on)))


def lcc(v, A, desc, directed=False):
    """grb_lcc: v = the local clustering coefficient of every vertex of A's graph (LCC, as Graphalytics and LAGraph define
    it).  A is n x n, f32 or i32; its values are never read (stored zeros are edges) and its diagonal takes no part.  With
    E = the stored off-diagonal entries, N(x) = { u != x : (x, u) in E or (u, x) in E } is a SET (a vertex joined both ways
    is in it once; cdlp's N(x) is a multiset), d(x) = |N(x)|, num(x) = the number of stored entries (u, w), u != w, with both
    ends in N(x) -- directed entries -- and v[x] = num(x) / (d(x) (d(x) - 1)) when d(x) >= 2, else exactly 0; on a
    symmetric structure that is 2 tri(x) / (d (d - 1)).  directed=False: A's structure is symmetric and only the CSR is
    read; with a CSC of its own an asymmetric A -> GrB_INVALID_VALUE, without one (a product result, the CSR-only format)
    the caller vouches for it.  directed=True: any structure, CSR and CSC are read; an A without its own CSC ->
    GrB_INVALID_OBJECT.  v is an f32 vector of size n and becomes dense; num and d are exact integers, the quotient is f64
    rounded to f32 once; the same inputs give the same bits.  A not square or v not of size n -> GrB_DIMENSION_MISMATCH;
    v not f32 or A outside f32 / i32 -> GrB_NOT_IMPLEMENTED (v unchanged on every error).  Returns (info, dict(edges =
    unordered joined pairs, triangles of that undirected graph, closed = the sum of num, wedges = the sum of d (d - 1),
    max_degree, loop_ms))."""
    res = _lib.LccResult()
    info = _lib.load().grb_lcc(_h(v), _h(A), int(directed), _h(desc), C.byref(res))
    return info, dict(edges=res.edges, triangles=res.triangles, closed=res.closed, wedges=res.wedges,
                      max_degree=res.max_degree, loop_ms=res.loop_ms)


def _kcore_dict(res):
    return dict(edges=res.edges, result_edges=res.result_edges, kmax=res.kmax, levels=res.levels,
                result_vertices=res.result_vertices, rounds=res.rounds, launches=res.launches, loop_ms=res.loop_ms)


def coreness(v, A, desc):
    """grb_coreness: v = the core number of every vertex of A's graph.  A is n x n, f32 or i32, with the same structure as
    its transpose; its values are never read (stored zeros are edges) and its diagonal takes no part.  The k-core is the
    largest subgraph in which every vertex has at least k neighbours inside the subgraph, core(x) = the largest k such that
    x is in the k-core (0 for an isolated vertex) and kmax = max core(x) is the degeneracy.  v is an i32 vector of size n and
    becomes dense; the same inputs give the same bits.  The whole peel is one launch on the device.  Only the CSR is read:
    with a CSC of its own an asymmetric A -> GrB_INVALID_VALUE, without one (a product result, the CSR-only format) the
    caller vouches for it.  A null or unbuilt argument -> GrB_UNINITIALIZED_OBJECT; A not square or v not of size n ->
    GrB_DIMENSION_MISMATCH; v not i32 or A outside f32 / i32 -> GrB_NOT_IMPLEMENTED; a grid barrier that gave up ->
    GrB_PANIC (v unchanged on every error).  Returns (info, dict(edges, result_edges = edges inside the kmax-core, kmax,
    levels = distinct core numbers, result_vertices = vertices with core(x) == kmax, rounds = grid-wide passes of the
    device, launches, loop_ms))."""
    res = _lib.KcoreResult()
    info = _lib.load().grb_coreness(_h(v), _h(A), _h(desc), C.byref(res))
    return info, _kcore_dict(res)


def kcore(v, A, k, desc):
    """grb_kcore: v = the k-core of A's graph (A and the definition as for coreness): v[x] = the number of x's neighbours
    inside the k-core when x is in it (that is >= k), 0 when it is not; the vertex analogue of ktruss storing supports.
    k = 0 gives the plain degrees, k > kmax all zeros.  v is an i32 vector of size n and becomes dense; the same inputs give
    the same bits.  k < 0 -> GrB_INVALID_VALUE; the other error codes as for coreness (v unchanged on every error).
    Returns (info, dict(edges, result_edges = edges inside the k-core, kmax = k, levels = 1, result_vertices = vertices of
    the k-core, rounds, launches, loop_ms))."""
    res = _lib.KcoreResult()
    info = _lib.load().grb_kcore(_h(v), _h(A), int(k), _h(desc), C.byref(res))
    return info, _kcore_dict(res)


def scc(v, A, desc):
    """grb_scc: v = the strongly connected components of A's directed graph.  A is n x n, f32 or i32; its values are never
    read (stored zeros are edges) and its diagonal takes no part.  x and y are in one component when a directed path runs
    from x to y and one from y to x; v[x] = the smallest vertex number in x's component, so the same inputs give the same
    bits and A and its transpose give the same vector.  On a symmetric structure these are the connected components.  v is
    an i32 vector of size n and becomes dense; no descriptor field is read.  The whole computation (trimming, one
    forward-backward sweep from a pivot, colouring rounds) is one launch on the device.  The CSR and the CSC are both read:
    an A without a CSC of its own (a product result, the CSR-only format) -> GrB_INVALID_OBJECT.  A null or unbuilt
    argument -> GrB_UNINITIALIZED_OBJECT; A not square or v not of size n -> GrB_DIMENSION_MISMATCH; v not i32 or A outside
    f32 / i32 -> GrB_NOT_IMPLEMENTED; no device memory -> GrB_OUT_OF_MEMORY; a grid barrier that gave up -> GrB_PANIC (v
    unchanged on every error).  Returns (info, dict(edges = stored off-diagonal entries, components, largest = vertices of
    the largest component, trivial = components of one vertex, trimmed, rounds, passes = what the device ran, for the
    bench only, launches, loop_ms))."""
    res = _lib.SccResult()
    info = _lib.load().grb_scc(_h(v), _h(A), _h(desc), C.byref(res))
    return info, dict(edges=res.edges, components=res.components, largest=res.largest, trivial=res.trivial,
                      trimmed=res.trimmed, rounds=res.rounds, passes=res.passes, launches=res.launches, loop_ms=res.loop_ms)


def msf(Cm, comp, A, desc):
    """grb_msf: Cm = the minimum spanning forest of A's weighted undirected graph.  A is n x n, f32 or i32, symmetric in
    structure and in values; its diagonal takes no part, a stored zero is an edge of weight 0 and the weights ARE read.
    The edges are totally ordered by the key (w, min(u, v), max(u, v)), compared lexicographically -- i32 weights as signed
    integers, f32 weights by value with -0.0 and +0.0 the same weight and +-inf allowed -- and the forest is the one Kruskal
    builds when it takes the edges in key order, so it is unique and the same inputs give the same bits.  Cm is n x n of A's
    type and receives both directions of every forest edge with A's bits for it (columns ascending, empty rows for isolated
    vertices, CSC = a copy of the CSR unless Cm is CSR only); Cm may be A.  comp is None or an i32 vector of size n that
    becomes dense: comp[v] = the smallest vertex number in v's connected component.  No descriptor field is read.  The whole
    loop (Boruvka rounds) is one launch on the device.  Only the CSR is read: with a CSC of its own an A whose structure or
    values are not symmetric -> GrB_INVALID_VALUE, without one (a product result, the CSR-only format) the caller vouches for
    it and the call stays bounded.  A NaN off the diagonal -> GrB_INVALID_VALUE.  A null or unbuilt argument ->
    GrB_UNINITIALIZED_OBJECT; A not square, Cm not n x n or comp not of size n -> GrB_DIMENSION_MISMATCH; A outside f32 / i32 or
    comp not i32 -> GrB_NOT_IMPLEMENTED; Cm not of A's type -> GrB_DOMAIN_MISMATCH; no device memory -> GrB_OUT_OF_MEMORY; a
    grid barrier that gave up -> GrB_PANIC (Cm and comp unchanged on every error).  Returns (info, dict(edges, forest_edges =
    n - components, weight = the forest's weights summed in f64 in a fixed order (i32: the exact integer sum), components,
    isolated, rounds, passes = what the device ran, for the bench only, launches, loop_ms))."""
    res = _lib.MsfResult()
    info = _lib.load().grb_msf(_h(Cm), _h(comp), _h(A), _h(desc), C.byref(res))
    return info, dict(edges=res.edges, forest_edges=res.forest_edges, weight=res.weight, components=res.components,
                      isolated=res.isolated, rounds=res.rounds, passes=res.passes, launches=res.launches, loop_ms=res.loop_ms)


GRB_MATCH_HEAVIEST, GRB_MATCH_LIGHTEST, GRB_MATCH_HASHED = 0, 1, 2


def matching(mate, Cm, A, mode, seed, desc):
    """grb_matching: mate = the greedy matching of A's undirected graph.  A is n x n, f32 or i32, symmetric; its diagonal
    takes no part.  The edges are totally ordered by the key (p, min(u, v), max(u, v)), compared lexicographically, and the
    matching is the one the greedy scan builds: take the edges in key order and keep an edge when both ends are still free.
    It is unique and maximal, so the same inputs give the same bits.  mode selects p: GRB_MATCH_HEAVIEST = 0 orders by
    descending weight (i32 as signed integers; f32 by value with -0.0 and +0.0 the same weight and +-inf allowed; a stored
    zero or a negative weight is an edge like any other; its weight is at least half the maximum weight matching's when the
    weights are non-negative), GRB_MATCH_LIGHTEST = 1 the same ascending, GRB_MATCH_HASHED = 2 reads the structure only:
    p = mix(mix(min + seed) ^ max) in 32-bit unsigned arithmetic with mix(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13;
    x *= 0xc2b2ae35; x ^= x >> 16, the smaller p first; seed is ignored in the other modes.  mate is an i32 vector of size n
    that becomes dense: mate[v] = v's partner, or -1.  Cm is None or n x n of A's type and receives both directions of every
    matched edge, at most one entry a row, with A's bits from the row of min(u, v) (CSC = a copy of the CSR unless Cm is CSR
    only); Cm may be A.  No descriptor field is read.  The whole loop (locally dominant edges) is one launch on the device.
    Only the CSR is read: with a CSC of its own an A whose structure (in modes 0 and 1: or values) is not symmetric ->
    GrB_INVALID_VALUE, without one (a product result, the CSR-only format) the caller vouches for it and the call stays
    bounded.  A NaN off the diagonal in modes 0 and 1, or a mode outside 0..2 -> GrB_INVALID_VALUE.  A null or unbuilt
    argument -> GrB_UNINITIALIZED_OBJECT; A not square, mate not of size n or Cm not n x n -> GrB_DIMENSION_MISMATCH; A outside
    f32 / i32 or mate not i32 -> GrB_NOT_IMPLEMENTED; Cm not of A's type -> GrB_DOMAIN_MISMATCH; no device memory ->
    GrB_OUT_OF_MEMORY; a grid barrier that gave up -> GrB_PANIC (mate and Cm unchanged on every error).  Returns (info,
    dict(edges, matched = the edges of the matching, weight = the matched edges' stored values summed in f64 in a fixed order
    (i32: the exact integer sum), exposed = vertices with a neighbour but no partner, isolated, rounds, passes, evaluations =
    what the device ran, for the bench only, launches, loop_ms))."""
    res = _lib.MatchingResult()
    info = _lib.load().grb_matching(_h(mate), _h(Cm), _h(A), int(mode), int(seed) & 0xffffffff, _h(desc), C.byref(res))
    return info, dict(edges=res.edges, matched=res.matched, weight=res.weight, exposed=res.exposed, isolated=res.isolated,
                      rounds=res.rounds, passes=res.passes, evaluations=res.evaluations, launches=res.launches,
                      loop_ms=res.loop_ms)


GRB_RELABEL_LABELS, GRB_RELABEL_MATE = 0, 1


def relabel(map, labels, kind):
    """grb_relabel: map = the dense ranking of a label vector.  labels is an i32 vector of size n in either storage with all
    n values stored.  kind = GRB_RELABEL_LABELS (0): every value is in 0 .. n - 1 and L(v) = labels[v]; GRB_RELABEL_MATE (1):
    every value is in -1 .. n - 1 and L(v) = v when labels[v] < 0, otherwise min(v, labels[v]) -- what grb_matching writes,
    so a matched pair shares a label and an unmatched vertex keeps its own (the involution is not checked).  map is an i32
    vector of size n that becomes dense: map[v] = the number of distinct values of L smaller than L(v), so the coarse ids
    ascend with the labels; map may be labels.  Flags, the library's scan and a gather on the device; the same inputs give
    the same bits.  Errors are found before map is written: a null handle -> GrB_UNINITIALIZED_OBJECT; sizes differ ->
    GrB_DIMENSION_MISMATCH; not i32 -> GrB_NOT_IMPLEMENTED; nvals(labels) != n or kind outside {0, 1} -> GrB_INVALID_VALUE; a
    value out of range -> GrB_INVALID_INDEX.  Returns (info, count = the number of distinct values of L; 0 when n = 0)."""
    count = C.c_int32(0)
    info = _lib.load().grb_relabel(_h(map), _h(labels), int(kind), C.byref(count), None)
    return info, count.value


def contract(Cm, sizes, A, map, op, loops, desc):
    """grb_contract: Cm = S^T A S with S(v, map[v]) = 1, the quotient graph.  A is n x n, f32 or i32, any structure (only
    its CSR is read; stored zeros are entries).  map is an i32 vector of size n with all n values stored, each in
    -1 .. nc - 1 where Cm is nc x nc: -1 drops the vertex with every entry of its row and column, anything else out of range
    -> GrB_INVALID_INDEX.  A raw label vector works with an n x n Cm (unused labels leave empty rows), a relabel() result with
    an nc x nc Cm.  loops = 0 drops every entry with map[i] = map[j] (condensation, coarsening), 1 keeps them (community
    graph).  Cm(a, b) is stored exactly when some stored A(i, j) has map[i] = a, map[j] = b and survives loops; columns
    ascend; its value is the fold of the contributing entries under op, a binary operator by name or number: "plus" (i32
    wraps; f32 adds in f64 in an order fixed by the inputs alone and rounds once, no floating-point atomics), "minimum" /
    "maximum" (i32 signed; f32 in the total order -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN, the winner's bits
    copied), "first" (the bits of the contributing entry with the smallest (i, j)); any other -> GrB_NOT_IMPLEMENTED.  Cm is
    of A's type (else GrB_DOMAIN_MISMATCH) and gets its CSR and, unless it is CSR only, a CSC that is the transpose of that
    CSR; Cm may be A when nc = n.  sizes is None or an i32 vector of size nc that becomes dense: sizes[a] = the vertices
    mapped to a.  No descriptor field is read.  A null or unbuilt argument -> GrB_UNINITIALIZED_OBJECT; A or Cm not square,
    map not of size n or sizes not of size nc -> GrB_DIMENSION_MISMATCH; A outside f32 / i32, map or sizes not i32 ->
    GrB_NOT_IMPLEMENTED; loops outside {0, 1} or nvals(map) != n -> GrB_INVALID_VALUE; no device memory -> GrB_OUT_OF_MEMORY
    (Cm and sizes unchanged on every error).  Returns (info, dict(kept = entries of A with both ends kept, loops = those with
    map[i] = map[j] whatever the flag, entries = nvals(Cm), clusters = non-empty clusters, dropped = vertices with map -1,
    largest = the largest cluster, launches, loop_ms))."""
    res = _lib.ContractResult()
    opn = op if isinstance(op, int) else BINARY_OPS.index(op)
    info = _lib.load().grb_contract(_h(Cm), _h(sizes), _h(A), _h(map), int(opn), int(loops), _h(desc), C.byref(res))
    return info, dict(kept=res.kept, loops=res.loops, entries=res.entries, clusters=res.clusters, dropped=res.dropped,
                      largest=res.largest, launches=res.launches, loop_ms=res.loop_ms)


def louvain(labels, A, weighted, max_levels, max_rounds, desc):
    """grb_louvain: labels = the communities of A's undirected graph by Louvain modularity optimisation, deterministic and in
    exact integers.  A is n x n, f32 or i32, symmetric in structure and values.  weighted = 1 reads the values: i32 >= 0, f32
    a non-negative integer value <= 2^24 with -0.0 = +0.0 (negative, fractional, NaN, inf -> GrB_INVALID_VALUE); weighted = 0
    never reads them, every stored entry weighs 1.  A stored zero is an entry of weight 0, a diagonal entry a loop.  W = the
    sum of all stored weights, each entry once as stored, must be <= 2^31 - 1.  For a partition c, in(x) = the stored weight
    inside community x, tot(x) = the sum of the row sums k(v) of its members, QN = W * sum in(x) - sum tot(x)^2 and
    Q = QN / W^2; QN is invariant under contraction with loops kept.  A level starts from c(v) = v and runs rounds: every
    vertex with an off-diagonal entry proposes the neighbouring community with the largest gain
    W e(v, x) - k(v) tot(x) - stay, the smallest x on a tie, only if the gain is > 0; every proposal claims its source and its
    destination, a community's winner is the claimant with the largest gain, the smallest v on a tie; (v -> d, g) is accepted
    iff v wins c(v), and v wins d or d's winner itself enters d and g > k(v) (K(d) - k(v)) with K(d) the k of all proposers
    to d; all accepted moves are applied at once.  Every accepted round strictly increases QN.  A round without proposals
    ends the level (it counts in rounds), and so does max_rounds.  Between levels the graph is contracted (grb_relabel, then
    grb_contract with PLUS and loops kept); the call stops after the first level that accepted no move (it counts in levels)
    or after max_levels.  labels is an i32 vector of size n that becomes dense: labels[v] = the smallest original vertex
    number in v's final community, as in cc, scc and msf.  No descriptor field is read.  A level is one launch on the device;
    every vertex is evaluated in every round, and a path is the worst case (equal gains serialise on the smallest-v tie).
    Only the CSR is read: with a CSC of its own an A whose structure (with weighted = 1: or values) is not symmetric ->
    GrB_INVALID_VALUE, without one (a product result, the CSR-only format) the caller vouches for it and the call stays
    bounded.  A bad weight, W > 2^31 - 1, weighted outside {0, 1}, max_levels < 1 or max_rounds < 1 -> GrB_INVALID_VALUE.  A
    null or unbuilt argument -> GrB_UNINITIALIZED_OBJECT; A not square or labels not of size n -> GrB_DIMENSION_MISMATCH; A
    outside f32 / i32 or labels not i32 -> GrB_NOT_IMPLEMENTED; a built A with entries but no CSR on the device ->
    GrB_INVALID_OBJECT; no device memory -> GrB_OUT_OF_MEMORY; a grid barrier that gave up -> GrB_PANIC (labels unchanged on every error).  n = 0, an A without entries or W = 0 is a success with
    labels[v] = v, levels = rounds = 1 and qn = 0.  Returns (info, dict(levels, rounds, moves = accepted proposals,
    proposals, communities, qn, w, modularity = float(qn) / (float(w) * float(w)) or 0 -- all exact and the same on any number
    of CUs --, passes, launches = one a level, loop_ms))."""
    res = _lib.LouvainResult()
    info = _lib.load().grb_louvain(_h(labels), _h(A), int(weighted), int(max_levels), int(max_rounds), _h(desc), C.byref(res))
    return info, dict(levels=res.levels, rounds=res.rounds, moves=res.moves, proposals=res.proposals,
                      communities=res.communities, qn=res.qn, w=res.w, modularity=res.modularity, passes=res.passes,
                      launches=res.launches, loop_ms=res.loop_ms)


GRB_WALK_UNIFORM, GRB_WALK_WEIGHTED = 0, 1


def random_walk(walks, A, starts, length, mode, seed, desc):
    """grb_random_walk: walks = random walks on A's graph from the vertices in starts, counter-based: every draw is a pure
    function of (seed, walker, step), so the same inputs give the same bits on any number of CUs.  All arithmetic of the
    draw is unsigned 32-bit and wraps: mix(x): x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16;
    draw(seed, a, b) = mix(mix(mix((seed + 0x9e3779b9) ^ a) + b) ^ seed); pick(r, m) = (uint64(r) * uint64(m)) >> 32, a
    number in 0 .. m - 1.  A is n x n, f32 or i32, directed or not; a stored A(i, j) is the step i -> j, a diagonal entry an
    ordinary step; only the CSR is read (a product result and the CSR-only format work).  starts: vertex ids (duplicates
    are different walkers), or None for every vertex 0 .. n - 1 in order; ns = their number.  length >= 0 is the number of
    steps.  walks is an i32 vector of size ns * (length + 1) that becomes dense, walker-major:
    walks[w * (length + 1) + t] = walker w's vertex after t steps, walks[w * (length + 1)] = starts[w].  Step t (from 0) of
    walker w at vertex v, with r = draw(seed, w, t): mode = GRB_WALK_UNIFORM = 0 never reads the values: with d = the stored
    entries of row v, the next vertex is the column of entry pick(r, d) of the row in stored order.  mode =
    GRB_WALK_WEIGHTED = 1 reads the values under louvain's rule: i32 >= 0, f32 a non-negative integer value <= 2^24 with
    -0.0 = +0.0 (negative, fractional, NaN, inf -> GrB_INVALID_VALUE); S(v) = the row's sum must be <= 2^31 - 1 for every
    row, else GrB_INVALID_VALUE; the next vertex is the column of the first entry whose inclusive prefix sum in stored order
    exceeds pick(r, S(v)); an entry of weight 0 is never taken.  A dead end is a row with d = 0, or in weighted mode
    S(v) = 0: the walk stops there, and every later position of that walker is -1.  No descriptor field is read.  A null or
    unbuilt argument -> GrB_UNINITIALIZED_OBJECT; A not square or size(walks) != ns * (length + 1) ->
    GrB_DIMENSION_MISMATCH; a start outside 0 .. n - 1 -> GrB_INVALID_INDEX; length < 0, a mode outside {0, 1}, a bad weight
    or row sum, or ns * (length + 1) > INT32_MAX -> GrB_INVALID_VALUE; walks not i32 or A outside f32 / i32 ->
    GrB_NOT_IMPLEMENTED; a built A with entries but no CSR on the device -> GrB_INVALID_OBJECT; no device memory ->
    GrB_OUT_OF_MEMORY (walks unchanged on every error).  ns = 0 is a success with nothing written.  Out of scope:
    second-order (node2vec) walks and restarts.  Returns (info, dict(walkers = ns, steps = transitions made, summed over the
    walkers, dead_ends = walkers that stopped early -- exact and the same on any number of CUs --, launches, loop_ms))."""
    res = _lib.WalkResult()
    if starts is None:
        info = _lib.load().grb_random_walk(_h(walks), _h(A), None, 0, int(length), int(mode), int(seed) & 0xffffffff, _h(desc), C.byref(res))
    else:
        src = np.ascontiguousarray(starts, dtype=np.int32).ravel()
        buf = src if src.size else np.zeros(1, np.int32)   # an empty list is no walkers, not "every vertex"
        info = _lib.load().grb_random_walk(_h(walks), _h(A), buf.ctypes.data, int(src.size), int(length), int(mode),
                                           int(seed) & 0xffffffff, _h(desc), C.byref(res))
    return info, dict(walkers=res.walkers, steps=res.steps, dead_ends=res.dead_ends, launches=res.launches, loop_ms=res.loop_ms)


_byref = C.byref


def sample_neighbors(C, A, seeds, fanout, seed, desc):  # noqa: N803  (C is the result here; ctypes is _byref below)
    """grb_sample_neighbors: C = a fan-out-limited sample of the rows of A named by seeds, uniform without replacement, with
    random_walk's counter-based draw(seed, a, b) (its docstring has the arithmetic).  A is nrows x ncols (rectangular is
    fine), f32 or i32; only the CSR is read.  seeds: row numbers in any order, duplicates allowed; ns = their number.  C is
    ns x ncols, of A's type.  Row k of C is drawn from row seeds[k] of A, with d its length: if d <= fanout the whole row,
    otherwise the fanout entries with the smallest draw(seed, k, p), p = 0 .. d - 1 the entry's position in the row.  The
    key takes the list position k, not the vertex: a seed listed twice is sampled twice, independently.  The kept entries
    stay in A's stored order (the columns ascend) and carry A's value bits unchanged: stored zeros, -0.0 and NaN are copied,
    nothing is read as a number.  C gets a CSC by the transposition behind transpose where its format keeps one; C may be
    A.  No descriptor field is read.  A null or unbuilt argument -> GrB_UNINITIALIZED_OBJECT; C not ns x ncols ->
    GrB_DIMENSION_MISMATCH; a seed outside 0 .. nrows - 1 -> GrB_INDEX_OUT_OF_BOUNDS; fanout < 1 -> GrB_INVALID_VALUE; the
    types of A and C not both f32 or both i32 -> GrB_NOT_IMPLEMENTED; a built A with entries but no CSR on the device ->
    GrB_INVALID_OBJECT; more than INT32_MAX entries or no device memory -> GrB_OUT_OF_MEMORY (C unchanged on every error).
    ns = 0 gives an empty 0 x ncols C.  Out of scope: weighted sampling without replacement, sampling with replacement,
    the multi-hop loop (sample, take C's columns as the next seeds, sample again).  Returns (info, dict(rows = ns,
    entries = nvals(C), full_rows = rows copied whole -- exact and the same on any number of CUs --, launches, loop_ms))."""
    res = _lib.SampleResult()
    src = np.ascontiguousarray(seeds if seeds is not None else [], dtype=np.int32).ravel()
    buf = src if src.size else np.zeros(1, np.int32)
    info = _lib.load().grb_sample_neighbors(_h(C), _h(A), buf.ctypes.data, int(src.size), int(fanout), int(seed) & 0xffffffff,
                                            _h(desc), _byref(res))
    return info, dict(rows=res.rows, entries=res.entries, full_rows=res.full_rows, launches=res.launches, loop_ms=res.loop_ms)


GRB_FLOW_CAPACITY, GRB_FLOW_UNIT = 0, 1


def maxflow(F, side, A, source, sink, mode, desc):
    """grb_maxflow: the maximum flow from source to sink and its minimum cut.  A is n x n, f32 or i32, directed: A(i, j) is
    the capacity of the arc i -> j; no symmetry is asked for, diagonal entries take no part, antiparallel arcs are two arcs
    and a stored 0 is an arc of capacity 0.  mode = GRB_FLOW_CAPACITY = 0 reads the values: i32 must be >= 0, f32 an integer
    value in 0 .. 2^24 (anything else off the diagonal -- negative, fractional, NaN, +-inf, above 2^24 -> GrB_INVALID_VALUE);
    GRB_FLOW_UNIT = 1 gives every stored off-diagonal entry capacity 1 and never reads the values (a NaN is fine).  The
    arithmetic is exact: 32-bit residual capacities, 64-bit integer excesses and value, no floating-point atomics.  side is
    None or an i32 vector of size n that becomes dense: side[v] = 1 when sink can be reached from v in the residual graph of a
    maximum flow -- the smallest sink side of any minimum cut, unique; side[sink] = 1, side[source] = 0, and the arcs from
    side 0 to side 1 are a minimum cut whose capacities sum to value.  F is None or n x n of A's type and receives a maximum
    flow in cancelled form: entries only where A has one off the diagonal and the flow is positive, 0 < F(i, j) <= capacity,
    never both F(i, j) and F(j, i), columns ascending, the CSC by transposition unless F is CSR only; F may be A.  F is a valid
    maximum flow (capacity, conservation at every vertex but the terminals) and the same inputs give the same bits; with F
    None the preflow is not converted to a flow.  No descriptor field is read.  Synchronous push-relabel with global
    relabeling as one launch on the device; A's CSC is read for the reverse arcs.  A null or unbuilt A ->
    GrB_UNINITIALIZED_OBJECT; A not square, F not n x n or side not of size n -> GrB_DIMENSION_MISMATCH; source or sink outside
    0 .. n - 1 -> GrB_INDEX_OUT_OF_BOUNDS; source == sink, a mode outside 0..1 or a bad capacity -> GrB_INVALID_VALUE; A outside
    f32 / i32 or side not i32 -> GrB_NOT_IMPLEMENTED; F not of A's type -> GrB_DOMAIN_MISMATCH; an A without a CSC of its own ->
    GrB_INVALID_OBJECT; too many residual arcs or no device memory -> GrB_OUT_OF_MEMORY; a grid barrier that gave up ->
    GrB_PANIC (F and side unchanged on every error).  Returns (info, dict(value, arcs = stored off-diagonal entries of A,
    flow_arcs = nvals(F) or -1, sink_side = vertices with side 1, cut_arcs, cut_capacity = the cut's capacities summed after
    the loop, always equal to value, rounds, global_relabels, passes = what the device ran, for the bench only, launches,
    loop_ms))."""
    res = _lib.MaxflowResult()
    info = _lib.load().grb_maxflow(_h(F), _h(side), _h(A), int(source), int(sink), int(mode), _h(desc), C.byref(res))
    return info, dict(value=res.value, arcs=res.arcs, flow_arcs=res.flow_arcs, sink_side=res.sink_side, cut_arcs=res.cut_arcs,
                      cut_capacity=res.cut_capacity, rounds=res.rounds, global_relabels=res.global_relabels, passes=res.passes,
                      launches=res.launches, loop_ms=res.loop_ms)


GRB_BCC_BLOCKS, GRB_BCC_BRIDGES = 0, 1


def bcc(Cm, art, A, mode, desc):
    """grb_bcc: the biconnected components (blocks), articulation points and bridges of A's undirected graph.  A is n x n,
    f32 or i32, symmetric in structure; its values are never read (a stored zero is an edge) and its diagonal takes no part.
    A block is a class of "two edges lie on a common simple cycle, or are equal", a bridge a block of one edge; every edge is
    in exactly one block.  The blocks are numbered 0 .. blocks-1 in ascending order of their smallest edge key
    (min(u, v), max(u, v)), compared lexicographically, so the numbering is unique and the same inputs give the same bits.
    Cm is None or n x n and i32 whatever A's type: with mode = GRB_BCC_BLOCKS = 0 it receives A's off-diagonal structure,
    both directions, each entry's value the block number of that edge; with GRB_BCC_BRIDGES = 1 only the entries whose block
    is a single edge, with the same numbers (columns ascending, empty rows for isolated vertices, CSC = a copy of the CSR
    unless Cm is CSR only); Cm may be A when A is i32.  art is None or an i32 vector of size n that becomes dense: art[v] = the
    number of blocks that contain v, 0 without an off-diagonal entry, >= 2 exactly at the articulation points.
    Both may be None: only the record is filled.  No descriptor field is read.  Tarjan-Vishkin on a BFS forest as one launch on the
    device; the passes grow with the BFS depth.  Only the CSR is read: with a CSC of its own an A whose structure is not
    symmetric -> GrB_INVALID_VALUE, without one (a product result, the CSR-only format) the caller vouches for it and the
    call stays bounded.  A mode outside {0, 1} -> GrB_INVALID_VALUE.  A null or unbuilt A -> GrB_UNINITIALIZED_OBJECT; A not
    square, Cm not n x n or art not of size n -> GrB_DIMENSION_MISMATCH; A outside f32 / i32 or art not i32 ->
    GrB_NOT_IMPLEMENTED; Cm not i32 -> GrB_DOMAIN_MISMATCH; no device memory -> GrB_OUT_OF_MEMORY; a grid barrier that gave up
    -> GrB_PANIC (Cm and art unchanged on every error).  Returns (info, dict(edges, largest = edges of the largest block,
    blocks, bridges, articulation = vertices with art >= 2, components, isolated, levels = depth of the BFS forest + 1,
    rounds, passes = what the device ran, for the bench only, launches, loop_ms))."""
    res = _lib.BccResult()
    info = _lib.load().grb_bcc(_h(Cm), _h(art), _h(A), int(mode), _h(desc), C.byref(res))
    return info, dict(edges=res.edges, largest=res.largest, blocks=res.blocks, bridges=res.bridges,
                      articulation=res.articulation, components=res.components, isolated=res.isolated, levels=res.levels,
                      rounds=res.rounds, passes=res.passes, launches=res.launches, loop_ms=res.loop_ms)


def tc_set_product(on):
    """grb_tc_set_product: 0 = grb_tc counts without the product where that is a count and pays (default), 1 = always the
    product in B, 2 = the count wherever it is a count; < 0 queries."""
    return _lib.load().grb_tc_set_product(int(on))


def tc_release(A):
    """grb_tc_release: drops the orientation the matrix keeps after its first count."""
    return _lib.load().grb_tc_release(_h(A))


def tc_last():
    """grb_tc_last: which way the last tc went and what it cost."""
    t = _lib.TcInfo()
    info = _lib.load().grb_tc_last(C.byref(t))
    return info, dict(path=t.path, prep_ms=t.prep_ms, count_ms=t.count_ms, longest_list=t.longest_list, tasks=list(t.tasks))


def tc_dense_core(L, k_want, method=0, dense_from=0):
    """grb_tc_dense_core: the product C<L> = L (+.x) L^T restricted to the k_want longest rows of L, as K x K bit rows.
    method 0 popcount, 1 MFMA (v_mfma_i32_16x16x64_i8), 2 MFMA for tiles of >= dense_from mask entries.  Returns (info, dict)."""
    res = _lib.TcCoreResult()
    info = _lib.load().grb_tc_dense_core(_h(L), int(k_want), int(method), int(dense_from), C.byref(res))
    return info, dict(core_rows=res.core_rows, min_row_length=res.min_row_length, core_entries=res.core_entries, count=res.count,
                      checksum=res.checksum, build_ms=res.build_ms, product_ms=res.product_ms, tiles=res.tiles,
                      tiles_mfma=res.tiles_mfma, tiles_by_density=list(res.tiles_by_density))


def traceMxmTranspose(op, A, B, desc):
    out = C.c_double(0)
    info = _lib.load().grb_trace_mxm_transpose(C.byref(out), _semiring_id(op), _h(A), _h(B), _h(desc))
    return info, out.value


def scatter(w, mask, u, val, desc):
    return _lib.load().grb_scatter(_h(w), _h(mask), _h(u), float(val), _h(desc))


def graph_color(w, A, desc):
    n = C.c_int(0)
    info = _lib.load().grb_graph_color(_h(w), _h(A), _h(desc), C.byref(n))
    return info, n.value


def mis(v, A, seed, desc, weights=None):
    """algorithm::mis; `weights` (an int Vector) replaces the host-drawn srand(seed)/rand() vector."""
    res = AlgoResult()
    info = _lib.load().grb_mis(_h(v), _h(A), int(seed), _h(weights), _h(desc), C.byref(res))
    return info, dict(iterations=res.iterations, tight_ms=res.tight_ms)


def gc(v, A, seed, max_colors, algo, desc, weights=None):
    """algorithm::gcJP (algo 0) / gcMIS (1) / gcIS (2)."""
    res = AlgoResult()
    info = _lib.load().grb_gc(_h(v), _h(A), int(seed), _h(weights), int(max_colors), int(algo), _h(desc),
                              C.byref(res))
    return info, dict(iterations=res.iterations, tight_ms=res.tight_ms, succ=res.last_value)


def lgc(p, A, s, alpha, eps, desc):
    res = AlgoResult()
    info = _lib.load().grb_lgc(_h(p), _h(A), int(s), float(alpha), float(eps), _h(desc), C.byref(res))
    return info, dict(iterations=res.iterations, tight_ms=res.tight_ms, succ=res.last_value)


def diameter(v, A, s_start, s_end, desc):
    dmax, dind = C.c_int(0), C.c_int(-1)
    info = _lib.load().grb_diameter(_h(v), _h(A), int(s_start), int(s_end), _h(desc), C.byref(dmax), C.byref(dind))
    return info, dmax.value, dind.value


# ---- raw kernels / timing -----------------------------------------------------------
def k_spmv(A, tran, op, d_u, d_mask, scmp, accum, d_w):
    return _lib.load().grb_k_spmv(_h(A), int(tran), _semiring_id(op), d_u, d_mask, int(scmp), int(accum), d_w)


def sssp_set_nearfar(mode=-2):
    """-1 auto (default), 0 synchronous rounds only, 1 near / far whenever eligible; -2 queries (grb_sssp_set_nearfar)."""
    return int(_lib.load().grb_sssp_set_nearfar(int(mode)))


def sssp_last_work():
    """(vertices expanded, out-edges relaxed, vertices marked) over all passes of the last near / far sssp()"""
    out = (C.c_int64 * 3)()
    _lib.load().grb_sssp_last_work(out)
    return tuple(int(x) for x in out)


def sssp_last_order():
    """0: the last sssp() ran the reference's synchronous rounds; else the passes of the near / far order."""
    return int(_lib.load().grb_sssp_last_order())


def spmv_set_bands(k=0):
    """LDS prefixes SpMV plans prepared from now on may use (grb_spmv_set_bands); 0 only queries."""
    return int(_lib.load().grb_spmv_set_bands(int(k)))


def spmv_plan_info(A, tran=0, warm=False):
    """{"bands", "band_nnz", "pieces", "nhot"} of the SpMV plan of this orientation (grb_spmv_plan_info)."""
    bands, nhot = C.c_int(0), C.c_int(0)
    bn, pc = C.c_int64(0), C.c_int64(0)
    _lib.call("grb_spmv_plan_info", _h(A), int(bool(tran)), int(bool(warm)), C.byref(bands), C.byref(bn), C.byref(pc),
              C.byref(nhot))
    return {"bands": bands.value, "band_nnz": bn.value, "pieces": pc.value, "nhot": nhot.value}


def cc_set_fused(on=-1):
    """1: FastSV's element-wise tail in one launch (default); 0: the reference's call sequence; < 0 queries"""
    return int(_lib.load().grb_cc_set_fused(int(on)))


def spmv_set_format(fmt=-1):
    """matrix format of the generic SpMV (grb_spmv_set_format): 0 CSR only, 1 auto, 2 column-sorted bands wherever
    the monoid allows; < 0 only queries"""
    return int(_lib.load().grb_spmv_set_format(int(fmt)))


def set_lazy(on=-1):
    """the queue of element-wise calls (grb_set_lazy): 1 queue and fuse (default), 0 run every call at once; < 0 queries.
    Returns the previous setting."""
    return int(_lib.load().grb_set_lazy(int(on)))


def lazy_pending():
    """element-wise calls waiting in the queue (grb_lazy_pending; does not flush)"""
    return int(_lib.load().grb_lazy_pending())


def lazy_fused_reductions():
    """reductions that ran inside a chain's launch so far (grb_lazy_fused_reductions)"""
    return int(_lib.load().grb_lazy_fused_reductions())


def spmv_set_reuse_threshold(launches=-1):
    """CSR-kernel products after which `auto` prepares the column-sorted format for an orientation
    (grb_spmv_set_reuse_threshold; 0 = at once); < 0 only queries.  Returns the previous value."""
    return int(_lib.load().grb_spmv_set_reuse_threshold(int(launches)))


def spmv_format_info(A, tran=0):
    """the column-sorted copy of this orientation, if prepared (grb_spmv_format_info)"""
    used, bands, items, hub, iso = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    groups, nbytes = C.c_int64(0), C.c_int64(0)
    _lib.call("grb_spmv_format_info", _h(A), int(bool(tran)), C.byref(used), C.byref(groups), C.byref(bands),
              C.byref(items), C.byref(hub), C.byref(iso), C.byref(nbytes))
    return {"in_use": used.value, "groups": groups.value, "bands": bands.value, "items": items.value,
            "hub_rows": hub.value, "iso": iso.value, "bytes_per_launch": nbytes.value}


def k_spmv_bytes(A, tran):
    return int(_lib.load().grb_k_spmv_bytes(_h(A), int(tran)))


def timer_start():
    _lib.call("grb_timer_start")


def timer_stop():
    out = C.c_float(0)
    _lib.call("grb_timer_stop", C.byref(out))
    return out.value


def set_stream(ptr):
    _lib.call("grb_set_stream", ptr)


def device_info():
    buf = C.create_string_buffer(256)
    _lib.call("grb_device_info", buf, 256)
    return buf.value.decode()
