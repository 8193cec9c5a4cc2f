/*
 * grb_hip.h -- C ABI of libgrb_hip.so, the MI355X (gfx950) backend for the
 * GraphBLAST mxv/vxm hot path.
 *
 * The reference (gunrock/graphblast) has no FFI: its boundary is the C++ template
 * frontend `graphblas::{Vector,Matrix,Descriptor}` + the free functions of
 * graphblas/operations.hpp.  This header is that frontend flattened to C: one
 * opaque handle per frontend class, one entry point per frontend method/operation
 * on the path, enums in place of the functor template arguments.  Every entry point
 * cites the reference interface it replaces.  All functions return a grb_info
 * whose values are `graphblas::Info` (graphblas/types.hpp:28-42); nothing calls
 * exit().  Plain pointers and sizes only; no C++ or torch types.
 *
 * One process drives one GPU (hipSetDevice is the caller's business); all work is
 * enqueued on the stream set with grb_set_stream (default: the null stream).
 * Host-visible results (nvals, reduce, extractTuples) synchronise that stream, as
 * the reference's API does.
 */
#ifndef GRB_HIP_H_
#define GRB_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t grb_index;                 /* graphblas::Index, types.hpp:18 */
typedef int grb_info;                      /* graphblas::Info,  types.hpp:28-42 */

enum {
  GRB_SUCCESS = 0, GRB_UNINITIALIZED_OBJECT, GRB_NULL_POINTER, GRB_INVALID_VALUE,
  GRB_INVALID_INDEX, GRB_DOMAIN_MISMATCH, GRB_DIMENSION_MISMATCH, GRB_OUTPUT_NOT_EMPTY,
  GRB_NO_VALUE, GRB_NOT_IMPLEMENTED, GRB_OUT_OF_MEMORY, GRB_INSUFFICIENT_SPACE,
  GRB_INVALID_OBJECT, GRB_INDEX_OUT_OF_BOUNDS, GRB_PANIC
};

/* graphblas::Storage, types.hpp:21-23 */
enum { GRB_UNKNOWN = 0, GRB_SPARSE = 1, GRB_DENSE = 2 };

/* graphblas::Desc_field, types.hpp:44-55 */
enum { GRB_MASK = 0, GRB_OUTP, GRB_INP0, GRB_INP1, GRB_MODE, GRB_TA, GRB_TB, GRB_NT,
       GRB_MXVMODE, GRB_TOL, GRB_BACKEND, GRB_NDESCFIELD };

/* graphblas::Desc_value, types.hpp:57-78 (GRB_HIP takes the slot of GrB_CUDA) */
enum { GRB_SCMP = 0, GRB_REPLACE = 1, GRB_TRAN = 2, GRB_DEFAULT = 3, GRB_FIXEDROW = 6,
       GRB_PUSHPULL = 10, GRB_PUSHONLY = 11, GRB_PULLONLY = 12, GRB_SEQUENTIAL = 13,
       GRB_HIP = 14 };

/* Element type of a Vector<T> / Matrix<T>.  The reference instantiates float
 * (BFS/SSSP/PR) and int (CC/TC). */
typedef enum { GRB_F32 = 0, GRB_I32 = 1 } grb_dtype;

/* Additive monoids, graphblas/stddef.hpp:159-172 (same order). */
typedef enum {
  GRB_PLUS_MONOID = 0, GRB_MULTIPLIES_MONOID, GRB_MINIMUM_MONOID, GRB_MAXIMUM_MONOID,
  GRB_LOGICAL_OR_MONOID, GRB_LOGICAL_AND_MONOID, GRB_GREATER_MONOID,
  GRB_CUSTOM_LESS_MONOID, GRB_NOT_EQUAL_TO_MONOID, GRB_N_MONOIDS
} grb_monoid;

/* Semirings, graphblas/stddef.hpp:195-213 (same order). */
typedef enum {
  GRB_LOGICAL_OR_AND = 0, GRB_PLUS_MULTIPLIES, GRB_MINIMUM_PLUS, GRB_MAXIMUM_MULTIPLIES,
  GRB_PLUS_DIVIDES, GRB_PLUS_GREATER, GRB_GREATER_PLUS, GRB_PLUS_MINUS, GRB_PLUS_LESS,
  GRB_CUSTOM_LESS_PLUS, GRB_MINIMUM_MULTIPLIES, GRB_MULTIPLIES_MULTIPLIES,
  GRB_NOT_EQUAL_TO_PLUS, GRB_MINIMUM_SELECT_SECOND, GRB_PLUS_NOT_EQUAL_TO,
  GRB_CUSTOM_LESS_LESS, GRB_MINIMUM_NOT_EQUAL_TO, GRB_N_SEMIRINGS
} grb_semiring;

/* Binary operators, in the order graphblas/stddef.hpp:14-138 defines its functor templates
 * (logical_or ... divides; select_second == second). */
typedef enum {
  GRB_OP_LOGICAL_OR = 0, GRB_OP_LOGICAL_AND, GRB_OP_LOGICAL_XOR, GRB_OP_EQUAL, GRB_OP_NOT_EQUAL_TO,
  GRB_OP_GREATER, GRB_OP_LESS, GRB_OP_GREATER_EQUAL, GRB_OP_LESS_EQUAL, GRB_OP_FIRST, GRB_OP_SECOND,
  GRB_OP_MINIMUM, GRB_OP_MAXIMUM, GRB_OP_PLUS, GRB_OP_MINUS, GRB_OP_MULTIPLIES, GRB_OP_DIVIDES, GRB_N_BINARY_OPS
} grb_binary_op;

/* Unary operators of the device-side apply (the reference declares apply and implements it as a HOST loop under
 * GrB_BACKEND = GrB_SEQUENTIAL only, backend/cuda/apply.hpp:34-42,102-111; its own callers pass stateful random
 * functors that only a host loop in index order can serve).  BIND_FIRST / BIND_SECOND make a unary operator of any
 * grb_binary_op and a scalar: x -> op(scalar, x) / x -> op(x, scalar). */
typedef enum {
  GRB_UNARY_IDENTITY = 0, GRB_UNARY_AINV /* -x */, GRB_UNARY_MINV /* 1 / x */, GRB_UNARY_ABS, GRB_UNARY_LNOT /* !x */,
  GRB_UNARY_BIND_FIRST, GRB_UNARY_BIND_SECOND, GRB_N_UNARY_OPS
} grb_unary_op;

/* Predicates of select (GraphBLAS C API 2.0, GrB_select with the predefined index-unary operators).  i, j: the row and
 * column of the entry in op(A) (a vector is an n x 1 matrix: j = 0), a: its value, k: the thunk.
 *   TRIL j <= i + k   TRIU j >= i + k   DIAG j == i + k   OFFDIAG j != i + k
 *   ROWLE i <= k   ROWGT i > k   COLLE j <= k   COLGT j > k
 *   VALUEEQ a == k   VALUENE a != k   VALUELT a < k   VALUELE a <= k   VALUEGT a > k   VALUEGE a >= k
 * GRB_SEL_VALUENE with thunk 0 is "drop stored zeros". */
typedef enum {
  GRB_SEL_TRIL = 0, GRB_SEL_TRIU, GRB_SEL_DIAG, GRB_SEL_OFFDIAG, GRB_SEL_ROWLE, GRB_SEL_ROWGT, GRB_SEL_COLLE, GRB_SEL_COLGT,
  GRB_SEL_VALUEEQ, GRB_SEL_VALUENE, GRB_SEL_VALUELT, GRB_SEL_VALUELE, GRB_SEL_VALUEGT, GRB_SEL_VALUEGE, GRB_N_SELECT_OPS
} grb_select_op;

/* `accum` argument: the reference only tests its presence
 * (typeid(accum).name().size() > 1, backend/cuda/spmv.hpp:34-40). */
typedef enum { GRB_ACCUM_NULL = 0, GRB_ACCUM_PRESENT = 1 } grb_accum;

/* Semirings an application registers itself -- REGISTER_SEMIRING(SR, ADD_MONOID, MULT_BINARYOP) over
 * REGISTER_MONOID(M, BINARYOP, IDENTITY), graphblas/stddef.hpp:140-191: *id (>= 64) is accepted wherever a
 * grb_semiring is.  A composition that is one of the 17 above runs their compiled kernels; any other runs the
 * same kernels with the operators selected at run time. */
grb_info grb_semiring_register(int add_op /* grb_binary_op */, double add_identity, int mul_op /* grb_binary_op */,
                               int* id);

typedef struct grb_vector_s*     grb_vector;      /* graphblas::Vector<T>   vector.hpp:12-66 */
typedef struct grb_matrix_s*     grb_matrix;      /* graphblas::Matrix<T>   matrix.hpp:13-84 */
typedef struct grb_descriptor_s* grb_descriptor;  /* graphblas::Descriptor  descriptor.hpp:17-39 */

/* ---- library ----------------------------------------------------------------- */
/* Stream for all subsequent work (a hipStream_t cast to void*; NULL = null stream). */
grb_info grb_set_stream(void* hip_stream);
/* "gfx950:<CU count>:<device name>" of the current device, for logs. */
grb_info grb_device_info(char* buf, size_t buflen);
const char* grb_version(void);
/* HIP-event stopwatch on the library stream (backend::GpuTimer, backend/cuda/util.hpp:92-120). */
grb_info grb_timer_start(void);
grb_info grb_timer_stop(float* elapsed_ms);

/* ---- Descriptor (graphblas/descriptor.hpp:17-39, backend/cuda/descriptor.hpp) -- */
grb_info grb_descriptor_new(grb_descriptor* desc);
grb_info grb_descriptor_free(grb_descriptor desc);
grb_info grb_descriptor_set(grb_descriptor desc, int field, int value);      /* Descriptor::set    */
grb_info grb_descriptor_get(grb_descriptor desc, int field, int* value);     /* Descriptor::get    */
grb_info grb_descriptor_toggle(grb_descriptor desc, int field);              /* Descriptor::toggle */
/* Descriptor::loadArgs (backend/cuda/descriptor.hpp:207-287): grb_descriptor_load_defaults
 * applies the parseArgs defaults of graphblas/util.hpp:39-132, grb_descriptor_set_arg one
 * named CLI flag: mxvmode switchpoint struconly opreuse earlyexit fusedmask sort endbit
 * memusage atomic dirinfo nthread max_niter niter timing debug directed transpose. */
grb_info grb_descriptor_load_defaults(grb_descriptor desc);
grb_info grb_descriptor_set_arg(grb_descriptor desc, const char* name, double value);
grb_info grb_descriptor_get_arg(grb_descriptor desc, const char* name, double* value);
/* desc->descriptor_.lastmxv_ : GRB_PUSHONLY or GRB_PULLONLY of the last mxv/vxm. */
grb_info grb_descriptor_lastmxv(grb_descriptor desc, int* value);

/* ---- Vector (graphblas/vector.hpp:12-66) ------------------------------------- */
grb_info grb_vector_new(grb_vector* v, grb_dtype dtype, grb_index nsize);    /* Vector(Index)      */
grb_info grb_vector_free(grb_vector v);
grb_info grb_vector_dup(grb_vector dst, grb_vector src);                     /* dup / operator=    */
grb_info grb_vector_clear(grb_vector v);
grb_info grb_vector_size(grb_vector v, grb_index* nsize);
/* Vector::resize (vector.hpp:230-237): keeps the first min(nsize, nvals) stored entries. */
grb_info grb_vector_resize(grb_vector v, grb_index nsize);
grb_info grb_vector_nvals(grb_vector v, grb_index* nvals);
/* build(indices, values, nvals, dup) -> sparse; host arrays; values are dtype-typed. */
grb_info grb_vector_build_sparse(grb_vector v, const grb_index* indices, const void* values,
                                 grb_index nvals);
/* build(values, nvals) -> dense; host array. */
grb_info grb_vector_build_dense(grb_vector v, const void* values, grb_index nvals);
/* build(T* values, nvals) / build(Index*, T*, nvals): adopt caller DEVICE pointers
 * without ownership (dense_vector.hpp:215-224, sparse_vector.hpp:164-175).
 * Adopted pointers (here, in grb_matrix_adopt_device_csr, and the raw pointers of grb_k_spmv / grb_spmm) need 4-byte
 * alignment only: where a kernel has a 16-byte path it looks at the pointer and falls back to 4-byte accesses, and the
 * library never writes outside [ptr, ptr + nvals).  An adopted sparse vector that is used as an OUTPUT must have room
 * for nsize entries in both arrays (the library cannot check that); as an input nvals entries suffice. */
grb_info grb_vector_adopt_dense(grb_vector v, void* d_values, grb_index nvals);
grb_info grb_vector_adopt_sparse(grb_vector v, grb_index* d_indices, void* d_values,
                                 grb_index nvals);
grb_info grb_vector_set_element(grb_vector v, double val, grb_index index);
grb_info grb_vector_extract_element(grb_vector v, double* val, grb_index index);
/* extractTuples(indices, values, n): sparse vector only; *n must equal nvals. */
grb_info grb_vector_extract_tuples_sparse(grb_vector v, grb_index* indices, void* values,
                                          grb_index* n);
/* extractTuples(values, n): densifies a sparse vector with fill 0 (vector.hpp:208-217);
 * *n must equal size. */
grb_info grb_vector_extract_tuples_dense(grb_vector v, void* values, grb_index* n);
grb_info grb_vector_fill(grb_vector v, double val);
grb_info grb_vector_fill_ascending(grb_vector v, grb_index nvals);
grb_info grb_vector_get_storage(grb_vector v, int* storage);
grb_info grb_vector_set_storage(grb_vector v, int storage);
grb_info grb_vector_swap(grb_vector a, grb_vector b);
/* backend::Vector::{convert,sparse2dense,dense2sparse} (backend/cuda/vector.hpp:291-425). */
grb_info grb_vector_convert(grb_vector v, double identity, float switchpoint, grb_descriptor desc);
grb_info grb_vector_sparse2dense(grb_vector v, double identity, grb_descriptor desc /*nullable*/);
grb_info grb_vector_dense2sparse(grb_vector v, double identity, grb_descriptor desc);
/* Raw device views (sparse_.d_ind_, sparse_.d_val_, dense_.d_val_) for zero-copy
 * interop (RCCL buffers, torch tensors); valid until the vector is freed or resized. */
grb_info grb_vector_device_ptrs(grb_vector v, grb_index** d_sparse_ind, void** d_sparse_val,
                                void** d_dense_val);

/* ---- Matrix (graphblas/matrix.hpp:13-84) ------------------------------------- */
grb_info grb_matrix_new(grb_matrix* A, grb_dtype dtype, grb_index nrows, grb_index ncols);
grb_info grb_matrix_free(grb_matrix A);
/* build(row_indices, col_indices, values, nvals, dup): host COO, sorted internally
 * (coo2csr + coo2csc, backend/cuda/sparse_matrix.hpp:289-351). */
grb_info grb_matrix_build(grb_matrix A, const grb_index* row_indices, const grb_index* col_indices,
                          const void* values, grb_index nvals);
/* Ingest on the device: the loader's semantics of readMtx (util.hpp:197-329,
 * 363-430) applied to a DEVICE coordinate list, then the same sort + compress as build().
 * flags: 1 add the reverse of every off-diagonal entry (symmetric / --directed 2), 2 drop self
 * loops, 4 drop duplicates (first occurrence wins).  d_values NULL = pattern (every value 1). */
grb_info grb_matrix_ingest_device(grb_matrix A, const grb_index* d_rows, const grb_index* d_cols,
                                  const void* d_values, grb_index nvals, int flags);
/* Host CSR in, CSC derived (csr2csc); `csc_*` may be given to skip the transpose. */
grb_info grb_matrix_build_csr(grb_matrix A, const grb_index* csr_row_ptr, const grb_index* csr_col_ind,
                              const void* csr_val, grb_index nvals, const grb_index* csc_col_ptr,
                              const grb_index* csc_row_ind, const void* csc_val);
/* build(row_ptr, col_ind, values, nvals) adopting DEVICE CSR (+ optional CSC) pointers
 * without ownership (sparse_matrix.hpp:417-435).  Every array may start at any 4-byte boundary (see
 * grb_vector_adopt_dense); the library only reads them. */
grb_info grb_matrix_adopt_device_csr(grb_matrix A, grb_index* d_csr_row_ptr, grb_index* d_csr_col_ind,
                                     void* d_csr_val, grb_index nvals, grb_index* d_csc_col_ptr,
                                     grb_index* d_csc_row_ind, void* d_csc_val);
grb_info grb_matrix_nrows(grb_matrix A, grb_index* nrows);
grb_info grb_matrix_ncols(grb_matrix A, grb_index* ncols);
grb_info grb_matrix_nvals(grb_matrix A, grb_index* nvals);
/* Host mirrors h_csrRowPtr_/h_csrColInd_/h_csrVal_ and h_cscColPtr_/h_cscRowInd_/h_cscVal_
 * (sparse_matrix.hpp:120-132) that the CPU oracles read (algorithm/bfs.hpp:100-107). */
grb_info grb_matrix_host_csr(grb_matrix A, const grb_index** row_ptr, const grb_index** col_ind,
                             const void** val);
grb_info grb_matrix_host_csc(grb_matrix A, const grb_index** col_ptr, const grb_index** row_ind,
                             const void** val);
/* Overwrite the stored values (CSR order; CSC is re-derived): what gsssp.cu:79-86 does
 * through apply() + syncCpu, and gpr.cu:82-90 through the matrix eWiseMult variants. */
grb_info grb_matrix_set_values(grb_matrix A, const void* csr_val);

/* Binary CSR cache, the reference's interchange format (Appendix B of SURVEY.md):
 * `<dir>/.<file>.<ud|d>.<nosl|sl>.bin` = int32 nrows, int32 nvals, int32 rowptr[nrows+1],
 * int32 colind[nvals]; square matrices, values implied 1.
 *   grb_cache_name          util.hpp:340-357 (convert): the cache path for a .mtx path
 *   grb_matrix_write_cache  backend/cuda/sparse_matrix.hpp:328-348 (end of build(..., dat_name))
 *   grb_matrix_build_cache  backend/cuda/sparse_matrix.hpp:355-407 (build(char* dat_name)):
 *                           GrB_NO_VALUE when the file cannot be opened */
grb_info grb_cache_name(const char* mtx_path, int is_undirected, char* out, size_t cap);
grb_info grb_matrix_write_cache(grb_matrix A, const char* path);
grb_info grb_matrix_build_cache(grb_matrix A, const char* path);

/* ---- Operations (graphblas/operations.hpp) ----------------------------------- */
/* vxm  operations.hpp:59-87   -> backend/cuda/operations.hpp:80-209  */
grb_info grb_vxm(grb_vector w, grb_vector mask, grb_accum accum, grb_semiring op, grb_vector u,
                 grb_matrix A, grb_descriptor desc);
/* mxv  operations.hpp:97-127  -> backend/cuda/operations.hpp:215-327 */
grb_info grb_mxv(grb_vector w, grb_vector mask, grb_accum accum, grb_semiring op, grb_matrix A,
                 grb_vector u, grb_descriptor desc);
/* eWiseMult (vector x vector)  operations.hpp:137-158 -> backend :331-410 */
grb_info grb_eWiseMult(grb_vector w, grb_vector mask, grb_accum accum, grb_semiring op, grb_vector u,
                       grb_vector v, grb_descriptor desc);
/* eWiseAdd (vector + vector)   operations.hpp:277-298 -> backend :567-627 */
grb_info grb_eWiseAdd(grb_vector w, grb_vector mask, grb_accum accum, grb_semiring op, grb_vector u,
                      grb_vector v, grb_descriptor desc);
/* eWiseAdd (vector + scalar)   operations.hpp:333-352 -> backend :649-699 */
grb_info grb_eWiseAdd_scalar(grb_vector w, grb_vector mask, grb_accum accum, grb_semiring op,
                             grb_vector u, double val, grb_descriptor desc);
/* reduce (vector -> scalar)    operations.hpp:642-660 -> backend :1004-1030; result on host. */
grb_info grb_reduce_vector(double* val, grb_accum accum, grb_monoid op, grb_vector u,
                           grb_descriptor desc);
/* reduce (matrix -> vector, row-wise)  operations.hpp:620-640 -> backend :953-986 */
grb_info grb_reduce_matrix_rows(grb_vector w, grb_vector mask, grb_accum accum, grb_monoid op,
                                grb_matrix A, grb_descriptor desc);
/* assign (constant under mask, GrB_ALL)  operations.hpp:509-530 -> backend :822-860 */
grb_info grb_assign(grb_vector w, grb_vector mask, grb_accum accum, double val, grb_descriptor desc);

/* assignScatter  w[indices[k]] = u[k]   operations.hpp:771-790 -> backend :1170-1210 (scatter.hpp:85-123) */
grb_info grb_assignScatter(grb_vector w, grb_vector mask, grb_accum accum, grb_vector u, grb_vector indices,
                           grb_descriptor desc);
/* extractGather  w[k] = u[indices[k]]   operations.hpp:800-815 -> backend :1212-1253 (gather.hpp:11-50) */
grb_info grb_extractGather(grb_vector w, grb_vector mask, grb_accum accum, grb_vector u, grb_vector indices,
                           grb_descriptor desc);

/* The queue of element-wise calls (csrc/lazy.hip).  eWiseAdd / eWiseMult / dup on dense, library-owned
 * vectors without a mask are not run when they are called: up to six of them wait and run as ONE kernel -- every vector
 * read once, every result written once -- as soon as ANY other entry point of this header is called (each one starts by
 * flushing), so nothing can observe the difference except the launch count.  Vectors over adopted (caller-owned)
 * storage never take part.  grb_set_lazy(0) / GRB_LAZY=0: every call runs when it is called; on < 0 only queries;
 * returns the previous setting.  grb_lazy_pending(): steps waiting (does not flush). */
int grb_set_lazy(int on);
int grb_lazy_pending(void);
/* reductions that ran inside a chain's launch so far (grb_reduce_vector on a pending result); does not flush */
int grb_lazy_fused_reductions(void);

/* apply on the device   operations.hpp:559-579 / :581-601 -> backend :878-957 (apply.hpp: host loops there).
 * Vector: w = f(u) on every stored element (dense: all of them; sparse: the nvals stored ones, indices copied), w takes
 * u's storage; w == u is allowed.  A mask is GrB_NOT_IMPLEMENTED (the reference prints "apply masked not implemented").
 * Matrix: in place on the stored values of both orientations (C == A, owned storage), as the reference's
 * C->h_csrVal_[i] = op(A->h_csrVal_[i]) + syncCpu.  binop is a grb_binary_op for the two BIND kinds, ignored otherwise. */
grb_info grb_vector_apply(grb_vector w, grb_vector mask, grb_accum accum, int unary, int binop, double scalar, grb_vector u,
                          grb_descriptor desc);
grb_info grb_matrix_apply(grb_matrix C, grb_matrix mask, grb_accum accum, int unary, int binop, double scalar, grb_matrix A,
                          grb_descriptor desc);

/* mxm   operations.hpp:22-51 -> backend :18-78.  C = op(A) (+.x) op(B); op(A) is A^T under GrB_INP0 = GrB_TRAN (read from
 * A's CSC), op(B) is B^T under GrB_INP1 = GrB_TRAN (read from B's CSC); accum and the other descriptor fields are ignored.
 * With a mask (spgemm.hpp:22-110): C takes the mask's structure and C(i,j) is computed where the mask value is nonzero.
 * Without one (mask == NULL; the reference's cuSPARSE call, spgemm.hpp:282-): f32 A, B and C only -- every other type
 * combination is GRB_NOT_IMPLEMENTED, as in the reference -- but every semiring is honoured, registered ones included.
 * C holds every (i, j) with at least one k where op(A)(i,k) and op(B)(k,j) are both stored (stored zeros count), columns
 * ascending, C(i,j) = add(mul(a_ik, b_kj), acc) folded over k ascending from the identity; the same inputs give the same
 * bits.  C == A or C == B: GRB_NOT_IMPLEMENTED; the side an orientation needs absent: GRB_INVALID_OBJECT; inner or outer
 * dimensions that do not agree: GRB_DIMENSION_MISMATCH; more than INT32_MAX entries in C, or a failed device allocation:
 * GRB_OUT_OF_MEMORY.  On any error C keeps what it held.  The result is CSR only (no CSC), as the masked product's. */
grb_info grb_mxm(grb_matrix C, grb_matrix mask, grb_accum accum, grb_semiring op, grb_matrix A, grb_matrix B,
                 grb_descriptor desc);
/* eWiseMult, matrix (x) broadcast scalar / vector, in place (C == A)   operations.hpp:206-267 ->
 * backend ewisemult.hpp:275-341,470-622 + kernels/ewisemult.hpp:160-237.  Vector form:
 * C(i,j) = A(i,j) (x) B(i), or B(j) with GrB_INP1 = GrB_TRAN; B must be dense. */
grb_info grb_matrix_eWiseMult_scalar(grb_matrix C, grb_semiring op, grb_matrix A, double val);
grb_info grb_matrix_eWiseMult_vector(grb_matrix C, grb_semiring op, grb_matrix A, grb_vector B,
                                     grb_descriptor desc);
/* eWiseAdd / eWiseMult of two matrices   operations.hpp:166-204 (eWiseMult), 307-325 (eWiseAdd); the reference's
 * backend returns GrB_NOT_IMPLEMENTED (backend/cuda/operations.hpp:414-423).  op(A) is A^T under GrB_INP0 = GrB_TRAN and
 * op(B) is B^T under GrB_INP1 = GrB_TRAN, read from that matrix's CSC as grb_mxm reads it (eWiseAdd(C, A, A) with INP1 =
 * TRAN is A + A^T).  C holds the union (eWiseAdd) or the intersection (eWiseMult) of the two structures -- stored zeros
 * count, nothing is dropped by value -- with columns ascending in every row.  An entry in both: add(a, b) (eWiseAdd) or
 * mul(a, b) (eWiseMult) of op's operators, a from op(A) first; an entry in one operand only (eWiseAdd): copied bit for
 * bit.  The same inputs give the same bits.  With a mask, an entry is kept only where the mask stores a nonzero value
 * (mxm's rule), inverted under GrB_MASK = GrB_SCMP; the mask is f32 or i32 and read from its CSR.  accum and the other
 * descriptor fields are ignored: C is replaced, as grb_mxm replaces it.  A, B and C all GRB_F32 or all GRB_I32, else
 * GRB_NOT_IMPLEMENTED.  C may be A, B or the mask.  On any error C keeps what it held: a null handle or an unbuilt A, B or
 * mask: GRB_UNINITIALIZED_OBJECT; shapes of op(A), op(B), C and the mask that differ: GRB_DIMENSION_MISMATCH; a transposed
 * operand without a CSC of its own (a product result, the CSR-only format): GRB_INVALID_OBJECT; more than INT32_MAX
 * entries in C, or a failed device allocation: GRB_OUT_OF_MEMORY.  C always gets its CSR, and also a CSC (the same merge
 * over the other orientations: the same entries and bits) when op(A), op(B) and the mask each have their other
 * orientation; otherwise C is CSR only, as a product result.  A C of the CSR-only format aliases its CSC to the CSR. */
grb_info grb_matrix_eWiseAdd(grb_matrix C, grb_matrix mask, grb_accum accum, grb_semiring op, grb_matrix A, grb_matrix B,
                             grb_descriptor desc);
grb_info grb_matrix_eWiseMult(grb_matrix C, grb_matrix mask, grb_accum accum, grb_semiring op, grb_matrix A, grb_matrix B,
                              grb_descriptor desc);
/* transpose   operations.hpp:682.  C = A^T, or C = A under GrB_INP0 = GrB_TRAN (GraphBLAS's definition), f32 or i32 with
 * C of A's type (else GRB_NOT_IMPLEMENTED); a mask: GRB_NOT_IMPLEMENTED.  C gets both orientations, sorted (subject to
 * its own format): two device copies when A has both, a device sort of A's CSR when A is CSR only.  So transpose with
 * INP0 = TRAN is how a product result gets a CSC.  Aliasing, error codes and C after an error as for eWiseAdd. */
grb_info grb_transpose(grb_matrix C, grb_matrix mask, grb_accum accum, grb_matrix A, grb_descriptor desc);
/* extract   operations.hpp:355-410 (subvector, submatrix, matrix column; the reference prints "not implemented yet" and
 * returns GrB_NOT_IMPLEMENTED for all three).  Index lists are host arrays, as the reference's const std::vector<Index>*;
 * a null list means every index in order (GrB_ALL) and its count must then be the dimension it stands for.  Lists may be
 * in any order and may hold duplicates: a duplicate repeats a row, a column or an element.  desc == NULL: the defaults.
 * accum and the descriptor fields other than GrB_INP0 are ignored: the output is replaced.  A mask: GRB_NOT_IMPLEMENTED
 * (a caller who wants one applies grb_matrix_eWiseAdd under it afterwards).  The same inputs give the same bits.
 *
 * grb_matrix_extract: C = op(A)(I, J).  op(A) is A, or A^T under GrB_INP0 = GrB_TRAN, read from A's CSC as grb_mxm reads
 * it (a transposed operand without a CSC of its own: GRB_INVALID_OBJECT).  C is nrows x ncols and C(i, j) =
 * op(A)(I[i], J[j]) wherever that entry is stored -- stored zeros count, values are copied bit for bit -- with columns
 * ascending in every row.  A and C both GRB_F32 or both GRB_I32, else GRB_NOT_IMPLEMENTED.  C may be A.  C gets its CSR,
 * and also a CSC (the same extraction with I and J exchanged over op(A)'s other orientation: the same entries and bits)
 * when that orientation exists; otherwise C is CSR only, as a product result.  A C of the CSR-only format aliases its CSC.
 *
 * grb_matrix_extract_col: w = op(A)(I, j): column col_index of A read from its CSC (A without a CSC of its own:
 * GRB_INVALID_OBJECT), or row col_index of A under GrB_INP0 = GrB_TRAN, read from the CSR.  w has size nrows and becomes
 * a sparse vector holding entry k wherever op(A)(I[k], j) is stored, indices ascending.  w of A's type, f32 or i32, else
 * GRB_NOT_IMPLEMENTED.
 *
 * grb_vector_extract: w = u(I); w has size nindices.  A dense u gives a dense w with w[k] = u[I[k]]; a sparse u (indices
 * ascending, as every operation of this library leaves them) a sparse w with entry k wherever I[k] is stored in u, indices
 * ascending.  Any element type, w of u's (else GRB_DOMAIN_MISMATCH); w may be u.
 *
 * On every error the output keeps what it held.  A null handle or an unbuilt input: GRB_UNINITIALIZED_OBJECT; nrows /
 * ncols / nindices that differ from the output's shape, or a null list whose count is not the dimension of op(A) / u:
 * GRB_DIMENSION_MISMATCH; an index (col_index included) < 0 or >= the dimension it addresses, found before anything is
 * written: GRB_INDEX_OUT_OF_BOUNDS; more than INT32_MAX entries in the result (possible through duplicates), or a failed
 * device allocation: GRB_OUT_OF_MEMORY.  A count of zero is legal: an empty matrix or vector of that shape. */
grb_info grb_matrix_extract(grb_matrix C, grb_matrix mask, grb_accum accum, grb_matrix A,
                            const grb_index* row_indices, grb_index nrows,
                            const grb_index* col_indices, grb_index ncols, grb_descriptor desc);
grb_info grb_matrix_extract_col(grb_vector w, grb_vector mask, grb_accum accum, grb_matrix A,
                                const grb_index* row_indices, grb_index nrows, grb_index col_index,
                                grb_descriptor desc);
grb_info grb_vector_extract(grb_vector w, grb_vector mask, grb_accum accum, grb_vector u,
                            const grb_index* indices, grb_index nindices, grb_descriptor desc);
/* assign, matrix forms   operations.hpp:441-551 (C(I, J) = A, C(I, j) = u, C(i, J) = u, C(I, J) = val; the reference prints
 * "assign matrix variant not implemented yet" and returns GrB_NOT_IMPLEMENTED for all four).  GraphBLAS's GrB_assign
 * without GrB_REPLACE.  Index lists are host arrays in any order; a null list is GrB_ALL and its count must then be C's
 * dimension.  A repeated index makes the result undefined in GraphBLAS: here it is GRB_INVALID_INDEX, found before anything
 * is written.  accum_op is -1 for no accum, else a grb_binary_op (all 17), applied as accum(c, t) in C's element type by the
 * operator dispatch of grb_matrix_apply's BIND forms.  desc == NULL: the defaults; fields other than GrB_INP0 (the matrix
 * form) and GrB_MASK are ignored.
 *
 * Let T hold the source at its targets -- T(I[i], J[j]) = op(A)(i, j) wherever that is stored; T(I[k], j) = u[k];
 * T(i, J[k]) = u[k]; val at every position of I x J -- and R = I x J.  Position by position, Z is: in T and in C:
 * accum(c, t), or t without an accum; in T only: t; in C only inside R: kept under an accum, DELETED without one; in C only
 * outside R: kept bit for bit.  With a mask M of C's shape (the matrix and the constant form) the new C is Z where M stores a
 * nonzero value and the old C elsewhere, inverted under GrB_MASK = GrB_SCMP (mxm's rule).  Stored zeros count everywhere:
 * nothing is dropped by value.  Columns ascend in every row; the same inputs give the same bits.  op(A) is A, or A^T under
 * GrB_INP0 = GrB_TRAN, read from A's CSC as grb_matrix_extract reads it.  u may be sparse (its stored entries) or dense
 * (every element counts as stored).  val becomes C's element type.  C, A / u all GRB_F32 or all GRB_I32, else
 * GRB_NOT_IMPLEMENTED; the mask may be either type.  The vector mask of the row and column forms: GRB_NOT_IMPLEMENTED.
 * C may be A or the mask.  A C that was never built counts as empty.
 *
 * C gets its CSR, and also a CSC (the same routine over the other orientations with I and J exchanged: the same entries
 * and bits) when the old C, op(A) and the mask each have their other orientation; otherwise C is CSR only, as a product
 * result.  A C of the CSR-only format aliases its CSC.
 *
 * On every error C keeps what it held.  A null handle or an unbuilt input: GRB_UNINITIALIZED_OBJECT; nrows / ncols that
 * differ from op(A)'s shape or u's size, a mask not of C's shape, or a null list whose count is not C's dimension:
 * GRB_DIMENSION_MISMATCH; an index, row_index or col_index outside C: GRB_INDEX_OUT_OF_BOUNDS; a repeated index:
 * GRB_INVALID_INDEX; a transposed A without a CSC of its own: GRB_INVALID_OBJECT; more than INT32_MAX entries in the result
 * (a 64-bit total, checked before C is touched), or a failed device allocation: GRB_OUT_OF_MEMORY.  A count of zero is
 * legal and leaves C as it was. */
grb_info grb_matrix_assign(grb_matrix C, grb_matrix mask, int accum_op, grb_matrix A,
                           const grb_index* row_indices, grb_index nrows,
                           const grb_index* col_indices, grb_index ncols, grb_descriptor desc);
grb_info grb_matrix_assign_scalar(grb_matrix C, grb_matrix mask, int accum_op, double val,
                                  const grb_index* row_indices, grb_index nrows,
                                  const grb_index* col_indices, grb_index ncols, grb_descriptor desc);
grb_info grb_matrix_assign_col(grb_matrix C, grb_vector mask, int accum_op, grb_vector u,
                               const grb_index* row_indices, grb_index nrows, grb_index col_index,
                               grb_descriptor desc);
grb_info grb_matrix_assign_row(grb_matrix C, grb_vector mask, int accum_op, grb_vector u,
                               grb_index row_index, const grb_index* col_indices, grb_index ncols,
                               grb_descriptor desc);
/* select   (GraphBLAS C API 2.0, GrB_select; the reference has no such operation, so the definition is GraphBLAS's own.)
 * The result keeps exactly the stored entries for which the predicate select_op (a grb_select_op, above) holds with the
 * thunk; values are copied bit for bit and the order is unchanged.  Stored zeros are entries like any other, so
 * GRB_SEL_VALUENE with thunk 0 is how they are dropped.  desc == NULL: the defaults.  accum and the descriptor fields
 * other than GrB_INP0 are ignored: the output is replaced.  A mask: GRB_NOT_IMPLEMENTED, as for extract and transpose (a
 * caller who wants one applies grb_matrix_eWiseAdd under it afterwards).  The same inputs give the same bits.
 *
 * The thunk crosses the ABI as a double.  Positional operators (TRIL .. COLGT): it must be integer-valued, else
 * GRB_INVALID_VALUE, and is used in 64-bit arithmetic, so i + k cannot wrap for any thunk (+-2^40 included).  Value
 * operators on f32: the thunk is rounded to float and the comparison is IEEE f32 (NaN passes only VALUENE; -0.0f == 0.0f).
 * Value operators on i32: the thunk must be an integer in [INT32_MIN, INT32_MAX], else GRB_INVALID_VALUE (rounding it
 * silently would turn >= 2.5 into >= 2).
 *
 * grb_matrix_select: C = select(op(A)).  op(A) is A, or A^T under GrB_INP0 = GrB_TRAN, read from A's CSC as
 * grb_matrix_extract reads it (a transposed A without a CSC of its own: GRB_INVALID_OBJECT).  C has op(A)'s shape.  A and
 * C both GRB_F32 or both GRB_I32, else GRB_NOT_IMPLEMENTED.  C holds the kept entries with columns ascending in every row;
 * rows that lose everything stay as empty rows.  C may be A.  C always gets its CSR, and also a CSC (the same routine over
 * op(A)'s other orientation with the roles of i and j exchanged in the predicate: the same entries and bits) when that
 * orientation exists; otherwise C is CSR only, as a product result.  A C of the CSR-only format aliases its CSC.
 *
 * grb_vector_select: w = select(u), i the index and j = 0.  w has u's size and u's type (else GRB_DOMAIN_MISMATCH) and
 * always becomes a sparse vector with ascending indices: from a sparse u the stored entries that pass, from a dense u
 * every element counts as stored.  w may be u.
 *
 * On every error the output keeps what it held; all of them are found before anything of the output is written.  A null
 * handle or an unbuilt input: GRB_UNINITIALIZED_OBJECT; a C not of op(A)'s shape, or a w not of u's size:
 * GRB_DIMENSION_MISMATCH; select_op outside the enum, or a thunk the rules above reject: GRB_INVALID_VALUE; a failed device
 * allocation: GRB_OUT_OF_MEMORY.  The result is never larger than the input, so there is no INT32_MAX case. */
grb_info grb_matrix_select(grb_matrix C, grb_matrix mask, grb_accum accum, int select_op, double thunk,
                           grb_matrix A, grb_descriptor desc);
grb_info grb_vector_select(grb_vector w, grb_vector mask, grb_accum accum, int select_op, double thunk,
                           grb_vector u, grb_descriptor desc);
/* kronecker   (GraphBLAS C API, GrB_kronecker; the reference declares no such operation, so the definition is GraphBLAS's
 * own.)  C = op(A) (x) op(B): with op(A) mA x nA and op(B) mB x nB, C is (mA * mB) x (nA * nB) and
 * C(iA * mB + iB, jA * nB + jB) = mul(op(A)(iA, jA), op(B)(iB, jB)) wherever both entries are stored -- stored zeros
 * count, nothing is dropped by value, so nvals(C) = nvals(A) * nvals(B) -- with columns ascending in every row.  mul is the
 * multiplicative operator of op, A's value first: all 17 built-in semirings and the ids of grb_semiring_register; the
 * additive monoid is not used.  op(A) is A, or A^T under GrB_INP0 = GrB_TRAN; op(B) is B, or B^T under GrB_INP1 = GrB_TRAN,
 * read from that matrix's CSC as grb_mxm reads it.  desc == NULL: the defaults.  A, B and C all GRB_F32 or all GRB_I32,
 * else GRB_NOT_IMPLEMENTED.  A mask: GRB_NOT_IMPLEMENTED, as for extract, select and transpose (a caller who wants one
 * applies grb_matrix_eWiseMult under it afterwards).  accum and the other descriptor fields are ignored: C is replaced.
 * C may be A, B or both.  The same inputs give the same bits.  An operand with no entries gives an empty C of the right
 * shape.  C always gets its CSR, and also a CSC (the same routine over the other orientations of op(A) and op(B), since
 * (A (x) B)^T = A^T (x) B^T: the same entries and bits) when op(A) and op(B) both have their other orientation; otherwise
 * C is CSR only, as a product result.  A C of the CSR-only format aliases its CSC.
 *
 * On every error C keeps what it held; all of them are found before anything of C is written.  A null handle or an
 * unbuilt A or B: GRB_UNINITIALIZED_OBJECT; a C whose shape is not (mA * mB) x (nA * nB), the products taken in 64 bits:
 * GRB_DIMENSION_MISMATCH; a transposed operand without a CSC of its own (a product result, the CSR-only format):
 * GRB_INVALID_OBJECT; a semiring id that does not exist: GRB_INVALID_VALUE; nvals(A) * nvals(B) > INT32_MAX as a 64-bit
 * product, or a failed device allocation: GRB_OUT_OF_MEMORY. */
grb_info grb_kronecker(grb_matrix C, grb_matrix mask, grb_accum accum, grb_semiring op, grb_matrix A, grb_matrix B,
                       grb_descriptor desc);
/* reduce (matrix -> scalar)   operations.hpp:662-680 -> backend :1032-1059 (reduce.hpp:81-91) */
grb_info grb_reduce_matrix_scalar(double* val, grb_accum accum, grb_monoid op, grb_matrix A, grb_descriptor desc);
/* traceMxmTranspose (extension)   operations.hpp:698-711 -> backend :1076-1108 (trace.hpp:10-52):
 * *val = sum_i (+)_k A(i,k) (x) B(i,k), the trace of A (+).(x) B^T; A and B of one element type. */
grb_info grb_trace_mxm_transpose(double* val, grb_semiring op, grb_matrix A, grb_matrix B, grb_descriptor desc);
/* Extension: readMtx (graphblas/util.hpp:363-430) + Matrix::build in one call with the MatrixMarket text
 * parsed on the device (coordinate pattern / integer / real, general / symmetric).  *A is created here;
 * directed as readMtx (0 banner decides, 1 directed, 2 undirected); dims_out (nullable) = {nrows, ncols,
 * nvals after the loader}.  Where the loader drops entries of a valued file each survivor keeps its own
 * value (the reference leaves the values array unshifted there, util.hpp:311-323). */
grb_info grb_matrix_load_mtx(grb_matrix* A, const char* path, grb_dtype dtype, int directed, grb_index* dims_out);
/* tril   operations.hpp:872-886 -> tri.hpp:10-53 (host side, as in the reference) */
grb_info grb_matrix_tril(grb_matrix C, grb_matrix A, grb_descriptor desc);

/* ---- Algorithms: the drivers of graphblas/algorithm/{bfs,...}.hpp built on the ops above.
 * *_fused variants run the same level loop on the device-resident representation
 * (bitmap frontier, no per-op host round trips) and must return identical results. */
typedef struct {
  int      levels;            /* iterations executed                                  */
  float    tight_ms;          /* HIP-event time of the level loop ("tight", bfs.hpp:42-88) */
  int64_t  edges_traversed;   /* sum of out-degree over reached vertices (TEPS numerator) */
  int32_t  reached;           /* vertices with a nonzero label                         */
} grb_bfs_result;

/* Per-level record, filled when `levels_out` is non-NULL (capacity max_levels). */
typedef struct {
  int32_t direction;          /* 0 push (SpMSpV), 1 pull (SpMV): desc lastmxv_          */
  int32_t frontier;           /* nf: vertices in the input frontier                    */
  int64_t frontier_edges;     /* push: mf = sum of frontier out-degrees; pull: inspected edges (profile bit 1) */
  int32_t discovered;         /* vertices labelled by this level                       */
  float   ms;                 /* HIP-event time of this level (only in profiling mode) */
} grb_bfs_level;

/* algorithm::bfs (algorithm/bfs.hpp:14-89) op by op through grb_assign/grb_vxm/grb_reduce. */
grb_info grb_bfs(grb_vector v, grb_matrix A, grb_index source, grb_descriptor desc,
                 grb_bfs_result* result);
/* Same result, fused device-resident level loop.  profile bit 0: HIP events around every
 * level's expansion kernel(s) -> grb_bfs_level.ms (cheap).  profile bit 1: pull levels also
 * count the edges they inspect (slower kernel variant) -> grb_bfs_level.frontier_edges. */
grb_info grb_bfs_fused(grb_vector v, grb_matrix A, grb_index source, grb_descriptor desc,
                       grb_bfs_result* result, grb_bfs_level* levels_out, int max_levels,
                       int profile);
/* The same traversal, queued without waiting: the launch is put on the library's stream and the call returns; the
 * result block is read by grb_bfs_wait.  K traversals into K vectors run back to back on the device with no host
 * round trip between them (the reference's loop returns to the host several times per LEVEL, algorithm/bfs.hpp:42-88:
 * `reduce` -> succ, `nvals`, the timing branches).  The results are as if the traversals ran in the order they were
 * queued (several may run side by side in one launch, grb_bfs_set_coschedule: never two into the same vector); v, A and
 * desc must stay alive and untouched by the caller until the ticket has been waited for (v's contents are undefined
 * until then; any other entry point may be called meanwhile -- it is ordered behind the queued traversals on the
 * stream).  Under co-scheduling (the default) a queued traversal starts on the device when a ticket is waited for or
 * another entry point is called, not at the enqueue (see grb_bfs_set_coschedule); a gathered group of
 * 20 or more plain traversals runs as one bit-parallel sweep inside that call (see grb_bfs_set_sweep_from).  At most
 * 256 tickets may be outstanding (GRB_INSUFFICIENT_SPACE).  A traversal the one-launch kernel does not serve (road-network
 * queues, GRB_SPARSE_MATRIX_FORMAT=1) runs to its end inside the enqueue call; its ticket waits like any other.
 * grb_bfs_wait returns what grb_bfs_fused would have returned (a launch that could not finish is re-run through the
 * host-driven level loop there); a ticket can be waited for once (GRB_INVALID_VALUE afterwards).
 * Ordering of the labels: grb_bfs_wait returns when the traversal's RECORD has arrived; the library's own stream is
 * ordered behind the launch, so every entry point called afterwards sees the complete depth vector.  A caller that reads
 * v's storage itself (grb_vector_device_ptrs) on a stream of its own gets the same guarantee a different way: for a
 * vector whose storage has been handed out, grb_bfs_wait waits for the launch itself
 * (tests/test_gpu_algorithms.py::test_bfs_wait_on_a_vector_read_through_its_device_pointer). */
typedef int64_t grb_bfs_ticket;
grb_info grb_bfs_fused_enqueue(grb_vector v, grb_matrix A, grb_index source, grb_descriptor desc,
                               grb_bfs_ticket* ticket);
grb_info grb_bfs_wait(grb_bfs_ticket ticket, grb_bfs_result* result);
/* Traversals in flight at once (1 .. 8; default 1).  With n > 1 the traversals queued by grb_bfs_fused_enqueue go round n
 * lanes -- a stream each, launches of (CUs / n) workgroups -- so that n of them are resident together: a traversal spends
 * two thirds of its time in barriers and latency chains that more CUs do not shorten, so two on half the device each
 * finish in 1.4 x the time of one on all of it (RMAT-22), four in 2 x.  Per-traversal results are unchanged; the
 * blocking grb_bfs_fused keeps the whole device (and, issued while lanes are busy, waits for their grids to drain).
 * Changing the number waits for everything queued.  n < 1 only queries.  Returns the previous value. */
int grb_bfs_set_lanes(int n);
/* Traversals side by side in one LAUNCH (1 .. 12).  By default the library co-schedules by itself: a launch has one
 * sub-grid per gathered traversal, up to twelve, as many as fit in a quarter of the device memory that is free (a
 * sub-grid keeps about 77 MB of state at RMAT-22, provisioned with the matrix's once-per-matrix preparation by its first
 * one-traversal launch, or else by the first launch of several; when memory runs short the launches narrow, down to one
 * traversal per launch), and a lone gathered traversal takes the
 * one-traversal kernel.  k = 1 gives every traversal its own launch at the enqueue; k > 1 fixes k.  With co-scheduling
 * the traversals queued by grb_bfs_fused_enqueue
 * share launches: a launch is k sub-grids of one workgroup per CU each (512 threads for two, 256 up to four, 128 up to
 * twelve -- that instance is built for six waves per SIMD), every sub-grid runs one traversal at a time on state,
 * barrier counters and bitmaps of its own, and when it has finished one it draws the next of the launch's traversals (up to 48 per launch) from a counter.  A traversal is
 * barriers and dependent-load chains for half of its time; the CU's wave scheduler fills them with the other
 * traversals' work, and -- unlike lanes -- nothing depends on how the runtime maps streams to hardware queues: it is one
 * launch on the library's stream.  A ticket is issued at once; the launch goes out when one of the gathered tickets is
 * waited for, when any other entry point is called (so the ordering rules of grb_bfs_fused_enqueue hold unchanged),
 * when a traversal of another matrix or descriptor, or one into a vector a gathered one writes, is queued, or when 48
 * have gathered.  Per-traversal labels and
 * result blocks are those of grb_bfs_fused; a traversal's record is written after a barrier of its sub-grid, i.e. when
 * every label store has completed.  A traversal runs under the descriptor fields (mxvmode, switchpoint, edgeswitch,
 * max_niter) as they stood when it was QUEUED -- the descriptor's setters launch nothing, and one launch serves one set of
 * rules (a traversal queued under other rules starts a new launch).  Ignored while grb_bfs_set_lanes is above 1.  Changing the number launches and waits
 * for everything queued.  k < 1 only queries.  Returns the previous value: the k last set, 1 while the library chooses
 * (a caller who restores what a query returned gets one traversal per launch).  (No counterpart in the reference, whose loop
 * is one traversal with several host round trips per level: algorithm/bfs.hpp:42-88.) */
int grb_bfs_set_coschedule(int k);
/* Gathered traversals that run as ONE bit-parallel sweep.  Under the default width rule (no grb_bfs_set_coschedule, one
 * lane) a gathered group of k >= 24 traversals of one matrix (docs/experiments.md R8.1) runs as one sweep of the
 * batched traversal (grb_bfs_batch's: one 64-bit word per vertex, so one gather per edge serves every source) when the
 * matrix has both orientations and every traversal of the group is plain: GRB_PUSHPULL, max_niter not below the
 * descriptor's default, f32 vectors, one set of rules.  Everything else takes the co-scheduled launch, as does a sweep
 * that fails (out of memory, a barrier that gave up): nothing is reported, the group is launched the usual way.  The
 * sweep runs where the launch would have gone out (a wait, another entry point, another matrix or rules, 48 gathered),
 * to its end: the tickets hold their results when that call returns, parked only after the label pass has completed.
 * Labels and result blocks are those of grb_bfs_fused per source (levels, reached, edges_traversed; tight_ms is the
 * sweep's device time divided by k); desc's lastmxv is the last traversal's.  The sweep keeps buffers of its own, 22
 * 64-bit words per vertex plus its queues (about 0.85 GB at RMAT-22; kept from matrix to matrix and grown for a larger
 * one), provisioned within a quarter of the free device memory by the matrix's first gathered launch, of any size (one attempt per matrix: a matrix they cannot be made for then is not swept until it is built
 * again).  grb_bfs_set_sweep_from(k) sets the group
 * size from which the queue sweeps (0: never -- grb_bfs_set_coschedule(k >= 1) and grb_bfs_set_lanes(n > 1) also keep
 * every traversal on the per-traversal kernels); k < 0 only queries.  Returns the previous value. */
int grb_bfs_set_sweep_from(int k);
/* Groups the queue has run as a sweep since the process began and the traversals they carried (what has gathered is
 * launched first); either pointer may be NULL. */
grb_info grb_bfs_sweep_counts(long long* sweeps, long long* traversals);
/* Measurement: HIP events on the library's stream around every launch of several traversals.  on != 0 starts collecting
 * (what has gathered is launched first); on == 0 stops, waits for the launches and reports their summed duration, their
 * number and the traversals they ran (bench.py's roofline block of the co-scheduled sibling). */
grb_info grb_bfs_coschedule_profile(int on, double* launch_ms_total, int* launches, int* traversals);
/* Host time (microseconds, summed since the last reset) inside the one-launch traversal's two halves -- queueing the
 * launches / waiting for and unpacking the record -- and the number of traversals; any pointer may be NULL. */
grb_info grb_bfs_host_times(double* enqueue_us, double* wait_us, long long* calls, int reset);

/* ---- 1-D vertex-partitioned BFS level steps (one process per GPU).
 * The reference has no multi-GPU code (backend/cuda/descriptor.hpp:242,283-284 parse
 * --ndevice and ignore it); these follow the single-GPU level loop.  The rank owns
 * vertices [lo, lo + nrows(A)), lo % 64 == 0; A_out / A_in are nrows x n_global matrices
 * whose CSR rows are the owned vertices' out- / in-neighbour lists (global ids).  Bitmaps
 * are 2*ceil(n_global/64) 32-bit words on the device.  The "new bits" bitmaps of all ranks
 * are OR-combined by the caller (RCCL) between push/pull and apply. */
grb_info grb_bfs_part_pull(grb_matrix A_in, grb_index lo, grb_index n_global, const uint32_t* d_vis,
                           uint32_t* d_new /* fully written: zeroed, then the owned word range */,
                           float* d_label_local, float new_label);
grb_info grb_bfs_part_push(grb_matrix A_out, grb_index lo, grb_index n_global, const uint32_t* d_frontier,
                           const uint32_t* d_vis, uint32_t* d_work /* scratch bitmap */,
                           uint32_t* d_new /* fully written */, int64_t* expanded_edges_out /* nullable */);
grb_info grb_bfs_part_apply(const uint32_t* d_new_global, uint32_t* d_vis, grb_index lo, grb_index n_local,
                            grb_index n_global, float* d_label_local, float new_label,
                            int32_t* discovered_out);
grb_info grb_bfs_part_tally(grb_matrix A_out, const float* d_label_local, int64_t* edges_out,
                            int32_t* reached_out);
/* Leaner variants for the host-driven level loop (one launch and one host wake-up each):
 * apply2 = apply + the out-degree sum of the OWNED newly discovered vertices (A_out nullable) and, given the
 * out-degree of every vertex, of ALL of them (the same number on every rank: edge-aware direction switch);
 * push_small = push for a frontier with few out-edges on this rank (d_new fully written);
 * seed = zero vis / new / labels and plant the source; or_parts = OR of `world` all-gathered bitmaps. */
grb_info grb_bfs_part_apply2(const uint32_t* d_new_global, uint32_t* d_vis, grb_index lo, grb_index n_local,
                             grb_index n_global, grb_matrix A_out, const int32_t* d_deg_full /* nullable */,
                             float* d_label_local, float new_label, int32_t* discovered_out,
                             int64_t* local_frontier_edges_out, int64_t* frontier_edges_out /* -1 without d_deg_full */);
grb_info grb_bfs_part_push_small(grb_matrix A_out, grb_index lo, grb_index n_global, const uint32_t* d_frontier,
                                 const uint32_t* d_vis, uint32_t* d_new);
grb_info grb_bfs_part_seed(uint32_t* d_vis, uint32_t* d_new_global, float* d_label_local, grb_index lo,
                           grb_index n_local, grb_index n_global, grb_index source);
grb_info grb_bitmap_or_parts(const uint32_t* d_parts, int world, grb_index nwords, uint32_t* d_out);
/* label == value -> 0 on the owned labels (the host-driven loop after a max_niter cut-off, bfs.hpp:48-66) */
grb_info grb_bfs_part_unlabel(float* d_label_local, grb_index n_local, float value);

/* ---- The same traversal with the level loop on the DEVICE (csrc/bfs_part_run.hip).  A rank context holds the
 * shards (A_out / A_in: the owned vertices' out- / in-neighbour lists, nrows x n_global, global column ids;
 * A_in NULL = the graph is symmetric and one shard serves both), the replicated n-bit visited bitmap, the
 * frontier bitmaps of its owned vertices and the scalars of the level loop.  d_deg_full: out-degree of every
 * vertex (device, int32, replicated; must outlive the context).  grb_bfs_part_run enqueues ONE co-resident
 * launch per level (apply the gathered new bits -> grid barrier -> decide -> expand) followed by ONE all-gather
 * of the n/8-byte new-bits bitmaps on the library communicator (grb_comm_*; skipped when world == 1) and reads
 * nothing back until the traversal has ended: launch k + 1 is enqueued when launch k - 1 has reported through
 * one pinned word -- a rule that uses only values identical on every rank, so all ranks issue the same number
 * of collectives.  levels_per_launch > 1 (world == 1 only) runs that many levels inside one launch.
 * grb_bfs_part_run_group drives `nranks` contexts of a world of `nranks` in lock-step on ONE device with device
 * copies as the all-gather: the test stand-in for a multi-GPU run.  Labels are those of algorithm::bfs
 * (algorithm/bfs.hpp:14-89); the reference has no multi-GPU code (backend/cuda/descriptor.hpp:242). */
typedef struct grb_part_s* grb_part;
typedef struct {
  int32_t levels;             /* levels expanded                                        */
  int32_t launches;           /* level launches enqueued (levels + 2 when one level per launch) */
  int32_t hit_cap;            /* max_niter ended the loop with a non-empty frontier     */
  int64_t edges_traversed;    /* sum of out-degree over reached vertices, whole graph   */
  int64_t reached;            /* vertices with a nonzero label, whole graph             */
  float   ms;                 /* HIP-event time: first launch .. label pass             */
} grb_part_bfs_result;
grb_info grb_part_new(grb_part* part, int rank, int world, grb_index n_global, grb_index lo, grb_matrix A_out,
                      grb_matrix A_in /* nullable */, const int32_t* d_deg_full, int64_t nnz_global);
grb_info grb_part_free(grb_part part);
grb_info grb_bfs_part_run(grb_part part, grb_index source, int mxvmode, float switchpoint, float edgeswitch,
                          int max_niter, int levels_per_launch, float* d_label_local, grb_part_bfs_result* result,
                          grb_bfs_level* levels_out /* nullable */, int max_levels);
grb_info grb_bfs_part_run_group(grb_part* parts, int nranks, grb_index source, int mxvmode, float switchpoint,
                                float edgeswitch, int max_niter, float* const* d_labels,
                                grb_part_bfs_result* results /* nranks */, grb_bfs_level* levels_out, int max_levels);

/* ---- algorithm::sssp (algorithm/sssp.hpp:15-103) on the same 1-D partition, in its frontier form with the round
 * loop on the device (csrc/sssp_part_run.hip).  A_out: the owned vertices' out-edges (nrows x n_global, global
 * column ids, f32 weights >= 0).  Per launch: the (vertex, candidate) pairs the ranks exchanged are applied, a
 * round that every rank has finished expanding is closed (synchronous rounds: the distances after every round and
 * the loop counter are the reference's), the next queue is expanded -- owned targets at once, the others into an
 * outbox of `outbox_pairs` pairs; one all-gather of the outboxes follows every launch (grb_comm_*).  A full outbox
 * only postpones the rest of the round to the next launch.  Nothing is read back until the loop has ended (launch
 * rule as grb_bfs_part_run).  d_dist_local receives the owned distances (FLT_MAX = unreached).
 * grb_sssp_part_run_group: every rank of a world of `nranks` on one device (tests). */
typedef struct grb_part_sssp_s* grb_part_sssp;
typedef struct {
  int32_t iterations;         /* the reference's loop counter at exit (max_niter + 1 when the cap ended it) */
  int32_t rounds;             /* rounds closed                                          */
  int32_t launches;
  int32_t hit_cap;
  float   ms;                 /* HIP-event time, first launch .. distances copied       */
} grb_part_sssp_result;
grb_info grb_part_sssp_new(grb_part_sssp* part, int rank, int world, grb_index n_global, grb_index lo, grb_matrix A_out,
                           int outbox_pairs);
grb_info grb_part_sssp_free(grb_part_sssp part);
grb_info grb_sssp_part_run(grb_part_sssp part, grb_index source, int max_niter, int rounds_per_launch,
                           float* d_dist_local, grb_part_sssp_result* result);
grb_info grb_sssp_part_run_group(grb_part_sssp* parts, int nranks, grb_index source, int max_niter,
                                 float* const* d_dist_local, grb_part_sssp_result* results /* nranks */);

typedef struct {
  int    iterations;          /* loop iterations executed                              */
  float  tight_ms;            /* HIP-event time of the loop                            */
  double last_value;          /* sssp: distances improved by the last round (the part of the
                               * reference's `succ` that decides termination; the op-by-op
                               * driver reports the reference's reduce(m) itself);
                               * pr: last residual `error`                              */
} grb_algo_result;

/* mxm with a dense right-hand side (declared and left a stub by the reference:
 * backend/cuda/operations.hpp:52-70 "SpMM and GEMM not implemented yet", spmm.hpp:15-27):
 *   C = A (+).(x) B   (tran = 0)      C = A^T (+).(x) B   (tran = 1)
 * B [ncols(A or A^T) x k] and C [nrows x k] dense row-major DEVICE arrays of A's element type, any of
 * the 17 semirings; no mask / accum (NULL in the reference's signature).  Row sums in the stored order of a row's
 * entries.  (The Boolean multi-frontier product -- many traversals at once -- is grb_bfs_batch, not this.) */
grb_info grb_spmm(grb_semiring op, grb_matrix A, int tran, const void* d_B, void* d_C, grb_index k,
                  grb_descriptor desc);

/* How the generic SpMV (grb_k_spmv, the pull half of mxv / vxm) reads the input vector for this orientation:
 * `nhot` leading values of the rank-packed vector are staged in LDS; with `bands` > 1 the matrix is also split
 * by column rank into that many bands with an LDS prefix each (`band_nnz` entries in `pieces` (row, band) runs
 * live outside the first prefix's part).  warm != 0 prepares the plan first (otherwise the first product
 * does).  No reference counterpart: mgpu::SpmvCsrBinary (backend/cuda/spmv.hpp:188-190) has no plan. */
grb_info grb_spmv_plan_info(grb_matrix A, int tran, int warm, int* bands, int64_t* band_nnz, int64_t* pieces, int* nhot);
/* How many LDS prefixes (column bands) SpMV plans prepared from now on may use: 1..8, 1 = the one-prefix kernel
 * (the default; the environment variable GRB_SPMV_BANDS sets the initial value).  k <= 0 only queries.  Returns
 * the value in force.  Plans already prepared keep their layout. */
int grb_spmv_set_bands(int k);
/* Which matrix format the generic SpMV multiplies from (csrc/spmv_cband.hpp; GRB_SPMV_FORMAT=csr|auto|cband sets the
 * initial value): 0 the CSR arrays only; 1 (default) a second, column-sorted copy -- row bands of <= 32 Ki rows
 * whose entries are sorted by column rank and coded in 16 + 16 bits, values dropped when all equal -- on
 * orientations whose columns are skewed enough for the hub packing, for the commutative monoids (plus, times,
 * min, max, or, and); 2 that format wherever the monoid allows it.  fmt < 0 only queries.  Returns the value in
 * force.  grb_spmv_format_info reports the prepared copy of an orientation: groups of 64 coded entries (padding
 * included), bands, work items, rows in the hub band, whether the values are stored (iso = 0) and the bytes one
 * launch moves by design.  Results: identical for integer data and the idempotent monoids; float sums are formed
 * in column-rank order by atomics (within rounding of the CSR kernel's, not bit-reproducible run to run).
 * Replaces mgpu::SpmvCsrBinary (backend/cuda/spmv.hpp:178-220) as the CSR kernel does. */
int grb_spmv_set_format(int fmt);
/* Under `auto` an orientation takes the column-sorted format once it has run this many products through the CSR
 * kernel (default 48, GRB_SPMV_CBAND_AFTER; 0 = at its first product): preparing the second copy costs about
 * 70 launches' worth of what it saves per launch, so a matrix multiplied a few dozen times never pays for it.
 * launches < 0 only queries.  Returns the previous value. */
int grb_spmv_set_reuse_threshold(int launches);
grb_info grb_spmv_format_info(grb_matrix A, int tran, int* in_use, int64_t* groups, int* bands, int* items,
                              int* hub_rows, int* iso, int64_t* bytes_per_launch);

/* Which order grb_sssp (and algorithm::sssp through the shadow header) relaxes in on eligible matrices:
 *   -1 (default)  the work-efficient near / far order (csrc/sssp_nearfar.hip) for graphs with fewer than 8 stored
 *                 entries per row whose weights are small non-negative integers -- distances AND the reported round
 *                 count are the reference's (graphblas/algorithm/sssp.hpp:53-90); everything else runs the
 *                 reference's synchronous rounds (csrc/sssp_persist.hip);
 *    0            always the synchronous rounds;
 *    1            near / far whenever the matrix is f32 with non-negative weights (distances identical; with
 *                 non-integer weights the reported round count may differ from the reference's).
 * A run whose round count would exceed the descriptor's max_niter, or that asks for per-round records
 * (--timing), always takes the synchronous rounds.  mode < -1 only queries.  Returns the mode in force;
 * the environment variable GRB_SSSP_NEARFAR sets the initial value. */
int grb_sssp_set_nearfar(int mode);
/* 0 if the last grb_sssp of this process produced its result with the synchronous rounds, else the number of
 * passes the near / far order took. */
int grb_sssp_last_order(void);
/* After a grb_sssp that ran the near / far order: {vertices expanded, out-edges relaxed, vertices marked dirty} summed
 * over its passes -- what that kernel's algorithmic bytes are priced on (bench.py, config 3). */
void grb_sssp_last_work(int64_t* out3);

/* Batched traversals = the multi-frontier product (extension; the reference leaves sparse x dense
 * mxm a stub, backend/cuda/operations.hpp:52-70, spmm.hpp:15-27): 1 <= k <= 64 sources traversed at
 * once, one 64-bit word per vertex (bit s = source s), levels as word-wide OR.  v[s] (k dense f32
 * vectors of size nrows) receive exactly the labels grb_bfs / grb_bfs_fused give for sources[s]
 * under the same descriptor (mxvmode forces a direction; max_niter caps the levels).
 * result->edges_traversed / reached are summed over the k traversals. */
grb_info grb_bfs_batch(grb_vector* v, int k, grb_matrix A, const grb_index* sources, grb_descriptor desc,
                       grb_bfs_result* result);
/* Levels in which every live source is pushed and at most `edges` out-edges leave the frontiers run inside one
 * co-resident launch, one grid barrier per level, instead of four kernels and a host round trip each (the first level,
 * the tail, every level of a high-diameter graph).  0: never; < 0: only query.  Returns the previous limit
 * (default 1 Mi; GRB_BATCH_TAIL=0 / GRB_BATCH_TAIL_EDGES set it from the environment).  Same labels either way. */
long long grb_bfs_batch_set_tail(long long edges);
/* The hot block grb_bfs_batch and the queue's sweep keep for A (built here if A has none yet): the hubs are the vertices of
 * out-degree >= *t, t the smallest threshold that leaves at most *cap of them (GRB_BATCH_HOT_MAX; GRB_BATCH_HOT=0: none),
 * in ascending id.  *H receives their number (0: A sweeps without a hot block), hubs[0 .. min(H, hubs_len)) their ids;
 * any of the pointers may be null. */
grb_info grb_bfs_batch_hot(grb_matrix A, long long* H, long long* t, long long* cap, grb_index* hubs, long long hubs_len);

/* One record per iteration of the last grb_sssp / grb_pr / grb_cc call on a descriptor: what the
 * reference's drivers print per iteration under --timing 1 (sssp.hpp:55-62, pr.hpp:53-62) or 2
 * (cc.hpp:61-71).  Kept when the descriptor's `timing` argument is non-zero. */
typedef struct {
  int32_t iteration;          /* 1-based                                                        */
  int32_t direction;          /* desc lastmxv_ after the iteration: GRB_PUSHONLY / GRB_PULLONLY */
  double  value;              /* sssp: f1.nvals (vertices improved); pr: error; cc: succ        */
  float   ms;                 /* time of the iteration ("gpu_tight")                            */
  int32_t reserved;
} grb_algo_iter;
/* Copies up to `cap` records into out (nullable); *count = records held (may exceed cap). */
grb_info grb_descriptor_iter_log(grb_descriptor desc, grb_algo_iter* out, int cap, int* count);

/* algorithm::sssp (algorithm/sssp.hpp:15-103): v = distances, FLT_MAX when unreachable.
 * Non-negative f32 weights run the same synchronous rounds in one launch (sssp_persist.hip);
 * anything else, or GRB_SSSP_FUSED=0, runs the reference's call sequence op by op. */
grb_info grb_sssp(grb_vector v, grb_matrix A, grb_index source, grb_descriptor desc,
                  grb_algo_result* result);
/* algorithm::pr (algorithm/pr.hpp:15-94): A must already be the scaled column-stochastic
 * matrix the driver prepares (example/gpr.cu:67-90). */
grb_info grb_pr(grb_vector p, grb_matrix A, float alpha, float eps, grb_descriptor desc,
                grb_algo_result* result);

/* algorithm::cc (algorithm/cc.hpp:17-136): FastSV; v and A are int; v = parent labels.  Per iteration the
 * MinimumSelectSecond product and ONE launch for the element-wise tail (cc.hpp:77-119: three eWiseAdd,
 * assignScatter, extractGather, eWiseMult, reduce, masked assign, two dup); grb_cc_set_fused(0) (or GRB_CC_FUSED=0
 * in the environment) runs the tail as the reference's call sequence instead; on < 0 only queries. */
grb_info grb_cc(grb_vector v, grb_matrix A, int seed, grb_descriptor desc, grb_algo_result* result);
int grb_cc_set_fused(int on);

/* algorithm::tc (algorithm/tc.hpp:15-54): A = lower triangle (int), B = buffer matrix.
 * The reference forms B<A> = A (+.x) A^T and reduces it (tc.hpp:38-43); B is its "buffer matrix" (tc.hpp:17) and is not
 * read again.  When A is a STRICTLY lower (or strictly upper) triangle whose stored values are all 1 -- the matrix the
 * reference's driver builds (example/gtc.cu) -- that sum is the number of triangles, which does not depend on which way the edges point:
 * the library then counts on the degree-ordered orientation of the same edges (csrc/tc_count.hip: every vertex keeps
 * the neighbours of higher degree, the lists are short, one end of every edge is looked up in an LDS bitmap of the other)
 * and LEAVES B AS IT WAS.  The orientation is prepared by the first count on a matrix and kept with it.  Any other
 * matrix or descriptor (INP0 transposed, ...), and every matrix after grb_tc_set_product(1) (or GRB_TC_PRODUCT=1 in the
 * environment), runs the reference's two calls with the product in B.  ntris is the same number either way. */
grb_info grb_tc(int64_t* ntris, grb_matrix A, grb_matrix B, grb_descriptor desc, grb_algo_result* result);
/* 0 (default): the count without the product where it is a count AND pays -- the first count asked of a matrix without
 * long rows (squared row lengths summing to at most 256 per entry: road networks, uniform random graphs, whose product is
 * cheap) goes through the product, the second prepares the orientation; 1: always the product in B; 2: the count wherever
 * it is a count; < 0: query.  Returns the previous setting.  GRB_TC_PRODUCT=<0|1|2> in the environment sets the start. */
int grb_tc_set_product(int on);
/* The orientation a matrix keeps after its first count (about 34 bytes per stored entry: the lists, a 16-byte descriptor
 * per edge end, the task lists) is released by grb_matrix_free and by whatever rewrites the matrix; this releases it
 * at once -- the next count prepares it again. */
grb_info grb_tc_release(grb_matrix A);
typedef struct {
  int32_t path;           /* of the last grb_tc: 0 = product + reduce, 1 = counted on the oriented lists            */
  float   prep_ms;        /* the orientation, when that call had to build it (0 when the matrix brought it along)    */
  float   count_ms;       /* the counting kernels                                                                  */
  int32_t longest_list;   /* the longest list of the orientation                                                   */
  int32_t tasks[3];       /* workgroups launched: a wave + hash table, 512 threads + bitmap, 512 threads + hash table */
} grb_tc_info;
grb_info grb_tc_last(grb_tc_info* out);

/* The DENSE CORE of that product (csrc/mxm_core.hip): the k_want longest rows of the lower triangle L (all rows of a
 * length or none) as K x K bit rows H, and C_H(i, j) = sum_k H[i][k] H[j][k] for the entries (i, j) of L between core
 * rows -- the part of C<L> = L (+.x) L^T (algorithm/tc.hpp:15-54, kernels/spgemm.hpp:17-79) in which the lists are
 * dense enough to be bit rows.  method 0: a lane per mask entry, AND + popcount over 32 columns at a time; method 1:
 * v_mfma_i32_16x16x64_i8 on 0/1 bytes expanded from the bit rows, every pair of a 128 x 128 tile computed and the mask
 * applied to the finished tile; method 2: MFMA for the tiles with at least dense_from mask entries (of 16 384), popcount
 * for the others.  count = sum of C_H over those entries; checksum = position-weighted sum of the per-entry results (equal
 * across methods only if every entry is).  No counterpart in the reference (SURVEY.md 8(f)2 sketches it). */
typedef struct {
  int32_t  core_rows;          /* K */
  int32_t  min_row_length;     /* rows of at least this many entries are core rows */
  int64_t  core_entries;       /* entries of L between core rows = results */
  int64_t  count;
  uint64_t checksum;
  float    build_ms;           /* HIP events: ranks, bit rows, prefix counts, tile list */
  float    product_ms;         /* HIP events: the product kernels alone */
  int32_t  tiles;              /* 128 x 128 tiles with at least one entry */
  int32_t  tiles_mfma;         /* ... of which the MFMA kernel took */
  int32_t  tiles_by_density[10];   /* those tiles by tenths of 16 384 entries */
} grb_tc_core_result;
grb_info grb_tc_dense_core(grb_matrix L, int k_want, int method, int dense_from, grb_tc_core_result* res);

/* k-truss and edge trussness (csrc/ktruss.hip).  The reference has no such driver (graphblas/algorithm/), so the
 * definitions are this header's own; they follow LAGraph's convention, the usual one.
 *
 * A is an n x n matrix with the same structure as its transpose.  Stored values are never read: only the structure counts,
 * so stored zeros are edges like any other.  Diagonal entries take no part and never appear in a result.  G is the simple
 * undirected graph of A's off-diagonal entries.  For k >= 2 the k-truss of G is the largest subgraph T in which every edge
 * lies in at least k - 2 triangles of T; it is unique.
 *
 * grb_ktruss(C, A, k, desc, result): C is n x n and holds both (i, j) and (j, i) for every edge of T, columns ascending in
 * every row; C(i, j) is the support of {i, j} in T, the number of common neighbours of i and j within T.  Rows that lose
 * everything stay as empty rows.  k = 2 returns all of G with its supports -- the only case in which stored supports may be
 * 0.
 *
 * grb_trussness(C, A, desc, result): C has G's structure, both directions, and C(i, j) is the largest k such that {i, j}
 * is in the k-truss: 2 for an edge in no triangle.
 *
 * Both: C's element type is GRB_I32 or GRB_F32, A's is either of the two, independently of C's.  C gets both orientations,
 * the CSC a copy of the CSR (the result is symmetric); a C of the CSR-only format aliases its CSC, as in the other
 * operations.  C may be A.  The same inputs give the same bits.  desc == NULL means the defaults; no descriptor field is
 * read.  result may be NULL.
 *
 * How: the working graph stays on the device for the whole call.  A round computes the support of every edge of what is
 * left -- every edge intersected once, by its endpoint with the longer list -- and drops the edges below k - 2; the call
 * ends when a round drops nothing.  grb_trussness runs the same rounds for k = 3, 4, ...: what a round drops at level k has
 * trussness k - 1, a round that drops nothing raises k, and the call ends when nothing is left.  The host reads one record
 * per round.
 *
 * Every error is found before anything of C is written, and C keeps what it held.  A null C or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, or C not n x n: GRB_DIMENSION_MISMATCH; k < 2: GRB_INVALID_VALUE; an element type
 * of A or C outside f32 / i32: GRB_NOT_IMPLEMENTED; an A without a CSC of its own (a product result): GRB_INVALID_OBJECT
 * -- the caller gets one with grb_transpose under GrB_INP0 = GrB_TRAN; an A whose CSR and CSC differ in pointers or
 * indices, i.e. one that is not symmetric, found by one comparison on the device: GRB_INVALID_VALUE; a failed device
 * allocation: GRB_OUT_OF_MEMORY.  In the CSR-only matrix format (GRB_SPARSE_MATRIX_FORMAT=1) the CSC IS the CSR, there is
 * nothing to compare and the caller vouches for the symmetry (an entry whose transposed entry is missing is still found,
 * as GRB_INVALID_VALUE). */
typedef struct {
  int32_t rounds;             /* filter rounds run (each reads one record back; the last of grb_ktruss drops nothing)   */
  int32_t supports;           /* support computations run (grb_trussness: fewer than rounds)                            */
  int64_t edges;              /* undirected edges of G                                                                 */
  int64_t result_edges;       /* undirected edges of the result (grb_trussness: those of G)                            */
  int32_t kmax;               /* grb_trussness: the largest k with a non-empty truss (2 when G has no edge); else the k given */
  float   loop_ms;            /* HIP-event time of the rounds                                                          */
} grb_truss_result;
grb_info grb_ktruss(grb_matrix C, grb_matrix A, int k, grb_descriptor desc, grb_truss_result* result);
grb_info grb_trussness(grb_matrix C, grb_matrix A, grb_descriptor desc, grb_truss_result* result);

/* Betweenness centrality (csrc/bc.hip): batched Brandes.  The reference has no such driver (graphblas/algorithm/), so the
 * definition is this header's own; it follows LAGraph's convention.
 *
 * A is n x n, f32 or i32.  Only the structure counts: stored values are never read and a stored zero is an edge.  A stored
 * A(i, j) with i != j is the edge i -> j, the direction grb_bfs walks; diagonal entries take no part.  The graph may be
 * directed: the structure need not be symmetric.  For a source s, sigma_s(v) is the number of shortest s -> v paths
 * (sigma_s(s) = 1), d_s(v) is v's depth, and
 *     delta_s(v) = sum over the edges v -> w with d_s(w) = d_s(v) + 1 of sigma_s(v) / sigma_s(w) * (1 + delta_s(w)),
 * with delta_s(s) = 0 and delta_s(v) = 0 for a v that s does not reach.  The result is bc(v) = the sum of delta_s(v) over
 * the sources.  No normalisation and no halving: with every vertex a source on a symmetric graph every unordered pair is
 * counted twice, as in LAGraph.  A source listed twice counts twice.
 *
 * grb_bc(bc, A, sources, ns, desc, result): sources is a host array of ns vertex ids; sources == NULL means every vertex
 * 0 .. n - 1 (exact centrality) and ns is ignored.  bc is an f32 vector of size n; it becomes dense with all n values
 * stored, exactly 0 for a vertex between no pair.  desc may be NULL; no descriptor field is read.  result may be NULL.
 *
 * The same inputs give the same bits.  Path counts and dependencies are f64 on the device; bc is accumulated in f64 over
 * all sources and rounded to f32 once, at the end.  Path counts beyond the f64 range (about 1.8e308 shortest paths between
 * one pair) make the result undefined; LAGraph has the same limit.
 *
 * How: the sources are taken 64 at a time, a lane of a wave each, on n x 64 arrays of depths and path counts.  One sweep
 * finds the depths (those grb_bfs_batch gives) and the list of vertices at every depth with the path counts right behind
 * each level; the dependencies come back level by level.  Both are gathers in stored order without floating-point
 * atomics.  Working memory: 16 n x 64 bytes.
 *
 * Every error is found before bc is written, and bc keeps what it held.  A null bc or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, or size(bc) != n: GRB_DIMENSION_MISMATCH; sources != NULL and ns < 1:
 * GRB_INVALID_VALUE; a source < 0 or >= n: GRB_INVALID_INDEX (as grb_bfs_batch); bc not f32, or A not f32 / i32:
 * GRB_NOT_IMPLEMENTED; an A without a CSC of its own (a product result): GRB_INVALID_OBJECT, as grb_ktruss; a failed
 * device allocation: GRB_OUT_OF_MEMORY.  In the CSR-only matrix format (GRB_SPARSE_MATRIX_FORMAT=1) the CSC IS the CSR and
 * the caller vouches for the symmetry. */
typedef struct {
  int32_t sources;            /* traversals run (n when sources == NULL)                                               */
  int32_t batches;            /* sweeps of up to 64 sources                                                            */
  int32_t levels;             /* largest depth reached by any source, + 1                                              */
  int64_t reached;            /* vertices reached, summed over the sources (each source reaches itself)                */
  float   loop_ms;            /* HIP-event time of all batches                                                         */
} grb_bc_result;
grb_info grb_bc(grb_vector bc, grb_matrix A, const grb_index* sources, int ns, grb_descriptor desc, grb_bc_result* result);

/* Community detection by label propagation (csrc/cdlp.hip): synchronous CDLP.  The reference has no such driver
 * (graphblas/algorithm/), so the definition is this header's own; it is Graphalytics' and LAGraph's.
 *
 * A is n x n, f32 or i32.  Stored values are never read: a stored zero is an edge.  Diagonal entries take no part.  N(v) is a
 * multiset.  directed == 0: the off-diagonal column ids stored in row v of A's CSR; for a matrix with symmetric structure
 * that is the undirected graph, the library does not check the symmetry, and an asymmetric A simply means "rows only".
 * directed == 1: those ids plus the off-diagonal row ids stored in column v, taken from the CSC; a vertex joined to v in
 * both directions is in N(v) twice, as in Graphalytics.
 *
 * L_0(v) = v when init == NULL, otherwise L_0 = init: an i32 vector of size n in either storage with all n values stored,
 * each in 0 .. n - 1.  L_t+1(v) = the smallest label among those with the largest multiplicity in { L_t(u) : u in N(v) },
 * and L_t+1(v) = L_t(v) when N(v) is empty.  Updates are synchronous: iteration t + 1 reads only L_t.  The call runs
 * iterations 1, 2, ... and stops after the first one that changes no label, or after max_iter, whichever comes first
 * (synchronous CDLP need not converge: a single edge swaps its two labels forever).
 *
 * grb_cdlp(labels, A, init, directed, max_iter, desc, result): labels is an i32 vector of size n; it becomes dense with all
 * n values stored.  labels may be init.  desc may be NULL; no descriptor field is read.  result may be NULL.  The same
 * inputs give the same bits.
 *
 * evaluated: a vertex is evaluated in iteration 1 when N(v) is non-empty, and in iteration t >= 2 when some u in N(v)
 * changed its label in iteration t - 1 -- otherwise its mode cannot have changed and is not computed.  evaluated is the
 * exact count of those (vertex, iteration) pairs.  After grb_cdlp_set_skip(0) every vertex with a non-empty N(v) is
 * evaluated in every iteration and evaluated = iterations x that count; labels, iterations, changed and communities are
 * identical either way.
 *
 * How: a label's count is kept under integer atomic adds that return the count before the add, so the largest count any
 * add saw (the smallest label on a tie) is the mode after ONE walk over the list.  Lists of up to 8 entries take eight
 * lanes, up to 64 a wave (no table: all pairs compared), up to 512 one wave and up to 2048 four waves with an LDS hash
 * table, longer ones 1024 threads with one of 32 to 256 count arrays of n words in global memory (as many as fit in 128 MiB).  A vertex whose label changed marks the vertices it
 * is a neighbour of in a bitmap (its CSC column, or both lists when directed == 1), from which the next iteration's work
 * lists are compacted; an A without a CSC of its own has every task look at its neighbours' "changed" bits first
 * instead.  The host reads one record per iteration (two in an iteration that ran without marks because the one before had
 * changed every vertex, and then did not change them all).  Working memory: 36 n bytes, and 4 n bytes per list longer than 2048
 * (for at most 256 of them and at most 128 MiB, but for 32 in any case).
 *
 * Every error is found before labels is written, and labels keeps what it held.  A null labels or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, or size(labels) != n, or size(init) != n: GRB_DIMENSION_MISMATCH; max_iter < 1,
 * or directed outside {0, 1}, or nvals(init) != n: GRB_INVALID_VALUE; an init value outside 0 .. n - 1 (found by one
 * reduction on the device): GRB_INVALID_INDEX; labels or init not i32, or A outside f32 / i32: GRB_NOT_IMPLEMENTED;
 * directed == 1 and an A without a CSC of its own (a product result, the CSR-only matrix format): GRB_INVALID_OBJECT, as
 * grb_ktruss; a failed device allocation: GRB_OUT_OF_MEMORY.  directed == 0 reads only the CSR of such a matrix, so it
 * works on a product result and in the CSR-only matrix format.  n = 0 or an A without entries is a success: labels = L_0,
 * iterations = 1, changed = 0. */
typedef struct {
  int32_t iterations;         /* iterations run, the one that changed nothing included                                 */
  int32_t changed;            /* vertices whose label the last iteration changed (0 = a fixed point)                   */
  int64_t evaluated;          /* (vertex, iteration) pairs whose mode was computed, see above                          */
  int32_t communities;        /* distinct labels in the result                                                         */
  float   loop_ms;            /* HIP-event time of the iterations                                                      */
} grb_cdlp_result;
grb_info grb_cdlp(grb_vector labels, grb_matrix A, grb_vector init, int directed, int max_iter, grb_descriptor desc, grb_cdlp_result* result);
int grb_cdlp_set_skip(int on);   /* 1 (default) / 0; < 0 queries; returns the previous setting */

/* The local clustering coefficient (csrc/lcc.hip).  The reference has no such driver (graphblas/algorithm/), so the
 * definition is this header's own; it is Graphalytics' and LAGraph's.
 *
 * A is n x n, f32 or i32.  Stored values are never read: a stored zero is an edge.  Diagonal entries take no part.
 *   E      = { (i, j) : A(i, j) stored, i != j }
 *   N(v)   = { u != v : (v, u) in E or (u, v) in E }, a SET: a vertex joined to v both ways is in it once (grb_cdlp's N(v)
 *            is a multiset and counts such a vertex twice; this one does not)
 *   d(v)   = |N(v)|
 *   num(v) = |{ (u, w) : u, w in N(v), u != w, (u, w) in E }|, the number of DIRECTED stored entries between neighbours of v
 *   lcc(v) = num(v) / (d(v) (d(v) - 1)) when d(v) >= 2, else exactly 0.
 * On a matrix with symmetric structure this is the usual 2 tri(v) / (d (d - 1)).  One formula serves both cases; directed
 * only says what the library may read and assume:
 *   directed == 0   A's structure is symmetric and only the CSR is read.  When A has a CSC of its own the symmetry is
 *                   checked by one comparison on the device, and an asymmetric A is GRB_INVALID_VALUE.  The verdict is
 *                   part of the call's one host read, so the whole computation has run by then: on an asymmetric A the
 *                   lists are not bounded by sqrt(2 entries) and the error may take far longer than a good call.  An A without a CSC
 *                   of its own (a product result, the CSR-only matrix format) is taken on the caller's word: nothing is
 *                   read or written out of bounds whatever its structure is, and the values are then unspecified.
 *   directed == 1   any structure; the CSR and the CSC are both read.  An A without a CSC of its own is
 *                   GRB_INVALID_OBJECT, as in grb_cdlp.
 *
 * grb_lcc(lcc, A, directed, desc, result): lcc is an f32 vector of size n; it becomes dense with all n values stored.  desc
 * may be NULL; no descriptor field is read.  result may be NULL.
 *
 * Arithmetic: num(v) and d(v) are exact integers, num in 64 bits (d (d - 1) exceeds 2^32 on a hub).  The value is the f64
 * quotient (double)num / ((double)d * (double)(d - 1)) rounded to f32 once; both operands are below 2^53, so the quotient
 * is the correctly rounded one.  The same inputs give the same bits, every time.
 *
 * How: with m(v, u) in {1, 2} = how many of (v, u) and (u, v) are stored, num(a) = the sum of m(b, c) over the triangles
 * {a, b, c} of the undirected graph.  The call builds that graph on the device, structure only: row v = N(v) ascending (CSR
 * row v merged with CSC column v when directed == 1), every entry with the bit m - 1 on top of its 32-bit index.  Every
 * vertex keeps the neighbours that rank above it by (d, id) -- no list is longer than sqrt(2 entries) -- and every
 * triangle is enumerated ONCE: per edge the end with the longer list is the pivot, its list goes into an LDS hash table
 * (2048 entries at a time; a longer list in slices) and the other end's list is streamed past it, 16 bytes a lane.  A
 * found triangle credits its three corners in registers and in 32-bit LDS counters beside the table's slots, which are
 * flushed with one 64-bit integer atomic add per non-zero slot: no global atomic per triangle and no floating-point
 * atomic.  Pivots with lists of up to 256 entries are a wave's task, longer ones a workgroup's, 256 / 1024 partners a
 * task; the task lists come from counts, one scan and a fill.  Everything is carved from one allocation before the first
 * kernel and freed before the call returns; the host reads one record.  Working memory: 12.1 bytes per stored entry
 * (directed == 1: 24.2) and 88 bytes per vertex.  A matrix with 2 nvals (directed == 0: nvals) + 4 n >= 2^32 - 16 is
 * beyond the 32-bit positions of that memory: GRB_OUT_OF_MEMORY.
 *
 * Every error is found before lcc is written, and lcc keeps what it held.  A null lcc or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, or size(lcc) != n: GRB_DIMENSION_MISMATCH; directed outside {0, 1}:
 * GRB_INVALID_VALUE; lcc not f32, or A outside f32 / i32: GRB_NOT_IMPLEMENTED; directed == 1 and an A without a CSC of its
 * own: GRB_INVALID_OBJECT; directed == 0 and an A whose CSC differs from its CSR: GRB_INVALID_VALUE; a failed device
 * allocation: GRB_OUT_OF_MEMORY.  n = 0, or an A without off-diagonal entries, is a success: all zeros and a zero record. */
typedef struct {
  int64_t edges;              /* unordered pairs {u, v}, u != v, joined in either direction                            */
  int64_t triangles;          /* triangles of that undirected graph                                                    */
  int64_t closed;             /* sum of num(v) over all v                                                              */
  int64_t wedges;             /* sum of d(v) (d(v) - 1) over all v; closed / wedges is the transitivity                */
  int32_t max_degree;         /* largest d(v)                                                                          */
  float   loop_ms;            /* HIP-event time of the call's device work                                              */
} grb_lcc_result;
grb_info grb_lcc(grb_vector lcc, grb_matrix A, int directed, grb_descriptor desc, grb_lcc_result* result);

/* The k-core decomposition (csrc/kcore.hip): grb_coreness and grb_kcore.  The reference has no such driver
 * (graphblas/algorithm/), so the definition is this header's own; it is LAGraph's and Gunrock's, and the vertex counterpart
 * of grb_trussness / grb_ktruss.
 *
 * A is n x n, f32 or i32, with the same structure as its transpose.  Stored values are never read: a stored zero is an
 * edge.  Diagonal entries take no part.
 *   G       = the simple undirected graph of A's off-diagonal entries
 *   d(v)    = v's degree in G
 *   k-core  = for k >= 0 the largest subgraph of G in which every vertex has at least k neighbours inside the subgraph; it
 *             is unique
 *   core(v) = the largest k such that v is in the k-core
 *   kmax    = max core(v), the degeneracy; 0 for a graph without edges.
 *
 * grb_coreness(core, A, desc, result): core is an i32 vector of size n; it becomes dense with all n values stored: core(v),
 * and 0 for an isolated vertex.
 * grb_kcore(v, A, k, desc, result): v is an i32 vector of size n; it becomes dense.  v(x) = the number of x's neighbours
 * inside the k-core when x is in it (that is >= k), and 0 when it is not: the vertex analogue of grb_ktruss storing
 * supports.  k = 0 gives the plain degrees; k > kmax is a success with all zeros and result_vertices = 0.
 * Both: desc may be NULL; no descriptor field is read.  result may be NULL.  The same inputs give the same bits: core numbers
 * and in-core degrees are unique, so this holds whatever order the device peels in.  rounds is the one field that may
 * depend on scheduling.
 *
 * Structure (the rule of grb_lcc with directed == 0): only the CSR is read.  When A has a CSC of its own the symmetry is
 * checked by one comparison on the device before the peel, and an asymmetric A is GRB_INVALID_VALUE.  An A without a CSC of
 * its own (a product result, the CSR-only matrix format) is taken on the caller's word: nothing is read or written out of
 * bounds whatever its structure is, and the values are then unspecified.
 *
 * How: the peel loop lives on the device, in ONE co-resident launch of a 1024-thread workgroup per CU whose passes are
 * separated by a grid barrier with bounded spins; the host reads one record at the end, so launches does not grow with
 * the rounds or the levels.  State: the current degrees (row length minus a stored diagonal) and ONE queue that holds
 * every vertex in the order of its removal -- the frontier of a round is the part of it the round before appended.  A
 * level is the smallest degree left: the pass that lists a level's first frontier also takes the minimum, the number and
 * the degree sum of the vertices left, so an empty level costs nothing and the vertices left when the last level opens
 * are the kmax-core.  Removing a vertex walks its row (a lane for rows of up to 8 entries, a wave with 16-byte index
 * loads up to 2048, the workgroup beyond): a neighbour whose degree is still above the level gets one returning integer
 * atomic decrement; the thread that sees level + 1 come back appends it, a thread that sees less undoes its decrement,
 * so a degree never settles below its vertex's level and every vertex is appended exactly once.  Appends are staged per
 * wave in LDS and reserved with one atomic per batch.  grb_kcore is the same kernel with the one level k - 1 and a last
 * pass that zeroes what fell.  Working memory: 8 bytes per vertex and 2.25 KiB, one allocation made before the first kernel
 * and freed before the call returns; nothing is allocated inside the loop.
 *
 * Every error is found before the output is written, and the output keeps what it held.  A null output or A, or an unbuilt
 * A: GRB_UNINITIALIZED_OBJECT; A not square, or size(output) != n: GRB_DIMENSION_MISMATCH; k < 0: GRB_INVALID_VALUE; output
 * not i32, or A outside f32 / i32: GRB_NOT_IMPLEMENTED; an A whose own CSC differs from its CSR: GRB_INVALID_VALUE; a failed
 * device allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up: GRB_PANIC, as in the other one-launch drivers.  n = 0,
 * or an A without off-diagonal entries, is a success: all zeros, kmax = 0, and levels = 1 when n > 0. */
typedef struct {
  int64_t edges;            /* undirected edges of G                                                               */
  int64_t result_edges;     /* grb_coreness: edges inside the kmax-core; grb_kcore: edges inside the k-core        */
  int32_t kmax;             /* grb_coreness: the degeneracy; grb_kcore: the k given                                */
  int32_t levels;           /* grb_coreness: distinct values of core(v); grb_kcore: 1                              */
  int32_t result_vertices;  /* grb_coreness: vertices with core(v) == kmax; grb_kcore: vertices of the k-core      */
  int32_t rounds;           /* grid-wide peeling passes the device ran: implementation-defined, for the bench only */
  int32_t launches;         /* kernel launches of the peel itself: 1                                               */
  float   loop_ms;          /* HIP-event time of the call's device work                                            */
} grb_kcore_result;          /* 40 bytes */
grb_info grb_coreness(grb_vector core, grb_matrix A, grb_descriptor desc, grb_kcore_result* result);
grb_info grb_kcore(grb_vector v, grb_matrix A, int k, grb_descriptor desc, grb_kcore_result* result);

/* The strongly connected components (csrc/scc.hip): grb_scc.  The reference has no such driver (graphblas/algorithm/), so
 * the definition is this header's own; it is the textbook's, and the directed counterpart of grb_cc.
 *
 * A is n x n, f32 or i32.  Stored values are never read: a stored zero is an edge.  Diagonal entries take no part.
 *   E      = { (i, j) : A(i, j) stored, i != j }: the directed graph
 *   u ~ v  when a directed path runs from u to v and one from v to u, or u = v.  The classes of ~ are the strongly connected
 *            components
 *   scc(v) = the smallest vertex number in v's component.
 * That label is unique, so the same inputs give the same bits whatever order the device works in, and A and its transpose
 * give the same vector.
 *
 * grb_scc(scc, A, desc, result): scc is an i32 vector of size n; it becomes dense with all n values stored.  desc may be
 * NULL; no descriptor field is read: the components of the transpose are those of A.  result may be NULL.  On a symmetric
 * structure the result is the connected components, labelled by their smallest member.
 *
 * Structure (the rule of grb_lcc and grb_cdlp with directed = 1): the CSR (out-edges) and the CSC (in-edges) are both read.
 * An A without a CSC of its own (a product result, the CSR-only matrix format) is GRB_INVALID_OBJECT.
 *
 * How: the whole computation is ONE co-resident launch of a 1024-thread workgroup per CU (GRB_NUM_CU is honoured) whose
 * passes are separated by a grid barrier with bounded spins; the host reads one record at the end, so launches is 1 whatever
 * the graph.  Everything works on the live vertices, those without a label yet, in three phases.
 *   1. Trim.  A live vertex with no live in-neighbour or no live out-neighbour is a component of its own.  The live in- and
 *      out-degrees start as column and row length minus a stored diagonal.  ONE queue holds every vertex in the order of
 *      its removal; the frontier of a pass is what the pass before appended.  Removing v gives every live out-neighbour one
 *      returning integer atomic decrement of its in-degree and every live in-neighbour one of its out-degree; the thread
 *      that sees a degree reach 0 claims the vertex with one atomic on its state word, so it is appended exactly once though
 *      both degrees may get there.  Trimming runs to its fixpoint; it alone finishes every acyclic graph.
 *   2. The giant component.  The pivot is the live vertex with the largest live in-degree x live out-degree (64 bits), the
 *      smallest number on a tie.  A forward sweep over rows marks what it reaches; a backward sweep over columns that stays
 *      inside the marked set removes what it reaches: the pivot's component.  Its smallest number is taken with a wave
 *      reduction and one atomic per wave and written as the label.  Both sweeps are level-synchronous plain pushes over a
 *      queue.  Trimming runs again.
 *   3. Colouring rounds until no vertex is live.  colour(v) = v on the live vertices; the minimum travels along live edges
 *      to a fixpoint (a vertex whose colour dropped is queued, once per pass, by a bit of its state word; its neighbours
 *      get atomicMin).  The live vertices with colour(r) = r are the roots, each the smallest member of its own component,
 *      so the label needs no reduction.  From all roots at once a sweep against the direction that stays inside the colour
 *      removes every root's component, and trimming runs again.  Even rounds colour along rows and collect along columns,
 *      odd rounds the other way round, so that a one-way chain of small components costs a single round one way or the
 *      other.  The smallest live vertex is always a root, so every round removes a component and n rounds bound the loop;
 *      the worst case stays quadratic in passes on adversarial inputs.
 * Rows and columns are walked by a lane up to 8 entries, a wave with 16-byte index loads up to 2048, the workgroup beyond.
 * Appends are staged per wave in LDS and reserved with one atomic per batch.  Working memory: 24 bytes per vertex (state
 * word, two degrees, colour, the queue and one more frontier) and 2 KiB, one allocation made before the kernel and freed
 * before the call returns; nothing is allocated inside the loop and nothing is proportional to nvals.
 *
 * edges, components, largest and trivial are exact and do not depend on scheduling; trimmed, rounds and passes may, and
 * are for the bench only.
 *
 * Every error is found before scc is written, and scc keeps what it held: values, sparsity and caller-owned storage alike.
 * A null scc or A, or an unbuilt A: GRB_UNINITIALIZED_OBJECT; A not square, or size(scc) != n: GRB_DIMENSION_MISMATCH; scc
 * not i32, or A outside f32 / i32: GRB_NOT_IMPLEMENTED; an A without a CSC of its own: GRB_INVALID_OBJECT; a failed device
 * allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up: GRB_PANIC, as in the other one-launch drivers.  n = 0 is a
 * success with a zero record.  An A without off-diagonal entries is a success with scc(v) = v, components = trivial = n,
 * and largest = 1 when n > 0. */
typedef struct {
  int64_t edges;        /* |E|: stored off-diagonal entries                                                   */
  int32_t components;   /* number of components; n for an acyclic graph                                       */
  int32_t largest;      /* vertices of the largest component; 0 when n = 0                                    */
  int32_t trivial;      /* components of exactly one vertex                                                   */
  int32_t trimmed;      /* vertices settled by trimming: implementation-defined, for the bench only           */
  int32_t rounds;       /* colouring rounds (above): implementation-defined, for the bench only               */
  int32_t passes;       /* grid-wide passes the device ran: implementation-defined, for the bench only        */
  int32_t launches;     /* kernel launches of the loop itself: 1                                              */
  float   loop_ms;      /* HIP-event time of the call's device work                                           */
} grb_scc_result;        /* 40 bytes */
grb_info grb_scc(grb_vector scc, grb_matrix A, grb_descriptor desc, grb_scc_result* result);

/* The minimum spanning forest (csrc/msf.hip): grb_msf.  The reference has no such driver (graphblas/algorithm/), so the
 * definition is this header's own; LAGraph ships the algorithm as LAGraph_msf.  It is the one driver beside SSSP that reads
 * the stored values.
 *
 * A is n x n, f32 or i32, symmetric in structure and in values: A(i, j) and A(j, i) are both stored and equal.  Diagonal
 * entries take no part.  A stored zero is an edge of weight 0.  The weights ARE read.
 *   G     = the simple undirected weighted graph of A's off-diagonal entries
 *   key   = (w, min(u, v), max(u, v)) of the edge {u, v} of weight w, compared lexicographically: a total order of the edges.
 *           For i32, w is compared as a signed integer.  For f32, w is compared by value: -0.0 and +0.0 are the same weight,
 *           +-inf are allowed, and a NaN anywhere off the diagonal is GRB_INVALID_VALUE
 *   MSF   = the minimum spanning forest under that total order.  It is unique: it is the forest Kruskal builds when it takes
 *           the edges in key order.
 * It depends on no scheduling: the same inputs give the same bits.  A relabelled graph gives the relabelled forest only up to
 * the tie-break (the key holds vertex numbers), so nothing more may be expected on ties.
 *
 * grb_msf(C, comp, A, desc, result):
 *   C      n x n and of A's element type; any other type is GRB_DOMAIN_MISMATCH.  C receives both directions of every forest
 *          edge with its weight: columns ascending, empty rows for isolated vertices.  The CSC is a copy of the CSR, unless C
 *          is in the CSR-only format.  C may be A.  The stored weight is A's bits for that entry; a -0.0 stays -0.0, taken
 *          from the row of min(u, v).
 *   comp   may be NULL.  Otherwise an i32 vector of size n that becomes dense: comp(v) = the smallest vertex number in v's
 *          connected component, which is what grb_scc returns on a symmetric structure.
 *   desc   may be NULL; no descriptor field is read.  result may be NULL.
 * weight: for i32 the exact 64-bit integer sum, converted once to double.  For f32 an f64 sum taken in a fixed order over C's
 * stored entries above the diagonal (each edge once): blocks of partial sums whose shape depends only on n and forest_edges,
 * no floating-point atomics, so the bits repeat.
 *
 * Structure (the rule of grb_kcore): only the CSR is read.  When A has a CSC of its own, one comparison on the device before
 * the loop checks the CSR against the CSC: pointers, indices and also values, compared as bits after -0 has been mapped to
 * +0 (f32); a mismatch is GRB_INVALID_VALUE.  An A without a CSC of its own (a product result, the CSR-only matrix format) is
 * taken on the caller's word: whatever it holds, nothing is read or written out of bounds and the call returns -- the rounds
 * are bounded by 32, every pointer-jumping loop is bounded and forest appends are clamped to n - 1 -- and the output is then
 * unspecified.  The NaN scan runs in both cases: the first round reads every off-diagonal value.
 *
 * How: Boruvka, as ONE co-resident launch of a 1024-thread workgroup per CU (GRB_NUM_CU is honoured) whose passes are
 * separated by a grid barrier with bounded spins; the host reads one record at the end, so launches is 1 whatever the graph.
 * State per vertex: the representative of its component, a parent word, a 64-bit best key and a 32-bit second word per
 * component, the position of the vertex's candidate (or "finished"), and the forest list of (vertex, CSR position).  A round:
 *   A. Every unfinished vertex walks its row (a lane for rows of up to 8 entries, a wave with 16-byte index loads up to 2048,
 *      the workgroup beyond) and keeps the smallest key among the entries whose other end lies in another component; for a
 *      fixed vertex the key order is the order of (w, other end), one 64-bit compare.  A vertex all of whose neighbours share
 *      its component is finished and never walked again: components only merge.  The candidate gets one 64-bit atomicMin of
 *      (ordered weight bits << 32 | min endpoint) at its component's slot; the ordered bits are the usual monotone map for
 *      f32 with -0 canonicalised, a sign flip for i32.
 *   B. The vertices whose candidate equals the slot take a 32-bit atomicMin of the max endpoint.
 *   C. Exactly one vertex per component matches all three, and it owns the component's edge.  Ties are never broken by CSR
 *      position: the two directions of an edge sit at different positions.  Under a total order the only hook cycles are
 *      mutual pairs, two components that chose the same edge: the smaller representative stays root and alone appends the
 *      edge; otherwise the hooking component appends it.  Appends are staged per wave in LDS and reserved with one atomic per
 *      batch.
 *   D. Pointer jumping to the fixpoint: up to 16 parents a vertex and pass, at most 40 passes.
 *   E. comp(v) = parent(comp(v)); the slots are reset.
 * The loop stops when no vertex has a candidate or a round hooks nothing.  Then comp(v) becomes the smallest member (one
 * atomicMin per vertex at its root and a relabelling pass).  After the loop the forest list is expanded to both directions
 * and ordered by the library's radix sort on (row, column) -- a star's forest row is as long as the star, so rows are not
 * sorted one by one -- the pointers are a lower bound per row, and the weight is summed as above.  Working memory: 56 bytes
 * per vertex and 4.3 KiB, one allocation made before the kernel and freed before the call returns; nothing is allocated
 * inside the loop and nothing is proportional to nvals.  The sort after the loop brings 24 bytes per vertex of its own.
 *
 * edges, forest_edges, weight, components and isolated are exact and do not depend on scheduling; rounds and passes are for
 * the bench only.
 *
 * Every error is found before C or comp is written, and both keep what they held.  A null C or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, C not n x n, or size(comp) != n: GRB_DIMENSION_MISMATCH; A outside f32 / i32, or comp
 * not i32: GRB_NOT_IMPLEMENTED; C not of A's type: GRB_DOMAIN_MISMATCH; an asymmetric A (structure or values), or a NaN off the
 * diagonal: GRB_INVALID_VALUE; a failed device allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up: GRB_PANIC, as in the
 * other one-launch drivers.  n = 0 is a success with a zero record.  An A without off-diagonal entries is a success with an
 * empty C, comp(v) = v, components = isolated = n and weight 0. */
typedef struct {
  int64_t edges;         /* undirected edges of G                                                    */
  int64_t forest_edges;  /* edges of the forest = n - components                                     */
  double  weight;        /* sum of the forest's weights                                              */
  int32_t components;    /* connected components of G, isolated vertices included                    */
  int32_t isolated;      /* vertices without an off-diagonal entry                                   */
  int32_t rounds;        /* Boruvka rounds: implementation-defined, for the bench only               */
  int32_t passes;        /* grid-wide passes the device ran: implementation-defined, bench only      */
  int32_t launches;      /* kernel launches of the loop itself: 1                                    */
  float   loop_ms;       /* HIP-event time of the call's device work                                 */
} grb_msf_result;         /* 48 bytes */
grb_info grb_msf(grb_matrix C, grb_vector comp, grb_matrix A, grb_descriptor desc, grb_msf_result* result);

/* Greedy weighted and maximal matching (csrc/matching.hip): grb_matching.  The reference has no such driver
 * (graphblas/algorithm/), so the definition is this header's own; LAGraph ships the algorithm as LAGraph_MaximalMatching.
 *
 * A is n x n, f32 or i32, symmetric.  Diagonal entries take no part.  G is the simple undirected graph of the off-diagonal
 * entries.  Every edge {u, v} has a key (p, min(u, v), max(u, v)), compared lexicographically: a total order of the edges.
 * mode selects p:
 *   GRB_MATCH_HEAVIEST = 0   p orders by descending weight, heaviest first.  i32 weights are compared as signed integers.  f32
 *                            weights are compared by value: -0.0 and +0.0 are the same weight, +-inf are allowed, and a NaN
 *                            off the diagonal is GRB_INVALID_VALUE.  A stored zero or a negative weight is an edge like any
 *                            other.
 *   GRB_MATCH_LIGHTEST = 1   the same, ascending.
 *   GRB_MATCH_HASHED   = 2   structure only: the values are never compared, a NaN is fine.  p = mix(mix(min + seed) ^ max) in
 *                            32-bit unsigned arithmetic, where mix(x) is x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13;
 *                            x *= 0xc2b2ae35; x ^= x >> 16.  The smaller p goes first.  seed is ignored in the other modes.
 * The matching M is the one the greedy scan builds: take the edges in key order and keep an edge when both ends are still
 * free.  M is unique, and it is maximal: no edge of G has two free ends.  In mode 0 its weight is at least half the maximum
 * weight matching's, when the weights are non-negative.  In mode 2 it is a maximal cardinality matching with random-looking
 * priorities, reproducible from seed.  It depends on no scheduling: the same inputs give the same bits.
 *
 * grb_matching(mate, C, A, mode, seed, desc, result):
 *   mate   an i32 vector of size n.  It becomes dense: mate(v) = v's partner, or -1.
 *   C      may be NULL.  Otherwise n x n and of A's element type; any other type is GRB_DOMAIN_MISMATCH.  C receives both
 *          directions of every matched edge, at most one entry a row.  Both directions hold A's bits from the row of
 *          min(u, v), as in grb_msf.  The CSC is a copy of the CSR, unless C is in the CSR-only format.  C may be A.
 *   desc   may be NULL; no descriptor field is read.  result may be NULL.
 * weight follows grb_msf's rule: for i32 the exact 64-bit integer sum, converted once to double.  For f32 an f64 sum taken in
 * a fixed order over the matched entries above the diagonal (each edge once): blocks of partial sums whose shape depends on
 * n alone, no floating-point atomics, so the bits repeat.  In mode 2 it is the same sum of the stored values.
 *
 * Symmetry follows grb_msf's rule: only the CSR is read.  When A has a CSC of its own, one comparison on the device before
 * the loop checks the CSR against the CSC: pointers and indices, and in modes 0 and 1 also values, compared as bits after -0
 * has been mapped to +0 (f32); a mismatch is GRB_INVALID_VALUE.  An A without a CSC of its own (a product result, the
 * CSR-only matrix format) is taken on the caller's word: whatever it holds, nothing is read or written out of bounds and the
 * call returns -- a round that matches nothing is the last, so the rounds are bounded by n / 2 + 1, and the appends to the
 * queue and to the list of the matched are clamped to n -- and the output is then unspecified.  The NaN scan of modes 0 and
 * 1 runs in both cases: the first round reads every off-diagonal value.
 *
 * How: the locally dominant edge algorithm.  An edge that is the best live edge at both of its ends is in the greedy matching
 * of what is left.  ONE co-resident launch of a 1024-thread workgroup per CU (GRB_NUM_CU is honoured) whose passes are
 * separated by a grid barrier with bounded spins; the host reads one record at the end, so launches is 1 whatever the graph.
 * State per vertex: mate, the other end and the CSR position of its best live entry (or "finished"), one queue of vertices to
 * evaluate and one list of the matched.  A round:
 *   A. Every queued vertex (in the first round: every vertex with a neighbour) walks its row (a lane for rows of up to 8
 *      entries, a wave with 16-byte index loads up to 2048, the workgroup beyond) for the smallest 64-bit (ordered p << 32 |
 *      other end) among the entries whose other end has no partner; for a fixed vertex that is the order of the key.  The
 *      ordered bits are the usual monotone map for f32 with -0 canonicalised, a sign flip for i32, complemented in mode 0.
 *      No atomic: the walker owns its candidate.  A vertex with no free neighbour is finished for good.
 *   B. Every evaluated v with cand(cand(v)) = v is matched.  Either end or both may see the pair; each end is claimed by one
 *      compare-and-swap of its mate, and the claimer appends it to the list, so a vertex enters the list exactly once.
 *   C. Every newly matched x walks its row and queues each free neighbour y with cand(y) = x.  A vertex whose candidate is
 *      still free keeps it and is not walked again: 1.3 to 1.7 evaluations a vertex measured on paths, grids and RMAT
 *      graphs with random or hashed keys.
 * Appends are staged per wave in LDS and reserved with one atomic per batch.  The loop stops when the queue is empty or a
 * round matched nothing.  The worst case is equal weights, where the key falls back to vertex numbers: a path then takes
 * n / 2 rounds of three barrier-bound passes.  After the loop C needs no sort: pointers = a scan of (mate >= 0), index =
 * mate, value = the stored position's bits.  Working memory: 24 bytes per vertex and about 3 KiB, one allocation made before
 * the kernel and freed before the call returns; nothing is allocated inside the loop and nothing is proportional to nvals.
 *
 * edges, matched, weight, exposed and isolated are exact and do not depend on scheduling; rounds, passes and evaluations are
 * for the bench only.
 *
 * Every error is found before mate or C is written, and both keep what they held.  A null mate or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, size(mate) != n, or C not n x n: GRB_DIMENSION_MISMATCH; A outside f32 / i32, or mate
 * not i32: GRB_NOT_IMPLEMENTED; C not of A's type: GRB_DOMAIN_MISMATCH; mode outside 0..2, an asymmetric A, or a NaN off the
 * diagonal in modes 0 and 1: GRB_INVALID_VALUE; a failed device allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up:
 * GRB_PANIC, as in the other one-launch drivers.  n = 0 is a success with a zero record.  An A without off-diagonal entries
 * is a success with mate = -1 everywhere and an empty C. */
#define GRB_MATCH_HEAVIEST 0
#define GRB_MATCH_LIGHTEST 1
#define GRB_MATCH_HASHED 2
typedef struct {
  int64_t edges;         /* undirected edges of G                                                    */
  int64_t matched;       /* edges of M                                                               */
  double  weight;        /* sum of the matched edges' stored values                                  */
  int32_t exposed;       /* vertices with a neighbour but no partner                                 */
  int32_t isolated;      /* vertices without an off-diagonal entry                                   */
  int32_t rounds;        /* rounds of the loop: implementation-defined, for the bench only           */
  int32_t passes;        /* grid-wide passes the device ran: implementation-defined, bench only      */
  int32_t evaluations;   /* rows walked for a candidate: implementation-defined, bench only          */
  int32_t launches;      /* kernel launches of the loop itself: 1                                    */
  float   loop_ms;       /* HIP-event time of the call's device work                                 */
} grb_matching_result;    /* 56 bytes */
grb_info grb_matching(grb_vector mate, grb_matrix C, grb_matrix A, int mode, uint32_t seed, grb_descriptor desc,
                      grb_matching_result* result);

/* Graph contraction (csrc/contract.hip): grb_relabel and grb_contract.  The reference has no such driver
 * (graphblas/algorithm/), so the definitions are this header's own; LAGraph ships the operation as LAGraph_Coarsen_Matching,
 * cuGraph as coarsen_graph, networkx as quotient_graph / condensation.  They consume what grb_cc, grb_scc, grb_msf (comp),
 * grb_cdlp, grb_coreness and grb_matching produce: a partition of the vertices as a vector.
 *
 * grb_relabel(map, labels, kind, count, desc): the dense ranking of a label vector.
 *   labels  an i32 vector of size n, in either storage, with all n values stored (grb_cdlp's rule for init).
 *   kind    GRB_RELABEL_LABELS = 0   every value is in 0 .. n - 1, and L(v) = labels(v).
 *           GRB_RELABEL_MATE   = 1   every value is in -1 .. n - 1, and L(v) = v when labels(v) < 0, otherwise
 *                                    min(v, labels(v)): what grb_matching writes, so a matched pair shares a label and an
 *                                    unmatched vertex keeps its own.  The involution is not checked; the rule is applied as
 *                                    written.
 *   map     an i32 vector of size n.  It becomes dense: map(v) = the number of distinct values of L smaller than L(v), so the
 *           coarse ids ascend with the labels.  map may be labels.
 *   count   nullable: the number of distinct values of L, nc.      desc may be NULL; no field is read.
 * How: one word per possible label set where the label is in use, the library's exclusive scan, a gather.  The host reads nc
 * and the range check's flag in one wait.  The same inputs give the same bits.
 * Errors are found before map is written.  A null handle: GRB_UNINITIALIZED_OBJECT; sizes differ: GRB_DIMENSION_MISMATCH; not
 * i32: GRB_NOT_IMPLEMENTED; nvals(labels) != n, or kind outside {0, 1}: GRB_INVALID_VALUE; a value out of range, found by one
 * reduction on the device: GRB_INVALID_INDEX; a failed device allocation: GRB_OUT_OF_MEMORY.  n = 0: success, count 0.
 *
 * grb_contract(C, sizes, A, map, op, loops, desc, result): the quotient graph C = S^T A S with S(v, map(v)) = 1.
 *   A       n x n, f32 or i32, any structure (directed is fine).  Only the CSR is read, so a product result and the CSR-only
 *           matrix format work.  Stored zeros are entries.
 *   map     an i32 vector of size n with all n values stored, each in -1 .. nc - 1, where nc is C's own shape: C is nc x nc.
 *           map(v) = -1 drops vertex v with every entry of its row and column.  Anything else out of range is
 *           GRB_INVALID_INDEX, checked on the device before anything is written.  A raw label vector therefore works with an
 *           n x n C (the rows of unused labels stay empty), a grb_relabel result with an nc x nc C.
 *   loops   0 drops every entry with map(i) = map(j) (the condensation, a coarsening step); 1 keeps them (the community
 *           graph).
 *   C       of A's type, else GRB_DOMAIN_MISMATCH.  C(a, b) is stored exactly when some stored A(i, j) has map(i) = a and
 *           map(j) = b and survives loops.  Columns ascend in every row.  C gets its CSR, and a CSC made by transposing that
 *           CSR on the device (the path behind grb_transpose): the same entries and bits, never a second fold.  A C of the
 *           CSR-only format aliases its CSC as in every other operation.  C may be A when nc = n.
 *   op      how the contributions to one C(a, b) are combined, a grb_binary_op; any but these four is GRB_NOT_IMPLEMENTED:
 *           GRB_OP_PLUS      i32: two's-complement wrap-around.  f32: an f64 sum rounded to f32 once, taken in an order that
 *                            is a function of the inputs alone, not of GRB_NUM_CU or of scheduling: up to 32 contributions in
 *                            the order of (i, j); more, in pieces of 2048 consecutive contributions, inside a piece 64
 *                            interleaved partial sums joined by a fixed butterfly, the pieces' sums joined the same way.  No
 *                            floating-point atomic, so the bits repeat.
 *           GRB_OP_MINIMUM / GRB_OP_MAXIMUM   i32 as signed integers; f32 in the total order of the usual monotone map of the
 *                            bits: -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.  The winner's bits are copied, so no
 *                            order of evaluation can show.
 *           GRB_OP_FIRST     the bits of the contributing entry with the smallest (i, j).
 *   sizes   nullable: an i32 vector of size nc.  It becomes dense: sizes(a) = |{v : map(v) = a}|.
 *   desc    may be NULL; no descriptor field is read.  result may be NULL.
 * How: one sort-based path for every operator and every coarse row, in a fixed number of plain launches -- no level loop, no
 * grid barrier.  Every stored entry gets the key (map(i) << cb | map(j)), cb = the bits of nc, and its CSR position as
 * payload; an entry that does not survive gets a key above all others.  The library's stable radix sort over the 2 cb bits
 * that matter brings the contributions of one (a, b) together, still in the order of (i, j).  Head flags and the library's scan
 * number the runs; their total is nvals(C).  C's row pointers are a search per coarse row, the fold is a lane per run, and a
 * run of more than 32 contributions is cut into pieces of 2048 folded by a wave each, so that "everything collapses into one
 * entry" is 8192 pieces for sixteen million contributions and not a serial chain.  The host waits twice: for the range check
 * with the counts, and for nvals(C).  Every index read from map or from A is checked against its array before it is used, so
 * nothing is read or written out of bounds whatever map holds.  Working memory: about 24 bytes per stored entry of A in one
 * allocation made up front, beside the sort's own 12 bytes per entry and the transposition's.
 *
 * kept, loops, entries, clusters, dropped and largest are exact and do not depend on scheduling; launches and loop_ms are for
 * the bench only.
 *
 * Every error is found before C or sizes is written, and both keep what they held.  A null C, A or map, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, C not square, size(map) != n, or size(sizes) != nc: GRB_DIMENSION_MISMATCH; A outside
 * f32 / i32, or map / sizes not i32: GRB_NOT_IMPLEMENTED; C not of A's type: GRB_DOMAIN_MISMATCH; an operator outside the four:
 * GRB_NOT_IMPLEMENTED; loops outside {0, 1}, or nvals(map) != n: GRB_INVALID_VALUE; a map value out of range:
 * GRB_INVALID_INDEX; a failed device allocation: GRB_OUT_OF_MEMORY.  n = 0, nc = 0 or an A without entries: success with an
 * empty C. */
#define GRB_RELABEL_LABELS 0
#define GRB_RELABEL_MATE 1
typedef struct {
  int64_t kept;          /* entries of A with both ends kept                                         */
  int64_t loops;         /* those with map(i) = map(j), before combining, whatever the flag          */
  int64_t entries;       /* nvals(C)                                                                 */
  int32_t clusters;      /* non-empty clusters                                                       */
  int32_t dropped;       /* vertices with map -1                                                     */
  int32_t largest;       /* the largest cluster                                                      */
  int32_t launches;      /* kernel launches of the call: implementation-defined, bench only          */
  float   loop_ms;       /* HIP-event time of the call's device work                                 */
} grb_contract_result;    /* 48 bytes */
grb_info grb_relabel(grb_vector map, grb_vector labels, int kind, int32_t* count, grb_descriptor desc);
grb_info grb_contract(grb_matrix C, grb_vector sizes, grb_matrix A, grb_vector map, grb_binary_op op, int loops,
                      grb_descriptor desc, grb_contract_result* result);

/* Louvain community detection (csrc/louvain.hip): grb_louvain.  The reference has no such driver (graphblas/algorithm/), so
 * the definition is this header's own; cuGraph, networkx, igraph and Grappolo ship the method.  It is the modularity
 * optimisation on top of grb_relabel and grb_contract.  The rule below is deterministic, gives the same bits on any number of
 * CUs, and terminates: it uses exact 64-bit integer arithmetic and integer atomics only, and every accepted round strictly
 * increases the modularity.
 *
 * Input.  A is n x n, f32 or i32, with symmetric structure and values.  weighted = 1 reads the values: an i32 value must be
 * >= 0, an f32 value a non-negative integer value <= 2^24 (grb_maxflow's rule) with -0.0 = +0.0; anything else (negative,
 * fractional, NaN, +-inf, above 2^24) is GRB_INVALID_VALUE.  weighted = 0 never reads the values: every stored entry weighs 1.
 * A stored zero is an entry of weight 0.  A diagonal entry A(v, v) is a loop of that weight.  W = the sum of all stored
 * weights, the diagonal included, each entry once as stored; W must be <= 2^31 - 1, else GRB_INVALID_VALUE: the bound keeps
 * every product below in a signed 64-bit integer.  The weights become i32 once, on the device; every coarser level is i32.
 *
 * Modularity, as an exact integer.  For a partition c: in(x) = the sum of A(i, j) over the stored entries with
 * c(i) = c(j) = x; k(v) = the sum of row v with the diagonal; tot(x) = the sum of k(v) over c(v) = x;
 *   QN = W * sum_x in(x) - sum_x tot(x)^2,   Q = QN / W^2.
 * QN is invariant under contraction with loops kept and PLUS, so every level can be checked exactly.
 *
 * One level works on a graph G with n_G vertices (level 0: A; later: the contraction).  c(v) = v at first, tot(x) = k(x).
 * Rounds 1, 2, ... are
 *   1. Propose.  Every vertex v with a non-empty off-diagonal row computes e(v, x) = the sum of G(v, u) over u != v with
 *      c(u) = x, for its own community a = c(v) and for every neighbouring community.  stay = W e(v, a) - k(v) (tot(a) - k(v)).
 *      For x != a, gain(x) = W e(v, x) - k(v) tot(x) - stay.  v proposes the x with the largest gain, the smallest x on a
 *      tie, and only if that gain is > 0: the proposal (v -> d, g).  All of this reads the state at the start of the round.
 *   2. Claim.  Every proposal claims both a and d.  winner(x) = the claimant with the largest g, the smallest v on a tie.
 *      K(d) = the sum of k(v) over all proposers to d.
 *   3. Accept.  (v -> d, g) is accepted iff winner(c(v)) = v, and either winner(d) = v, or winner(d) itself proposes to
 *      enter d (it is not a vertex leaving d) and g > k(v) (K(d) - k(v)).
 *   4. Apply.  All accepted moves at once, to c and tot.
 * A round without proposals ends the level and counts in rounds; so does reaching max_rounds.
 * Why QN strictly increases: a community with an accepted leaver has no other accepted move touching it, and a destination
 * has no leaver, so every e, tot and stay a mover used is exact but for its co-entrants; the acceptance test charges every
 * pair of co-entrants its worst case k k' to a member that passed the test.  The globally best proposal is always accepted:
 * every round with a proposal moves a vertex, and the level terminates.  (DESIGN.md 5.4s has the derivation.)
 *
 * Levels.  After a level map = grb_relabel(c) and G' = grb_contract(G, map, GRB_OP_PLUS, loops = 1) on i32; the assignment
 * of the original vertices is gathered through map.  The call stops after the first level that accepted no move (it counts
 * in levels; its partition is the one before it) or after max_levels.  labels(v) = the smallest original vertex number in
 * v's final community: the convention of grb_cc, grb_scc and grb_msf.
 *
 * grb_louvain(labels, A, weighted, max_levels, max_rounds, desc, result): labels is an i32 vector of size n and becomes
 * dense.  desc may be NULL; no descriptor field is read.  result may be NULL.
 *
 * Symmetry follows grb_msf's rule: only the CSR is read.  When A has a CSC of its own, one comparison on the device checks the
 * CSR against the CSC: pointers and indices, and with weighted = 1 also the values as bits after -0 has been mapped to +0; a
 * mismatch is GRB_INVALID_VALUE.  An A without a CSC of its own (a product result, the CSR-only matrix format) is taken on the
 * caller's word: whatever it holds, nothing is read or written out of bounds and every level stops after max_rounds rounds;
 * the output is then unspecified.
 *
 * How: the weights are checked and converted, and W and k summed, by plain launches.  A level is ONE co-resident launch of a
 * 1024-thread workgroup per CU (GRB_NUM_CU is honoured) whose passes are separated by a grid barrier with bounded spins; the
 * host reads one record per level.  The propose pass deals the rows by length: up to 8 entries a lane, up to 64 a wave with
 * all pairs compared, up to 256 a wave and up to 2048 the workgroup with an LDS table of (community, 32-bit weight sum)
 * pairs, and beyond that a global array of n_G words per long row in flight, after one more barrier.  From the table on, rows
 * are streamed as 16-byte quads, indices and weights together.  The claim is a 64-bit integer atomicMax of g per touched
 * community and, after a barrier, a 32-bit atomicMin of v among the holders of the maximum; K(d) an integer atomicAdd (K <= W
 * fits 32 bits).  The accept pass decides, the apply pass writes c and tot by integer atomics and clears what the round
 * touched: four barriers a round, five with a long row.  The level's last pass sums in(x) and tot(x)^2.  No floating-point
 * atomics; nothing is allocated inside a level.  Every vertex is evaluated in every round.  Working memory: 44 bytes per
 * vertex of a level, 8 per original vertex, 4 per stored entry of A (the i32 weights), for n > 2048 the count arrays (as many
 * of n words each as fit in 128 MiB, one a CU at most and always at least one, so a single array where n is above 32 M; they
 * are allocated and zeroed once a call whether or not a row is long), and what grb_contract takes between the levels.  None of the constants has been measured; they mirror grb_cdlp's.
 * The worst case is a path: chains of equal gains serialise on the smallest-v tie, as in grb_matching with equal weights.
 *
 * levels, rounds, moves, proposals, communities, qn, w and modularity are exact and independent of scheduling and of
 * GRB_NUM_CU.  modularity = (double)qn / ((double)w * (double)w), 0 when w = 0.
 *
 * Every error is found before labels is written, and labels keeps what it held.  A null labels or A, or an unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square or size(labels) != n: GRB_DIMENSION_MISMATCH; labels not i32, or A outside f32 /
 * i32: GRB_NOT_IMPLEMENTED; an asymmetric A, a bad weight, W > 2^31 - 1, weighted outside {0, 1}, max_levels < 1 or
 * max_rounds < 1: GRB_INVALID_VALUE; a built A with entries but without CSR arrays on the device: GRB_INVALID_OBJECT, as in
 * grb_contract; a failed device allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up: GRB_PANIC,
 * as in the other one-launch drivers.  n = 0, an A without entries, or W = 0 is a success: labels(v) = v, levels = 1,
 * rounds = 1, qn = 0, communities = n. */
typedef struct {
  int64_t qn;            /* W * sum in(x) - sum tot(x)^2 of the final partition                      */
  int64_t w;             /* W: the sum of all stored weights                                         */
  int64_t moves;         /* accepted proposals, all levels                                           */
  int64_t proposals;     /* proposals, all levels                                                    */
  double  modularity;    /* (double)qn / ((double)w * (double)w); 0 when w = 0                       */
  int32_t levels;        /* levels run, the last one that moved nothing included                     */
  int32_t rounds;        /* rounds of all levels, each level's last one included                     */
  int32_t communities;   /* distinct values of labels                                                */
  int32_t passes;        /* grid-wide passes the device ran: implementation-defined, bench only      */
  int32_t launches;      /* co-resident launches: one a level                                        */
  float   loop_ms;       /* HIP-event time of the call's device work                                 */
} grb_louvain_result;     /* 64 bytes */
grb_info grb_louvain(grb_vector labels, grb_matrix A, int weighted, int max_levels, int max_rounds, grb_descriptor desc,
                     grb_louvain_result* result);

/* Random walks and neighbour sampling (csrc/sample.hip): grb_random_walk and grb_sample_neighbors.  The reference has no such
 * drivers (graphblas/algorithm/), so the definitions are this header's own; cuGraph, DGL and PyTorch Geometric ship the two
 * operations.  They draw from a graph instead of computing a function of it, and the randomness is counter-based: every draw
 * is a pure function of (seed, who, when), so the result is the same bits on any number of CUs and in any schedule, and a
 * host restatement (tests/sample_model.py) is compared for equality, not statistically.
 *
 * The draw.  All arithmetic is unsigned 32-bit and wraps.
 *   mix(x):  x ^= x >> 16; x *= 0x85ebca6b; x ^= x >> 13; x *= 0xc2b2ae35; x ^= x >> 16   (grb_matching's finaliser)
 *   draw(seed, a, b) = mix(mix(mix((seed + 0x9e3779b9) ^ a) + b) ^ seed)
 *   pick(r, m) = (uint64(r) * uint64(m)) >> 32, a number in 0 .. m - 1 for 1 <= m <= 2^31 - 1
 * mix is a bijection, so for fixed seed and a, draw is a bijection of b: keys drawn for the positions of one row are distinct.
 *
 * grb_random_walk(walks, A, starts, ns, length, mode, seed, desc, result).  A is n x n, f32 or i32, directed or not; a stored
 * A(i, j) is the step i -> j, the direction grb_bfs walks; a diagonal entry is an ordinary step.  Only the CSR is read, so a
 * product result and the CSR-only format work.  starts is a host array of ns vertices; duplicates are allowed, they are
 * different walkers.  starts == NULL means every vertex 0 .. n - 1 in order, and ns is ignored (ns = n below).  length >= 0 is
 * the number of steps.  walks is an i32 vector of size ns * (length + 1) that becomes dense, walker-major:
 * walks[w * (length + 1) + t] is walker w's vertex after t steps, walks[w * (length + 1)] = starts[w].
 * Step t (counting from 0) of walker w at vertex v, with r = draw(seed, w, t):
 *   mode = GRB_WALK_UNIFORM = 0: the values are never read.  With d = the number of stored entries in row v, the next vertex
 *     is the column of entry pick(r, d) of the row in stored order.
 *   mode = GRB_WALK_WEIGHTED = 1: the values are read under grb_louvain's rule: an i32 value must be >= 0, an f32 value a
 *     non-negative integer value <= 2^24 with -0.0 = +0.0; anything else (negative, fractional, NaN, +-inf, above 2^24) is
 *     GRB_INVALID_VALUE.  S(v) = the sum of row v must be <= 2^31 - 1 for every row, else GRB_INVALID_VALUE.  The next vertex
 *     is the column of the first entry whose inclusive prefix sum in stored order exceeds pick(r, S(v)).  An entry of weight 0
 *     is never taken.
 *   A dead end is a row with d = 0, or in weighted mode S(v) = 0.  The walk stops there, and every later position of that
 *   walker is -1.
 * result may be NULL.  walkers = ns; steps = the transitions made, summed over the walkers; dead_ends = the walkers that
 * stopped early (a walker that merely ends on a vertex without a way out has not): exact, the same on any number of CUs.
 * Every error is found before walks is written, and walks keeps what it held.  Null or unbuilt objects:
 * GRB_UNINITIALIZED_OBJECT; A not square, or size(walks) != ns * (length + 1): GRB_DIMENSION_MISMATCH; a start outside
 * 0 .. n - 1: GRB_INVALID_INDEX, as grb_bc; starts != NULL with ns < 0, length < 0, a mode outside {0, 1}, a bad weight or row
 * sum, or ns * (length + 1) > INT32_MAX: GRB_INVALID_VALUE; walks not i32, or A not f32 / i32: GRB_NOT_IMPLEMENTED; a built A
 * with entries but without CSR arrays on the device: GRB_INVALID_OBJECT; a failed device allocation: GRB_OUT_OF_MEMORY.
 * ns = 0 is a success with nothing written.  desc may be NULL; no descriptor field is read.
 * How: one lane per walker runs all length steps in registers, plain walker-major stores straight into walks' dense storage
 * (after the last check), per-wave counts folded into two 64-bit integer atomics a wave.  Weighted mode first builds a u32
 * array of per-row inclusive prefix sums, 4 bytes per entry, allocated inside the call and freed after it: rows of up to 8
 * entries by a lane, up to 2048 by a wave, longer ones by the workgroup, from the wave on with 16-byte loads and stores; the
 * same pass checks the weights and the row sums (in 64 bits) into a flag word the host reads once.  A weighted step is a
 * binary search in the row's prefix.  Two launches at most, no grid barrier, no floating-point atomics.
 *
 * grb_sample_neighbors(C, A, seeds, ns, fanout, seed, desc, result).  A is nrows x ncols (rectangular is fine), f32 or i32;
 * only the CSR is read.  seeds is a host array of ns row numbers, in any order, duplicates allowed; it may be NULL only when
 * ns = 0 (else GRB_NULL_POINTER).  C is ns x ncols, of A's type.  Row k of C is drawn from row seeds[k] of A, with d its
 * length: if d <= fanout, the whole row; otherwise the fanout entries with the smallest draw(seed, k, p), where p = 0 .. d - 1
 * is the entry's position in the row: uniform sampling without replacement.  The kept entries stay in A's stored order, so
 * the columns ascend, and carry A's value bits unchanged: stored zeros, -0.0 and NaN are copied, nothing is read as a number.
 * The key takes the list position k, not the vertex, so a seed listed twice is sampled twice, independently.  C's row
 * lengths are min(d, fanout), known before any draw: C's pointers come from A's pointers and the library's scan, with no
 * counting pass.  C gets its orientations by the rule grb_contract's C follows: the CSC by the transposition behind
 * grb_transpose where the format keeps one, aliased in the CSR-only format.  C may be A: the result is assembled first.
 * rows = ns, entries = nvals(C), full_rows = the rows copied whole (d <= fanout, empty rows included): exact.
 * On every error C keeps what it held.  Null or unbuilt objects: GRB_UNINITIALIZED_OBJECT; C not ns x ncols:
 * GRB_DIMENSION_MISMATCH; a seed outside 0 .. nrows - 1: GRB_INDEX_OUT_OF_BOUNDS, as grb_matrix_extract; fanout < 1, or
 * ns < 0: GRB_INVALID_VALUE; the types of A and C not both f32 or both i32: GRB_NOT_IMPLEMENTED; a built A with entries but
 * without CSR arrays on the device: GRB_INVALID_OBJECT; more than INT32_MAX entries in the result, or a failed allocation:
 * GRB_OUT_OF_MEMORY.  ns = 0 gives an empty 0 x ncols C.
 * How: keys are recomputed from (seed, k, p) and never loaded or stored.  T, the fanout-th smallest key of a row, is found by
 * a 32-step bisection on the count of keys <= a midpoint (not a radix select: the count is a ballot and a popcount, and a
 * lane's or a wave's row needs no LDS; the two have not been measured against each other), then one pass keeps the entries
 * with key <= T, compacted in stored order by ballot prefix; exactly fanout survive because the keys are distinct.  Rows of
 * up to 8 entries are taken by a lane (ranks among its own keys, no bisection), up to 512 by a wave with eight keys a lane in
 * registers, longer ones by one workgroup looping over the row, keys recomputed in each of the 32 steps.  Two host reads.
 *
 * Out of scope: second-order (node2vec p / q) walks; restarts; weighted sampling without replacement (its usual keys need
 * log, which is not the same bits on the host and the device); sampling with replacement; the multi-hop loop (a caller
 * samples, takes the columns of C as the next seeds, and samples again).  None of the constants has been measured against an
 * alternative. */
#define GRB_WALK_UNIFORM 0
#define GRB_WALK_WEIGHTED 1
typedef struct {
  int64_t walkers;       /* ns                                                                       */
  int64_t steps;         /* transitions made, summed over the walkers                                */
  int64_t dead_ends;     /* walkers that stopped before their last step                              */
  int32_t launches;      /* kernels launched: the walk, and in weighted mode the prefix pass         */
  float   loop_ms;       /* HIP-event time of the call's device work                                 */
} grb_walk_result;        /* 32 bytes */
grb_info grb_random_walk(grb_vector walks, grb_matrix A, const grb_index* starts, int64_t ns, int length, int mode, uint32_t seed,
                         grb_descriptor desc, grb_walk_result* result);
typedef struct {
  int64_t rows;          /* ns                                                                       */
  int64_t entries;       /* nvals(C)                                                                 */
  int64_t full_rows;     /* rows copied whole: d <= fanout                                           */
  int32_t launches;      /* kernels launched for C's CSR: the lengths, the scan, the rows            */
  float   loop_ms;       /* HIP-event time of the call's device work, the CSC included               */
} grb_sample_result;      /* 32 bytes */
grb_info grb_sample_neighbors(grb_matrix C, grb_matrix A, const grb_index* seeds, grb_index ns, int fanout, uint32_t seed,
                              grb_descriptor desc, grb_sample_result* result);

/* Maximum flow and minimum cut (csrc/maxflow.hip): grb_maxflow.  The reference has no such driver (graphblas/algorithm/), so
 * the definition is this header's own; LAGraph ships the algorithm as LAGr_MaxFlow.
 *
 * The network.  A is n x n, f32 or i32, directed: A(i, j) is the capacity of the arc i -> j.  No symmetry is asked for.
 * Diagonal entries take no part.  Antiparallel arcs (both (i, j) and (j, i) stored) are two arcs.  A stored 0 is an arc of
 * capacity 0.  mode selects how the values are read:
 *   GRB_FLOW_CAPACITY = 0   the values are the capacities.  i32 must be >= 0.  f32 must be an integer value in 0 .. 2^24, so
 *                           that it converts exactly.  Anything else off the diagonal (negative, fractional, NaN, +-inf,
 *                           above 2^24) is GRB_INVALID_VALUE.
 *   GRB_FLOW_UNIT     = 1   every stored off-diagonal entry has capacity 1 and the values are never read.  A NaN is fine.
 * The arithmetic is exact: 32-bit residual capacities, 64-bit integer excesses and value (the value may exceed 2^32), and no
 * floating-point atomic anywhere.  Integer atomic adds commute, which is what makes the bits repeat.
 *
 * grb_maxflow(F, side, A, source, sink, mode, desc, result):
 *   result->value   the maximum flow value from source to sink.  It is unique.
 *   side   may be NULL.  Otherwise an i32 vector of size n that becomes dense: side(v) = 1 when sink can be reached from v in
 *          the residual graph of a maximum flow, 0 otherwise.  That set is the smallest sink side of any minimum cut.  It is
 *          the same for every maximum flow and for every maximum preflow, so it is unique and needs no second phase.
 *          side(sink) = 1, side(source) = 0.  The arcs from side 0 to side 1 are a minimum cut, and their capacities sum to
 *          value.
 *   F      may be NULL.  Otherwise n x n and of A's element type; any other type is GRB_DOMAIN_MISMATCH.  F receives a maximum
 *          flow in cancelled form: there is an entry (i, j) only where A has one off the diagonal and the flow on it is
 *          positive, 0 < F(i, j) <= capacity, and never both F(i, j) and F(j, i).  Columns ascending, both orientations built
 *          (the CSC by the transposition behind grb_transpose, or aliased for a CSR-only F).  F may be A.  A maximum flow is
 *          not unique as a mathematical object.  What is promised of F: it is a valid maximum flow (capacity, conservation at
 *          every vertex but the two terminals, net outflow of source = net inflow of sink = value), and the same inputs give
 *          the same bits on any number of CUs, like every other driver here.  When F is NULL the preflow is not converted to
 *          a flow.
 *   desc   may be NULL; no descriptor field is read.  result may be NULL.
 *
 * How: synchronous push-relabel with exact global relabeling.
 *   1. Plain launches build the residual structure: the union of the off-diagonal structures of A and its transpose, rows in
 *      CSR order (A's CSC is read for the reverse arcs, which is why A needs one of its own, as in grb_scc).  Per residual arc:
 *      the other end, the residual capacity (A's capacity, or 0 for a pure reverse arc), the position of the twin arc, and
 *      the position in A or -1.  Every row starts at a multiple of 16 bytes and is filled up to one.
 *   2. ONE co-resident launch of a 1024-thread workgroup per CU (GRB_NUM_CU is honoured) whose passes are separated by a grid
 *      barrier with bounded spins, so launches is 1 whatever the network.  The source's arcs are saturated.  A round:
 *      push     every queued vertex u (excess > 0, not a terminal) walks its row in stored order against the heights and its
 *               excess as they stood at the start of the round, and pushes min(remaining excess, residual) over every arc
 *               with h(u) = h(v) + 1.  Under one snapshot of the heights only one direction of an arc pair can be
 *               admissible, so the pusher alone writes the arc's residual and its twin's, with plain stores; the receiver
 *               takes one 64-bit integer atomicAdd.  A lane walks a row of up to 8 slots, a wave one of up to 2048 with
 *               16-byte loads, the workgroup a longer one; in the latter two the stored-order rule is an exclusive prefix
 *               sum of the admissible residuals (a wave scan, no atomics among the lanes).
 *      relabel  every evaluated vertex and every receiver adds what it received to its excess.  An evaluated vertex that
 *               still has excess takes 1 + the minimum height over its residual arcs: read from the round's array, written
 *               to the next round's.  The pass also queues the next round's vertices; appends are staged per wave in LDS and
 *               reserved with one atomic per batch.
 *      The queue's order may differ from run to run.  Nothing else does: every decision reads the round's snapshot.
 *   3. Global relabeling inside the same launch: a level-synchronous backward BFS from the sink over residual arcs gives exact
 *      heights; with F asked a second one from the source, offset by n, labels what cannot reach the sink; the rest gets the
 *      limit (n without F, 2 n with it) and is not evaluated.  It runs before the first round and whenever n vertices have
 *      been evaluated since the last time: a function of the inputs and the round alone, never of timing or the CU count.
 *   4. The loop ends when the queue is empty.  Without F that is when no vertex with excess has a height below n, so none
 *      reaches the sink: the preflow is maximum.  With F every vertex with excess stays in the loop (heights up to 2 n), so
 *      the remaining excess returns to the source and the preflow becomes a flow.  value = the sink's excess; side = a last
 *      backward BFS from the sink.
 *   5. Plain launches make the outputs: one pass over A's entries for cut_arcs, cut_capacity and sink_side; F by flags, the
 *      library's scan and a write with values max(0, capacity - residual) at A's positions, as select does.  No sort: A's
 *      columns are ascending.  The host reads one record.
 * What bounds it: heights never exceed 2 n, and the kernel leaves with the panic flag if one would; a BFS has at most n
 * levels; the rounds are bounded by 8 n^2 + 4 n + 64 (and by 2^31).  Working memory: 44 bytes per vertex, 16 bytes per
 * residual slot (at most 2 nvals + 3 n slots) and with F 4 bytes per entry of A, one allocation made before the first kernel
 * and freed before the call returns; nothing is allocated inside the loop.  Unlike the other one-launch drivers, the working
 * memory is proportional to nvals: the reverse arcs and the residuals have to live somewhere.  The worst case is a long thin
 * network: a round moves the excess one arc and a global relabeling takes as many barrier-bound passes as the network is deep.
 *
 * value, arcs, flow_arcs, sink_side, cut_arcs and cut_capacity are exact and do not depend on scheduling; rounds,
 * global_relabels, passes and loop_ms are for the bench only.
 *
 * Every error is found before F or side is written, and both keep what they held.  A null or unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, F not n x n, size(side) != n: GRB_DIMENSION_MISMATCH; source or sink outside
 * 0 .. n - 1: GRB_INDEX_OUT_OF_BOUNDS (n = 0 cannot name two terminals, so it falls under this rule); source == sink, a mode
 * outside 0..1, a bad capacity: GRB_INVALID_VALUE; A outside f32 / i32, or side not i32: GRB_NOT_IMPLEMENTED; F not of A's
 * type: GRB_DOMAIN_MISMATCH; an A without a CSC of its own (a product result, the CSR-only format): GRB_INVALID_OBJECT; more
 * than INT32_MAX residual slots: GRB_OUT_OF_MEMORY, as grb_matrix_extract answers an oversized result; a failed device
 * allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up: GRB_PANIC.  No path from source to sink is a success with value
 * 0, an empty F and side = the vertices that reach the sink. */
#define GRB_FLOW_CAPACITY 0
#define GRB_FLOW_UNIT 1
typedef struct {
  int64_t value;            /* the maximum flow value                                                */
  int64_t arcs;             /* stored off-diagonal entries of A                                      */
  int64_t flow_arcs;        /* nvals(F); -1 when F is NULL                                           */
  int64_t sink_side;        /* vertices with side = 1                                                */
  int64_t cut_arcs;         /* arcs from side 0 to side 1                                            */
  int64_t cut_capacity;     /* their capacities, summed after the loop: always equal to value        */
  int32_t rounds;           /* push-relabel rounds: implementation-defined, for the bench only       */
  int32_t global_relabels;  /* global relabelings: implementation-defined, bench only                */
  int32_t passes;           /* grid-wide passes the device ran: implementation-defined, bench only   */
  int32_t launches;         /* kernel launches of the loop itself: 1                                 */
  float   loop_ms;          /* HIP-event time of the call's device work                              */
} grb_maxflow_result;        /* 72 bytes */
grb_info grb_maxflow(grb_matrix F, grb_vector side, grb_matrix A, int64_t source, int64_t sink, int mode, grb_descriptor desc,
                     grb_maxflow_result* result);

/* Biconnected components, articulation points and bridges (csrc/bcc.hip): grb_bcc.  The reference has no such driver
 * (graphblas/algorithm/), so the definition is this header's own; LAGraph does not ship the algorithm either.
 *
 * A is n x n, f32 or i32.  Its structure is symmetric.  Its values are never read, so a stored zero is an edge.  Diagonal
 * entries take no part.
 *   G      = the simple undirected graph of A's off-diagonal entries
 *   block  = a class of the relation "two edges lie on a common simple cycle, or are equal".  A bridge is a block of one
 *            edge.  Every edge is in exactly one block.
 *   key    = (min(u, v), max(u, v)) of the edge {u, v}, compared lexicographically.  The blocks are 0 .. blocks-1,
 *            numbered in ascending order of their smallest edge key.  That numbering is unique, so the same inputs give the
 *            same bits on any number of CUs.
 *   art(v) = the number of blocks that contain v: 0 for a vertex without an off-diagonal entry, 1 for an ordinary vertex,
 *            2 or more exactly when v is an articulation point.  It is v's degree in the block-cut tree.
 *
 * grb_bcc(C, art, A, mode, desc, result):
 *   C      may be NULL.  Otherwise n x n and i32, whatever A's type; any other type is GRB_DOMAIN_MISMATCH.
 *          GRB_BCC_BLOCKS:  C gets A's off-diagonal structure, both directions; the value is the block number of that edge.
 *                           Columns ascend, and isolated vertices have empty rows.
 *          GRB_BCC_BRIDGES: C gets only the entries whose block is a single edge, with the same block numbers as in
 *                           GRB_BCC_BLOCKS mode.
 *          The CSC is a copy of the CSR, unless C is in the CSR-only format.  C may be A when A is i32.
 *   art    may be NULL.  Otherwise an i32 vector of size n that becomes dense.
 *   desc   may be NULL; no descriptor field is read.  result may be NULL.  C and art may both be NULL: only the record is
 *          filled.
 *
 * Structure (the rule of grb_kcore / grb_msf): only the CSR is read.  When A has a CSC of its own, one comparison on the
 * device before the loop checks pointers and indices; a mismatch is GRB_INVALID_VALUE.  An A without a CSC of its own (a
 * product result, the CSR-only matrix format) is taken on the caller's word: whatever it holds, nothing is read or written
 * out of bounds and the call returns -- the levels are bounded by n, the hooking rounds by n + 1 each, every pointer-jumping
 * loop by 40 passes, every column and every preorder number is checked before it is used as an index, and a vertex joins the
 * queue once -- and the output is then unspecified.
 *
 * How: Tarjan-Vishkin on a BFS forest, as ONE co-resident launch of a 1024-thread workgroup per CU (GRB_NUM_CU is honoured)
 * whose passes are separated by a grid barrier with bounded spins; the host reads one record at the end, so launches is 1
 * whatever the graph.  A BFS forest and not an arbitrary spanning forest: its levels make subtree sizes, preorder numbers and
 * low / high plain level-synchronous sweeps (no Euler tour, no list ranking), and a non-tree edge of a BFS tree never joins an
 * ancestor with a descendant.  No floating point appears anywhere.
 *   1. comp(v) = the smallest member of v's connected component: every off-diagonal entry hooks the larger of its ends'
 *      labels (the label's slot and the end itself, atomicMin) onto the smaller, then pointer jumping (up to 16 labels a
 *      vertex and pass), until a round finds every entry's ends agreed.  Rows are walked by a lane up to 8 entries, by a wave
 *      with 16-byte index loads up to 2048, by the workgroup beyond, here and in every row pass below.
 *   2. The vertices with comp(v) = v are the roots and all start at level 0.  ONE queue holds every vertex in level order with
 *      an offset per level.  A level's vertices walk their rows: an unseen neighbour is claimed by a compare-and-swap of its
 *      level and appended (staged per wave in LDS, one reservation per batch), and every neighbour on the next level takes an
 *      atomicMin of the vertex: parent(w) = the smallest-numbered neighbour on the level above, so the forest repeats.
 *   3. size(v), bottom-up by level: children add into their parent (integer atomicAdd).
 *   4. pre(v), top-down by level.  The roots take consecutive ranges of one counter, so pre is a permutation of 0 .. n-1 and
 *      names the tree edge (parent(w), w) as slot pre(w).  A child takes pre(parent) + 1 + its parent's cursor and adds its
 *      size to the cursor: the order of siblings is the order of those atomics.  Every preorder gives the same blocks; the
 *      order reaches nothing that leaves the call except rounds and passes.
 *   5. low(v) / high(v) = min / max of pre(v) and of pre(w) over the non-tree edges {v, w}, over v's subtree: a row walk,
 *      then bottom-up by level with atomicMin / atomicMax into the parent.
 *   6. The auxiliary graph over the slots: (i) a non-tree edge {v, w} joins pre(v) with pre(w); (ii) for v = parent(w), v not
 *      a root, pre(w) joins pre(v) when low(w) < pre(v) or high(w) >= pre(v) + size(v).  Its components by the same minimum
 *      hooking and jumping as in 1, on pre, to the fixpoint: a block's representative is its tree edge of smallest pre, a
 *      child of the block's top vertex.
 *   7. The block of a tree edge is the label of its child's slot, of a non-tree edge the label of the end with the larger
 *      pre.  Per representative an atomicMin of the CSR position over its entries with i < j (rows ascend: position order is
 *      key order) and their count, a thread handing over a run of equal representatives at once.  art(v) = [v is not a root]
 *      + the children c of v whose slot is its own label.  largest, bridges, articulation: integer counts per representative.
 * After the loop the representatives' (smallest position, slot) pairs go through the library's radix sort, at most n of
 * them: a block's number is its rank.  C is a count per row, the library's scan and one writing pass (a wave a row, stored
 * order); GRB_BCC_BRIDGES keeps the entries of blocks with one entry above the diagonal.
 * Working memory: 76 bytes per vertex and 2.5 KiB, one allocation made before the kernel and freed before the call returns;
 * nothing is allocated inside the loop and nothing is proportional to nvals.  The sort brings 12 bytes per block of its own.
 * Passes: four per BFS level (expansion, size, pre, low / high) plus the hooking rounds and their jumps.  Known worst case: a
 * path of a million vertices costs millions of barrier-bound passes, as a long path does in grb_scc.
 *
 * edges, largest, blocks, bridges, articulation, components, isolated and levels are exact and do not depend on scheduling;
 * rounds and passes are for the bench only.
 *
 * Every error is found before C or art is written, and both keep what they held.  A null or unbuilt A:
 * GRB_UNINITIALIZED_OBJECT; A not square, C not n x n, size(art) != n: GRB_DIMENSION_MISMATCH; A outside f32 / i32, or art not
 * i32: GRB_NOT_IMPLEMENTED; C not i32: GRB_DOMAIN_MISMATCH; a mode outside {0, 1}, or an asymmetric A (with a CSC of its own):
 * GRB_INVALID_VALUE; a failed device allocation: GRB_OUT_OF_MEMORY; a grid barrier that gave up: GRB_PANIC.  n = 0 is a success
 * with a zero record.  An A without off-diagonal entries is a success with an empty C, art = 0 everywhere, blocks = 0 and
 * components = isolated = n. */
#define GRB_BCC_BLOCKS  0
#define GRB_BCC_BRIDGES 1
typedef struct {
  int64_t edges;         /* undirected edges of G                                            */
  int64_t largest;       /* edges of the largest block; 0 without edges                      */
  int32_t blocks;        /* biconnected components, bridges included                         */
  int32_t bridges;       /* blocks of one edge                                               */
  int32_t articulation;  /* vertices with art(v) >= 2                                        */
  int32_t components;    /* connected components of G, isolated vertices included            */
  int32_t isolated;      /* vertices without an off-diagonal entry                           */
  int32_t levels;        /* depth of the BFS forest + 1; 0 when n = 0                        */
  int32_t rounds;        /* hooking rounds: implementation-defined, for the bench only       */
  int32_t passes;        /* grid-wide passes: implementation-defined, for the bench only     */
  int32_t launches;      /* kernel launches of the loop itself: 1                            */
  float   loop_ms;       /* HIP-event time of the call's device work                         */
} grb_bcc_result;         /* 56 bytes */
grb_info grb_bcc(grb_matrix C, grb_vector art, grb_matrix A, int mode, grb_descriptor desc, grb_bcc_result* result);

/* ---- The remaining drivers of graphblas/algorithm/  and the two extension
 * operations only they use. */
/* scatter   operations.hpp:748-761 -> backend :1110-1142 (scatter.hpp:10-82): w[(Index)u[k]] = val
 * for every stored u[k] with 0 < u[k] < size(w); masked variants are no-ops as in the reference. */
grb_info grb_scatter(grb_vector w, grb_vector mask, grb_vector u, double val, grb_descriptor desc);
/* graphColor   operations.hpp:816-826 -> backend/cuda/color.hpp:18-88 (cuSPARSE csrcolor there):
 * w = a proper colouring of A's graph, colours from 0; *ncolors (nullable) = colours used. */
grb_info grb_graph_color(grb_vector w, grb_matrix A, grb_descriptor desc, int* ncolors);
/* algorithm::mis (algorithm/mis.hpp:22-141): v = 1 on a maximal independent set chosen by Luby
 * rounds over the int weight vector `weights` (NULL: srand(seed) + rand() per vertex on the host,
 * as apply(set_random) does there, algorithm/common.hpp:8-20).  v, A, weights are int. */
grb_info grb_mis(grb_vector v, grb_matrix A, int seed, grb_vector weights, grb_descriptor desc,
                 grb_algo_result* result);
/* algorithm::gcJP / gcMIS / gcIS (algorithm/gc.hpp:258-421, :152-255, :43-149); algo = --gcalgo
 * (0 JP, 1 MIS, 2 IS).  v = colours from 1. */
grb_info grb_gc(grb_vector v, grb_matrix A, int seed, grb_vector weights, int max_colors, int algo,
                grb_descriptor desc, grb_algo_result* result);
/* algorithm::lgc (algorithm/lgc.hpp:14-176): p = approximate personalised PageRank from s. */
grb_info grb_lgc(grb_vector p, grb_matrix A, grb_index s, double alpha, double eps, grb_descriptor desc,
                 grb_algo_result* result);
/* algorithm::diameter (algorithm/diameter.hpp:14-59): largest BFS eccentricity over the sources
 * s_start..s_end-1 and the last source attaining it; v = the last traversal's depth labels. */
grb_info grb_diameter(grb_vector v, grb_matrix A, grb_index s_start, grb_index s_end, grb_descriptor desc,
                      int* diameter_max, int* diameter_ind);

/* ---- The library's RCCL communicator (the reference has no multi-GPU path:
 * backend/cuda/descriptor.hpp:242,283-284 leave --ndevice unused).  One process per GPU; collectives
 * are enqueued from C++ on a second HIP stream, fenced with events against the stream of
 * grb_set_stream: a collective starts when the work enqueued before it has finished, and the
 * compute stream continues until grb_comm_wait() makes it wait (on the device) for the last one.
 * RCCL is bound with dlopen; GrB_NOT_IMPLEMENTED when it is absent. */
/* Host-staged transport instead of RCCL: the same collectives, each one a callback over pinned HOST buffers (the
 * library waits for its compute stream, stages the data, calls fn, copies the result back).  For ranks that cannot form
 * an RCCL communicator -- several processes on one GPU (the tests drive grb_bfs_part_run / grb_sssp_part_run from two
 * processes this way), a gloo group.  op 0: all-gather of `bytes` per rank, send -> recv[world * bytes]; op 1: in-place
 * all-gather of the byte ranges offsets[r] .. + counts[r] of recv (bytes = the buffer's extent); op 2: sum all-reduce
 * of bytes / 8 doubles in place.  fn returns 0 on success.  fn == NULL switches it off. */
typedef int (*grb_comm_host_fn)(void* user, int op, const void* send, void* recv, long long bytes,
                                const long long* offsets, const long long* counts);
grb_info grb_comm_set_host_transport(int rank, int world, grb_comm_host_fn fn, void* user);
grb_info grb_comm_unique_id(void* out128);                  /* ncclGetUniqueId: rank 0 calls it, every rank gets the bytes */
grb_info grb_comm_init(const void* id128, int rank, int world);
grb_info grb_comm_destroy(void);
grb_info grb_comm_info(int* rank, int* world);               /* world = 0: not initialised */
grb_info grb_comm_wait(void);
grb_info grb_comm_allgather(const void* d_send, void* d_recv, size_t bytes_per_rank);
/* rank r's slice = d_buf[offsets[r] .. +counts[r]) bytes, in place; afterwards every rank holds all slices */
grb_info grb_comm_allgatherv_inplace(void* d_buf, const long long* offsets, const long long* counts);
grb_info grb_comm_allreduce_sum_f64(void* d_buf, size_t count);
grb_info grb_comm_timing(int on);                            /* HIP-event time of every collective (adds a host wait) */
grb_info grb_comm_stats(double* total_us, long long* calls, int reset);
/* element-wise tail of a PageRank iteration on a chunk of owned rows (algorithm/pr.hpp:70-80):
 * p_next = y + c, *d_acc (double) += sum (p_next - p_old)^2 */
grb_info grb_pr_part_update(const void* d_y, const void* d_p_old, float c, void* d_p_next, grb_index n, void* d_acc);
/* The whole iteration loop of algorithm::pr (algorithm/pr.hpp:52-90) on this rank's in-edge shard, cut into nchunks
 * row chunks: chunk c's slice of the next vector is all-gathered (library communicator, if one is up) while chunk
 * c + 1 is multiplied; the squared residual is all-reduced and read once per iteration -- the only host read.
 * chunks[c]: local rows [row_cut[c], row_cut[c+1]) x n, values alpha / outdeg; vertex_cut: [world][nchunks+1] global
 * vertex ids of every rank's chunk boundaries; lo: this rank's first vertex; c_add = (1 - alpha) / n.
 * d_p_cur (initial vector) / d_p_next: n floats; d_y: n_local floats; d_acc: one double.
 * errors (may be NULL): max_niter doubles; *result_in_next: 1 when the result is in d_p_next. */
grb_info grb_pr_part_run(int nchunks, const grb_matrix* chunks, const long long* row_cut, const long long* vertex_cut,
                         grb_index lo, float c_add, float eps, int max_niter, void* d_p_cur, void* d_p_next, void* d_y,
                         void* d_acc, int* iterations, double* errors, int* result_in_next);

/* ---- Raw kernels on plain device pointers (micro-benchmarks / multi-GPU shards) --- */
/* Generic semiring SpMV  w[i] = (+)_j A[i,j] (x) u[j] on this matrix's CSR (tran=0) or
 * CSC (tran=1) arrays: the kernel behind the pull branch (backend/cuda/spmv.hpp:178-220).
 * mask may be NULL. */
grb_info grb_k_spmv(grb_matrix A, int tran, grb_semiring op, const void* d_u, const void* d_mask,
                    int scmp, int accum, void* d_w);
/* Algorithmic bytes of one grb_k_spmv launch: 8*nnz + 12*n + 4. */
int64_t grb_k_spmv_bytes(grb_matrix A, int tran);

#ifdef __cplusplus
}
#endif
#endif  /* GRB_HIP_H_ */
