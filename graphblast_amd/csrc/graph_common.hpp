// graph_common.hpp -- the helpers the graph algorithms share (ktruss, bc, cdlp, lcc, kcore, scc, msf, matching, contract,
// maxflow, bcc): searches in a row, the order of weights, the structural-symmetry check, a wave's staged appends, the split
// of a row into 16-byte quads, the weight sum's fixed-order tail; and on the host the event pair, padding, result arrays,
// and the dense output vector (the occupancy check: persist_common.hpp).  The tuning constants (k*LaneLen, k*WaveLen, k*Stage), the row dealers
// and the persistent kernels' bodies stay in their files: each algorithm is retuned alone.
#pragma once
#include "persist_common.hpp"

namespace grb {

// ---- device: searches in a row (index_lower_bound: common.hpp) ------------------------------------------------------------
// the length of v's row (or column) without a stored diagonal
__device__ __forceinline__ int row_degree_no_diag(const Index* __restrict__ ptr, const Index* __restrict__ ind, Index v) {
  const Index b = ptr[v], e = ptr[v + 1];
  const Index lo = index_lower_bound(ind, b, e, v);
  const int d = (int)(e - b) - (lo < e && ind[lo] == v ? 1 : 0);
  return d > 0 ? d : 0;
}

// ---- device: the order of values -------------------------------------------------------------------------------------------
// the monotone map of a value's bits to an unsigned (f32: -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; i32 as a signed
// integer) and back.  Every bit pattern keeps its own key: contract.hip folds with it and must return the bits it was given.
__device__ __forceinline__ unsigned value_order(unsigned b, int f32) {
  if (!f32) return b ^ 0x80000000u;
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ unsigned value_unorder(unsigned o, int f32) {
  if (!f32) return o ^ 0x80000000u;
  return (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
}
// ... and of a weight: by value, so -0 = +0 (msf.hip and matching.hip compare edges, and the two rows of an edge may differ
// in the sign of a zero)
__device__ __forceinline__ unsigned weight_canon(unsigned b, int f32) { return f32 && b == 0x80000000u ? 0u : b; }
__device__ __forceinline__ unsigned weight_order(unsigned b, int f32) {
  if (!f32) return b ^ 0x80000000u;
  return value_order(weight_canon(b, 1), 1);
}

// ---- device: the 32-bit finaliser ------------------------------------------------------------------------------------------
// a bijection of the 32-bit words that spreads every input bit over the output (matching.hip's hashed priorities, sample.hip's
// draws).  Its bits are part of both definitions (include/grb_hip.h): they must not change.
__device__ __forceinline__ unsigned hash_mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// ---- the structural-symmetry check -------------------------------------------------------------------------------------------
// flag |= 1 when the CSR and the CSC differ (a symmetric matrix has the same arrays both ways): pointers, indices and, with
// kValues, values as bits with -0 taken as +0
template <bool kValues>
static __global__ __launch_bounds__(kBlock) void symmetric_compare_kernel(const Index* __restrict__ a_ptr, const Index* __restrict__ b_ptr,
                                                                          long long n1, const Index* __restrict__ a_ind,
                                                                          const Index* __restrict__ b_ind, const unsigned* __restrict__ a_val,
                                                                          const unsigned* __restrict__ b_val, long long nnz, int f32,
                                                                          unsigned int* __restrict__ flag) {
  bool bad = false;
  for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n1 + nnz; i += (long long)gridDim.x * kBlock) {
    if (i < n1) bad |= a_ptr[i] != b_ptr[i];
    else bad |= a_ind[i - n1] != b_ind[i - n1] || (kValues && weight_canon(a_val[i - n1], f32) != weight_canon(b_val[i - n1], f32));
  }
  if (__ballot(bad) != 0ull && lane_id() == 0) atomicOr(flag, 1u);
}
// one launch on s, or none: a matrix whose CSC is its CSR (the CSR-only format) or is missing has nothing to compare.
// (A template, so that a file holds only the instantiations it launches.)
template <bool kValues>
inline void launch_symmetry_check(const grb_matrix_s* A, unsigned int* flag, hipStream_t s) {
  if (A->csc_alias || A->csc.ptr == nullptr) return;
  const long long n1 = (long long)A->nrows + 1, nnz = (long long)A->nvals;
  hipLaunchKernelGGL(symmetric_compare_kernel<kValues>, dim3(stream_grid(n1 + nnz)), dim3(kBlock), 0, s, A->csr.ptr, A->csc.ptr, n1, A->csr.ind,
                     A->csc.ind, (const unsigned*)A->csr.val, (const unsigned*)A->csc.val, nnz, A->dtype == GRB_F32 ? 1 : 0, flag);
}

// ---- device: a wave's staged appends ---------------------------------------------------------------------------------------
// A wave collects what it appends in LDS and reserves room for a whole stage with one atomic.  cnt is the same in every lane;
// every lane of the wave calls these together.  (msf.hip stages two payloads an element and keeps its own.)
struct WaveStage {
  Index* stage;                     // the wave's stage (LDS)
  unsigned cnt;                     // staged
  Index* dst;                       // where the wave appends: dst[base + ...], below cap
  unsigned* counter;                // what has been appended behind base
  unsigned base, cap;
};
__device__ __forceinline__ void stage_flush(WaveStage& o, int lane) {
  if (o.cnt == 0u) return;
  const unsigned cnt = o.cnt;
  __builtin_amdgcn_wave_barrier();
  unsigned at = 0;
  if (lane == 0) at = atomicAdd(o.counter, cnt);
  at = o.base + (unsigned)__shfl((int)at, 0, kWave);
  for (unsigned i = (unsigned)lane; i < cnt; i += kWave)
    if (at + i < o.cap) publish(&o.dst[at + i], o.stage[i]);                 // (always: an element is appended once)
  __builtin_amdgcn_wave_barrier();
  o.cnt = 0u;
}
template <int kStage>
__device__ __forceinline__ void stage_push(WaveStage& o, int lane, bool want, Index v) {
  const unsigned long long m = __ballot(want);
  if (m == 0ull) return;
  if (o.cnt + kWave > (unsigned)kStage) stage_flush(o, lane);
  if (want) o.stage[o.cnt + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = v;
  o.cnt += (unsigned)__popcll(m);
}

// ---- device: a row as 16-byte quads ----------------------------------------------------------------------------------------
// [b, e) of ind: up to three entries before the first 16-byte boundary, whole quads, up to three entries behind them
struct QuadSpan {
  Index b4, nq, te;                 // the first quad's position, the quads, the first position behind them
  Index nh, ns;                     // the entries in front, and in front and behind together
};
__device__ __forceinline__ QuadSpan quad_span(const Index* ind, Index b, Index e) {
  QuadSpan q;
  q.b4 = b + (Index)((4u - (unsigned)((reinterpret_cast<uintptr_t>(ind + b) >> 2) & 3u)) & 3u);
  if (q.b4 > e) q.b4 = e;
  q.nq = (e - q.b4) >> 2;
  q.te = q.b4 + 4 * q.nq;
  q.nh = q.b4 - b;
  q.ns = q.nh + (e - q.te);
  return q;
}

// ---- the weight sum's fixed-order tail ---------------------------------------------------------------------------------------
// A weight is a two-level sum whose shape depends on the number of items alone, so that it is the same number every time:
// the threads' sums by a fixed butterfly, the waves' in order by thread 0, the blocks' in order by the final kernel.
// kF32: f64 sums; else exact 64-bit integer sums.  A kBlock-thread workgroup; every thread calls it.
template <bool kF32>
__device__ __forceinline__ void weight_block_sum(double fs, long long is, unsigned long long* __restrict__ partial) {
  __shared__ unsigned long long s_part[kWavesPerBlock];
  for (int s = kWave / 2; s > 0; s >>= 1) {
    if (kF32) fs += __shfl_xor(fs, s, kWave);
    else is += __shfl_xor(is, s, kWave);
  }
  if (lane_id() == 0) s_part[wave_id()] = kF32 ? (unsigned long long)__double_as_longlong(fs) : (unsigned long long)is;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kWavesPerBlock; ++w) {
      if (kF32) fs += __longlong_as_double((long long)s_part[w]);
      else is += (long long)s_part[w];
    }
    partial[blockIdx.x] = kF32 ? (unsigned long long)__double_as_longlong(fs) : (unsigned long long)is;
  }
}
template <bool kF32>
static __global__ void weight_final_kernel(const unsigned long long* __restrict__ partial, int blocks, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double fs = 0.0;
  long long is = 0;
  for (int b = 0; b < blocks; ++b) {
    if (kF32) fs += __longlong_as_double((long long)partial[b]);
    else is += (long long)partial[b];
  }
  *out = kF32 ? fs : (double)is;
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// the two events around a call's device work
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  grb_info create() {
    GRB_HIP_TRY(hipEventCreate(&a));
    GRB_HIP_TRY(hipEventCreate(&b));
    return GRB_SUCCESS;
  }
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};

// every array of a call's one allocation begins on a 256-byte line: a count of 4-byte words, or of bytes, rounded up
inline size_t pad_words(size_t words) { return (words + 63) & ~(size_t)63; }
inline size_t pad_bytes(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the bits of a sort key that holds numbers below dim: 1 .. 32.  An Index dimension is below 2^31 and needs 31 at most.
inline int key_bits(long long dim) {
  int b = 1;
  while (b < 32 && ((long long)1 << b) < dim) ++b;
  return b;
}

// a result's arrays for n rows and m entries, exactly
inline grb_info side_alloc(Side* sd, Index n, long long m) {
  GRB_TRY(ewm_alloc(&sd->ptr, 4 * ((size_t)n + 1)));
  GRB_TRY(ewm_alloc(&sd->ind, 4 * (size_t)(m > 0 ? m : 1)));
  GRB_TRY(ewm_alloc(&sd->val, 4 * (size_t)(m > 0 ? m : 1)));
  sd->nnz = (Index)m;
  sd->h_ptr.assign((size_t)n + 1, 0);
  return GRB_SUCCESS;
}
// the CSC of a symmetric result is a copy of its CSR (the device arrays; h_ptr is the caller's, once the CSR's has arrived)
inline grb_info side_mirror(Side* csc, const Side& csr, Index n, long long m, hipStream_t s) {
  GRB_HIP_TRY(hipMemcpyAsync(csc->ptr.p, csr.ptr.p, 4 * ((size_t)n + 1), hipMemcpyDeviceToDevice, s));
  if (m > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(csc->ind.p, csr.ind.p, 4 * (size_t)m, hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipMemcpyAsync(csc->val.p, csr.val.p, 4 * (size_t)m, hipMemcpyDeviceToDevice, s));
  }
  return GRB_SUCCESS;
}

// A dense output vector of n 4-byte values, in two steps.  prepare, before anything runs: the vector has dense storage from
// here on (allocated only where it has none yet) and is otherwise as it was.  commit, after everything that can fail: the
// values are copied in and the vector is dense.  Nothing of the caller's vector changes in between.
inline grb_info dense_out_prepare(grb_vector v, Index n) {
  const int old_type = v->vec_type;
  const grb_info si = grb_vector_set_storage(v, GRB_DENSE);
  v->vec_type = old_type;
  if (si != GRB_SUCCESS) return si;
  return n > 0 && !v->d_val ? GRB_OUT_OF_MEMORY : GRB_SUCCESS;
}
inline grb_info dense_out_commit(grb_vector v, const void* src, Index n, hipStream_t s) {
  if (n > 0) {
    GRB_HIP_TRY(hipMemcpyAsync(v->d_val, src, 4 * (size_t)n, hipMemcpyDeviceToDevice, s));
    GRB_HIP_TRY(hipStreamSynchronize(s));
  }
  v->vec_type = GRB_DENSE;
  v->d_nnz = n;
  return GRB_SUCCESS;
}

}  // namespace grb
